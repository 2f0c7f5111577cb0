"""NumPy restatement of the sparse matcher (bf_matcher_*: descriptor matching, the Kabsch key-point match filter,
filterFrames, AddCurrToResiduals) and a synthetic key-point generator. The checker of tests/test_match*.py.

Float decisions cannot be bit-equal across acosf implementations, so the restatement marks what sits on a
threshold: a key (row or column) is *borderline* when the relative margin of either acceptance comparison is below
1e-5; a pair is *borderline* for the filter when a residual (against maxKabschRes2), a pixel distance (against 5)
or a condition ratio (against 100) comes within 1 % of its threshold. Exact comparisons skip borderline items; the
fixtures are chosen so that there are (almost) none, and the CPU tests assert that.
"""
from __future__ import annotations

import numpy as np

MAX_RAW, MAX_FILT = 128, 25
KEY_MARGIN, FILTER_MARGIN = 1e-5, 1e-2
F32 = np.float32


# ---- stage 2: descriptor matching -----------------------------------------------------------------------------
def dots(dp: np.ndarray, dc: np.ndarray) -> np.ndarray:
    return dp.astype(np.int64) @ dc.astype(np.int64).T


def best_next_arg(D: np.ndarray):
    """Per row: best (from 0, index -1, strict >), lowest argument, max over the others (= best on a tie)."""
    n, m = D.shape
    arg = D.argmax(1)
    best = D[np.arange(n), arg]
    E = D.copy()
    E[np.arange(n), arg] = -1
    nxt = np.maximum(E.max(1), 0) if m > 0 else np.zeros(n, np.int64)
    zero = best <= 0
    return np.where(zero, 0, best), np.where(zero, 0, nxt), np.where(zero, -1, arg)


def dist_of(dot):
    return np.arccos(np.minimum(np.asarray(dot, np.float64) * 2.0 ** -18, 1.0))


def _rel_margin(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.abs(a - b) / np.abs(b)
    return np.where((a == 0) & (b == 0), np.inf, m)  # 0 < 0 is exactly false on any implementation


def accept(best, nxt, arg, thresh, ratio):
    """(result index or -1, distance, borderline flag) per key."""
    thresh, ratio = float(F32(thresh)), float(F32(ratio))
    d, dn = dist_of(best), dist_of(nxt)
    ok = (d < thresh) & (d < dn * ratio) & (arg >= 0)
    border = (_rel_margin(d, thresh) < KEY_MARGIN) | (_rel_margin(d, dn * ratio) < KEY_MARGIN)
    return np.where(ok, arg, -1), d, border & (arg >= 0)


def match_pair(dp: np.ndarray, dc: np.ndarray, thresh=0.7, ratio=0.8):
    """Raw list of one pair: dict(count, idx [k, 2] image-local (prev key, cur key), dist [k], dot [k]) in the
    matcher's order (dot descending, cur key ascending), k = min(count, 128); border_rows / border_cols."""
    if len(dp) == 0 or len(dc) == 0:
        return dict(count=0, idx=np.zeros((0, 2), np.int64), dist=np.zeros(0), dot=np.zeros(0, np.int64),
                    border_rows=np.zeros(len(dp), bool), border_cols=np.zeros(len(dc), bool), D=None,
                    rows=(np.zeros(len(dp), np.int64),) * 3)
    D = dots(dp, dc)
    rb, rn, ra = best_next_arg(D)
    cb, cn, ca = best_next_arg(D.T)
    rres, rdist, rborder = accept(rb, rn, ra, thresh, ratio)
    cres, _, cborder = accept(cb, cn, ca, thresh, ratio)
    out = []
    for b in range(len(dc)):
        f1 = cres[b]
        if f1 >= 0 and rres[f1] == b:
            out.append((int(f1), b, int(rb[f1]), float(rdist[f1])))
    out.sort(key=lambda t: (-t[2], t[1]))
    count = len(out)
    out = out[:MAX_RAW]
    return dict(count=count, idx=np.array([(a, b) for a, b, _, _ in out], np.int64).reshape(-1, 2),
                dist=np.array([d for _, _, _, d in out]), dot=np.array([v for _, _, v, _ in out], np.int64),
                border_rows=rborder, border_cols=cborder, D=D, rows=(rb, rn, ra))


# ---- stage 3: key-point match filter --------------------------------------------------------------------------
def key_points32(keys: np.ndarray, kinv) -> np.ndarray:
    """intrinsicsInv * (depth * (x, y, 1)) in float32, in the library's operation order: [n, 3] float32."""
    k = np.asarray(kinv, F32).reshape(4, 4)
    keys = np.asarray(keys, F32).reshape(-1, 4)
    d = keys[:, 3]
    v = np.stack([d * keys[:, 0], d * keys[:, 1], d * F32(1.0)], 1).astype(F32)
    out = np.empty((len(keys), 3), F32)
    for r in range(3):
        out[:, r] = ((k[r, 0] * v[:, 0] + k[r, 1] * v[:, 1]) + k[r, 2] * v[:, 2]) + k[r, 3] * F32(1.0)
    return out


def kabsch(src: np.ndarray, tgt: np.ndarray):
    """Rigid transform src -> tgt (4x4) and the cross-covariance's largest / second singular value."""
    p0, q0 = src.mean(0), tgt.mean(0)
    H = (src - p0).T @ (tgt - q0) / len(src)
    U, S, Vt = np.linalg.svd(H)
    W = Vt.T
    d = 1.0 if np.linalg.det(W @ U.T) >= 0 else -1.0
    R = W @ np.diag([1.0, 1.0, d]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = q0 - R @ p0
    with np.errstate(divide="ignore", invalid="ignore"):
        c1 = S[0] / S[1]
    return T, c1


def _cov_ratio(p: np.ndarray) -> float:
    c = (p - p.mean(0)).T @ (p - p.mean(0)) / len(p)
    ev = np.linalg.eigvalsh(c)[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return ev[0] / ev[1]


class _Filter:
    def __init__(self, keys, kinv, min_matches, max_res2):
        self.keys = np.asarray(keys, F32).reshape(-1, 4)
        self.kinv, self.min_matches, self.max_res = kinv, min_matches, float(F32(max_res2))
        self.border = False
        self.T = np.eye(4)

    def _near(self, v, t):
        if np.isfinite(v) and abs(v - t) < FILTER_MARGIN * t:
            self.border = True

    def reproject(self, n):
        """ComputeReprojection on the first n entries of self.idx / self.dist; returns validity."""
        pts = key_points32(self.keys[self.idx[:n].ravel()], self.kinv).astype(np.float64).reshape(n, 2, 3)
        src, tgt = pts[:, 0], pts[:, 1]
        self.T, c1 = kabsch(src, tgt)
        res = (((src @ self.T[:3, :3].T + self.T[:3, 3]) - tgt) ** 2).sum(1)
        order = list(range(n))
        res = list(res)
        for i in range(n):  # the reference's exchange sort
            for j in range(i, n):
                if res[i] > res[j]:
                    res[i], res[j] = res[j], res[i]
                    order[i], order[j] = order[j], order[i]
        self.idx[:n] = self.idx[:n][order]
        self.dist[:n] = self.dist[:n][order]
        self.res[:n] = res
        cp, cq = _cov_ratio(src), _cov_ratio(tgt)
        for c in (c1, cp, cq):
            self._near(abs(c), 100.0)
        return not (np.isnan(c1) or np.isnan(cp) or np.isnan(cq) or abs(c1) > 100 or abs(cp) > 100 or abs(cq) > 100)

    def add_match(self, add, cur):
        a_i, a_j = self.keys[add[0], :2].astype(np.float64), self.keys[add[1], :2].astype(np.float64)
        ok = True
        for i in range(cur):
            for d in (np.linalg.norm(a_i - self.keys[self.idx[i, 0], :2]), np.linalg.norm(a_j - self.keys[self.idx[i, 1], :2])):
                self._near(d, 5.0)
                if d <= 5.0:
                    ok = False
            if not ok:
                break
        return ok

    def run(self, idx, dist):
        self.idx = np.array(idx, np.int64).reshape(-1, 2).copy()
        self.dist = np.array(dist, np.float64).copy()
        self.res = np.zeros(max(len(self.idx), 1))
        num_raw, i, cur = len(self.idx), 0, 0
        cur_max, valid = 100.0, False
        while True:
            if i == num_raw or cur >= MAX_FILT:
                if cur >= 3:
                    self._near(cur_max, self.max_res)
                if cur < self.min_matches or cur_max >= self.max_res or not valid:
                    cur = 0
                break
            add = self.idx[i].copy()
            if self.add_match(add, cur):
                self.idx[cur] = add
                self.dist[cur] = self.dist[i]
                cur += 1
                if cur >= 3:
                    valid = self.reproject(cur)
                    b, prev_t = valid, self.T.copy()
                    cur_max = self.res[cur - 1]
                    self._near(cur_max, self.max_res)
                    if cur_max > self.max_res:
                        last = -1.0
                        for k in range(cur - 1, 2, -1):
                            last = self.res[k]
                            cur -= 1
                            valid = self.reproject(cur)
                            cur_max = self.res[cur - 1]
                            self._near(cur_max, self.max_res)
                            if cur == 3 and (cur_max > self.max_res or (b and not valid)):
                                cur += 1
                                cur_max, valid, self.T = last, b, prev_t
                                break
                            if cur_max < self.max_res:
                                break
            i += 1
        return cur


def filter_pair(keys, idx, dist, kinv, min_matches=5, max_res2=0.0004):
    """filterKeyPointMatches on a raw list (global key indices, sorted by distance): dict(count, idx, dist, T,
    border)."""
    f = _Filter(keys, kinv, min_matches, max_res2)
    n = f.run(idx, dist) if len(idx) else 0
    return dict(count=n, idx=f.idx[:n].copy() if len(idx) else np.zeros((0, 2), np.int64),
                dist=f.dist[:n].copy() if len(idx) else np.zeros(0), T=f.T, border=f.border)


# ---- stages 2-4 over an image store ---------------------------------------------------------------------------
def run(images, cur, start, valid, kinv, thresh=0.7, ratio=0.8, min_matches=5, max_res2=0.0004):
    """images: list of (keys [n, 4] float32, descs [n, 128] uint8). Returns dict(pairs {prev: dict(raw, filt)},
    last, valid_cur, entries [(prev, cur, key_i, key_j)])."""
    offs = np.concatenate([[0], np.cumsum([len(k) for k, _ in images])]).astype(np.int64)
    all_keys = np.concatenate([np.asarray(k, F32).reshape(-1, 4) for k, _ in images]) if images else np.zeros((0, 4), F32)
    pairs = {}
    for prev in range(start, len(images)):
        if prev == cur:
            continue
        if not valid[prev] or len(images[prev][0]) == 0 or len(images[cur][0]) == 0:
            raw = match_pair(np.zeros((0, 128), np.uint8), np.zeros((0, 128), np.uint8))
            raw["border_rows"] = np.zeros(len(images[prev][0]), bool)
            raw["border_cols"] = np.zeros(len(images[cur][0]), bool)
        else:
            raw = match_pair(images[prev][1], images[cur][1], thresh, ratio)
        gidx = raw["idx"] + np.array([offs[prev], offs[cur]])
        raw["gidx"] = gidx
        filt = filter_pair(all_keys, gidx, raw["dist"], kinv, min_matches, max_res2)
        pairs[prev] = dict(raw=raw, filt=filt)
    last = 0xFFFFFFFF
    for i in range(len(images) - 1, start - 1, -1):
        if i != cur and valid[i] and pairs[i]["filt"]["count"] > 0:
            last = i
            break
    entries = [(prev, cur, int(a), int(b)) for prev in sorted(pairs) for a, b in pairs[prev]["filt"]["idx"]]
    return dict(pairs=pairs, last=last, valid_cur=last != 0xFFFFFFFF, entries=entries, offsets=offs, keys=all_keys)


# ---- synthetic generator ----------------------------------------------------------------------------------------
FX, FY, CX, CY, WIDTH, HEIGHT = 580.0, 580.0, 319.5, 239.5, 640, 480


def intrinsics_inv() -> np.ndarray:
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = FX, FY, CX, CY
    return np.linalg.inv(K).astype(F32)


def sift_like(rng, n, base=None, noise=0.0):
    """Non-negative, unit norm, clamped at 0.2, renormalised, floor(512 v + 0.5) (SiftGPU's byte descriptor)."""
    v = rng.gamma(0.5, 1.0, size=(n, 128)) if base is None else base + rng.normal(0.0, noise, size=base.shape)
    v = np.maximum(v, 0.0)
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    v = np.minimum(v, 0.2)
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)
    return v, np.minimum(np.floor(512.0 * v + 0.5), 255).astype(np.uint8)


def pose(k: int, step=0.05, rot=0.03) -> np.ndarray:
    """Camera -> world of image k: a slow arc."""
    a = rot * k
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T[:3, 3] = [step * k, 0.01 * k, -0.02 * k]
    return T


def project(T_c2w, pts):
    w2c = np.linalg.inv(T_c2w)
    p = pts @ w2c[:3, :3].T + w2c[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = FX * p[:, 0] / p[:, 2] + CX, FY * p[:, 1] / p[:, 2] + CY
    inside = (p[:, 2] > 0.4) & (u >= 0) & (u <= WIDTH - 1) & (v >= 0) & (v <= HEIGHT - 1)
    return u, v, p[:, 2], inside


def make_images(seed, key_counts, n_landmarks=None, n_wrong=0, share=0.6, desc_noise=0.02, poses=None, keep=None,
                wrong_noise=None, pts=None):
    """Images of a random landmark cloud. Per image: the landmarks in view (a `keep[i]` fraction of them, at most
    share * n) projected exactly with depth = camera z and a re-noised descriptor, `n_wrong` of them planted at
    another 3-D point (same descriptor: a perfect but geometrically wrong match), distractor keys with fresh
    descriptors up to the key count, order shuffled. Returns (images, truth) with truth[i] = landmark id per key
    (-1 distractor, -2 - id planted wrong)."""
    rng = np.random.default_rng(seed)
    n_img = len(key_counts)
    n_landmarks = n_landmarks or max(8, int(max(key_counts) * 0.9))
    box = np.stack([rng.uniform(-1.6, 1.9, n_landmarks), rng.uniform(-1.1, 1.1, n_landmarks),
                    rng.uniform(1.6, 3.6, n_landmarks)], 1)
    pts = box if pts is None else np.asarray(pts, np.float64)
    n_landmarks = len(pts)
    alt = pts + rng.uniform(0.25, 0.5, pts.shape) * rng.choice([-1.0, 1.0], pts.shape)
    base, _ = sift_like(rng, n_landmarks)
    poses = poses if poses is not None else [pose(k) for k in range(n_img)]
    images, truth = [], []
    for i, n in enumerate(key_counts):
        u, v, z, inside = project(poses[i], pts)
        vis = np.flatnonzero(inside)
        rng.shuffle(vis)
        frac = 1.0 if keep is None else keep[i]
        vis = vis[: min(int(len(vis) * frac), int(np.ceil(share * n)))]
        ids = list(vis)
        wrong = set(ids[: min(n_wrong, len(ids))])
        keys, lab = [], []
        for l in ids:
            if l in wrong:
                ua, va, za, ok = project(poses[i], alt[l:l + 1])
                if not ok[0]:
                    continue
                keys.append((ua[0], va[0], 1.0, za[0]))
                lab.append(-2 - l)
            else:
                keys.append((u[l], v[l], 1.0, z[l]))
                lab.append(l)
        lm = np.array([l if l >= 0 else -2 - l for l in lab], np.int64)
        noise = np.full(len(lm), desc_noise)
        if wrong_noise is not None:
            noise[np.array(lab) < 0] = wrong_noise
        d_shared = sift_like(rng, len(lm), base[lm], noise[:, None])[1] if len(lm) else np.zeros((0, 128), np.uint8)
        nd = n - len(lm)
        kd = np.stack([rng.uniform(0, WIDTH - 1, nd), rng.uniform(0, HEIGHT - 1, nd), np.ones(nd), rng.uniform(0.5, 4.0, nd)], 1)
        dd = sift_like(rng, nd)[1]
        K = np.concatenate([np.array(keys, np.float64).reshape(-1, 4), kd]).astype(F32)
        Dm = np.concatenate([d_shared, dd])
        L = np.concatenate([np.array(lab, np.int64), -np.ones(nd, np.int64)])
        perm = rng.permutation(n)
        images.append((np.ascontiguousarray(K[perm]), np.ascontiguousarray(Dm[perm])))
        truth.append(L[perm])
    return images, truth


def borderline_fraction(images, cur, start, valid, thresh=0.7, ratio=0.8):
    """(borderline keys, keys looked at) over every pair of a match call."""
    b = t = 0
    for prev in range(start, len(images)):
        if prev == cur or not valid[prev] or len(images[prev][0]) == 0 or len(images[cur][0]) == 0:
            continue
        r = match_pair(images[prev][1], images[cur][1], thresh, ratio)
        b += int(r["border_rows"].sum() + r["border_cols"].sum())
        t += len(r["border_rows"]) + len(r["border_cols"])
    return b, t


def rot_diff(Ra, Rb) -> float:
    """Angle between two rotations from the chord |Ra - Rb|_F = 2 sqrt(2) sin(theta / 2) (resolves ~1e-7 rad)."""
    chord = np.linalg.norm(np.asarray(Ra, np.float64)[:3, :3] - np.asarray(Rb, np.float64)[:3, :3]) / (2.0 * np.sqrt(2.0))
    return float(2.0 * np.arcsin(min(1.0, chord)))


# ---- the fixtures of tests/test_match_gpu.py (tests/test_match.py asserts their borderline conditions) ---------
RAW_SHAPES = [(1, 1), (31, 33), (100, 65), (33, 257), (1024, 1000)]
RAW_SEEDS = {(1, 1): 3, (31, 33): 3, (100, 65): 3, (33, 257): 3, (1024, 1000): 1}


def raw_fixture(shape):
    """Two images of shape = (n_prev, n_cur) keys; the pair (0, 1)."""
    if shape == (1, 1):  # one landmark seen by both
        return make_images(RAW_SEEDS[shape], [1, 1], share=1.0, pts=[[0.2, 0.1, 2.5]])[0]
    return make_images(RAW_SEEDS[shape], list(shape))[0]


STORE6_COUNTS = [100, 0, 65, 257, 33, 120]
STORE6_INVALID = 2


def store6_fixture():
    """6 images with an empty one (1) and one to invalidate (2)."""
    return make_images(5, STORE6_COUNTS)[0]


def filter_fixture():
    """6 images of differing overlap with planted wrong matches (noisier descriptors, so they sort late)."""
    return make_images(7, [220, 200, 180, 240, 160, 230], n_landmarks=260, n_wrong=6, keep=[1.0, 0.8, 0.5, 0.9, 0.3, 1.0],
                       wrong_noise=0.035)[0]


E2E_KEYS = 300


def e2e_fixture(poses):
    """Exact, noise-free key points of landmarks spread over every camera's frustum (poses: camera -> world)."""
    rng = np.random.default_rng(11)
    pts = []
    for T in poses:
        T = np.asarray(T, np.float64)
        c = np.stack([rng.uniform(-1.0, 1.0, 90), rng.uniform(-0.75, 0.75, 90), rng.uniform(1.5, 3.5, 90)], 1)
        pts.append(c @ T[:3, :3].T + T[:3, 3])
    return make_images(11, [E2E_KEYS] * len(poses), poses=[np.asarray(T, np.float64) for T in poses],
                       pts=np.concatenate(pts), share=0.8)[0]
