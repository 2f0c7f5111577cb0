"""NumPy restatement of the bundler's own steps (csrc/bundler.hip), on top of sift_ref, match_ref, match_verify_ref and
fuse_ref which restate the stages it drives: the Gaussian intensity filter (gaussFilterIntensityDevice), the closing
launch (filterFrames + residual order + capacity rule + getSiftTransformCU_Kernel with its three cases) and the submap
bookkeeping (overlap frame, swap, isValid). float32 in the library's operation order, so that results compare bit for bit;
`dt=F64` evaluates the same formulas in float64 for the measured bars."""
import functools

import numpy as np

import match_ref as M
import sift_ref as R

F32, F64 = np.float32, np.float64
NONE = 0xFFFFFFFF
FILT = 25


# ---- k_gauss_intensity ------------------------------------------------------------------------------------------------
def gauss_weights(sigma) -> np.ndarray:
    """[2 r + 1, 2 r + 1] float32, index [dy + r, dx + r]: exp in double of the float32 argument, rounded to float32."""
    s = F32(sigma)
    r = int(np.ceil(2.0 * float(s)))
    d = np.arange(-r, r + 1)
    xx = (d[None, :] ** 2 + d[:, None] ** 2).astype(F32)  # the integer numerator, converted
    arg = -(xx / (F32(2.0) * s * s))
    return np.exp(arg.astype(F64)).astype(F32)


def gauss_intensity(img: np.ndarray, sigma) -> np.ndarray:
    """Window clipped at the borders; sum order m (x) outer, n (y) inner; sum / sumWeight."""
    img = np.asarray(img, F32)
    h, w = img.shape
    wt = gauss_weights(sigma)
    r = wt.shape[0] // 2
    s, sw = np.zeros((h, w), F32), np.zeros((h, w), F32)
    ys, xs = np.mgrid[0:h, 0:w]
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            m, n = xs + dx, ys + dy
            ok = (m >= 0) & (n >= 0) & (m < w) & (n < h)
            wgt = wt[dy + r, dx + r]
            cur = img[np.clip(n, 0, h - 1), np.clip(m, 0, w - 1)]
            sw = np.where(ok, sw + wgt, sw).astype(F32)
            s = np.where(ok, s + wgt * cur, s).astype(F32)
    return (s / sw).astype(F32)


# ---- 4 x 4 arithmetic of the chain ------------------------------------------------------------------------------------
def mat_mul(a, b, dt=F32):
    """s = 0, then += a[r][k] * b[k][c] for k = 0..3, each product and sum rounded to dt."""
    a, b = np.asarray(a, dt).reshape(4, 4), np.asarray(b, dt).reshape(4, 4)
    out = np.zeros((4, 4), dt)
    for k in range(4):
        out = (out + (a[:, k:k + 1] * b[k:k + 1, :]).astype(dt)).astype(dt)
    return out


def rigid_inverse(t, dt=F32):
    """[R^T | -R^T t]: the translation's dot products in float64, rounded to dt once (k_filter's Tinv)."""
    t = np.asarray(t, dt).reshape(4, 4)
    out = np.zeros((4, 4), dt)
    out[:3, :3] = t[:3, :3].T
    for r in range(3):
        a, b = t[:3, r].astype(F64), t[:3, 3].astype(F64)
        out[r, 3] = dt(-((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]))
    out[3, 3] = 1
    return out


# ---- k_frame_close ----------------------------------------------------------------------------------------------------
def close_frame(counts, valid, cur, start, list_end, cap):
    """filterFrames + the exclusive scan + the capacity rule. counts / valid: per image of the store.
    dict(last, valid, bases {prev: offset behind list_end}, added, total, overflow)."""
    n = len(counts)
    last, bases, s = NONE, {}, 0
    for prev in range(start, n):
        if prev == cur:
            continue
        c = min(int(counts[prev]), FILT)
        bases[prev] = s
        s += c
        if c > 0 and valid[prev]:
            last = prev
    overflow = last != NONE and list_end + s > cap
    ok = last != NONE and not overflow
    return dict(last=last if ok else NONE, valid=ok, bases=bases, added=s if ok else 0, total=list_end + (s if ok else 0),
                overflow=overflow, sum=s)


def residuals(keys, filt_idx, counts, cur, start, kinv):
    """AddCurrToResidualsCU's records for a matched frame: pairs in ascending prev, matches in list order.
    keys [n, 4] the store's linear key array, filt_idx {prev: [count, 2]}. (EntryJ array, key index pairs)."""
    from bundlefusion_amd.abi import ENTRYJ_DTYPE
    pos = M.key_points32(keys, kinv)
    rows, kidx = [], []
    for prev in range(start, len(counts)):
        if prev == cur:
            continue
        for t in range(min(int(counts[prev]), FILT)):
            i, j = int(filt_idx[prev][t][0]), int(filt_idx[prev][t][1])
            rows.append((prev, cur, pos[i], pos[j]))
            kidx.append((i, j))
    return np.array(rows, ENTRYJ_DTYPE) if rows else np.zeros(0, ENTRYJ_DTYPE), np.array(kidx, np.uint32).reshape(-1, 2)


def sift_step(sift, f, cur, counts, tinv, frame_valid, complete=None, last_valid=0, dt=F32):
    """getSiftTransformCU_Kernel + computeCurrentSiftTransform for frame f (local frame cur > 0). sift: {frame: 4x4};
    counts / tinv per local image. Returns (sift[f], integrate transform); the three cases on last_valid."""
    if not frame_valid:
        return np.asarray(sift[f - 1], dt).copy(), np.full((4, 4), -np.inf, dt)
    i = cur - 1
    while i >= 0 and counts[i] == 0:
        i -= 1
    assert i >= 0
    known = f - (cur - i)
    s = mat_mul(sift[known], tinv[i], dt)
    if last_valid == 0:
        return s, s.copy()
    if known < last_valid:
        return s, mat_mul(complete[known], tinv[i], dt)
    offset = mat_mul(rigid_inverse(sift[last_valid], dt), sift[known], dt)
    return s, mat_mul(mat_mul(complete[last_valid], offset, dt), tinv[i], dt)


# ---- submap bookkeeping (OnlineBundler::processInput, prepareLocalSolve, Bundler::copyFrame / isValid) --------------------
class Book:
    """Which local image a frame becomes, when a submap closes, what the other set starts with."""

    def __init__(self, submap_size: int):
        self.S = submap_size
        self.images = []   # frame indices of the current local set
        self.valid = []
        self.frame = 0
        self.closed = None  # dict(frames, valid, is_valid, submap)

    def add(self):
        """-> (frame, local frame, submap, closes)."""
        f = self.frame
        self.images.append(f)
        self.valid.append(1 if len(self.images) == 1 else 0)
        self.frame += 1
        return f, len(self.images) - 1, 0 if f == 0 else (f - 1) // self.S, f > 0 and f % self.S == 0

    def decide(self, valid: bool):
        self.valid[-1] = int(valid)

    def close(self):
        self.closed = dict(frames=list(self.images), valid=list(self.valid), is_valid=any(self.valid[1:]),
                           submap=(self.images[-1] - 1) // self.S)
        self.images, self.valid = [self.images[-1]], [1]  # the overlap frame: the other set's image 0, valid


# ---- the chain over a sift_ref scene, all in the restatement -----------------------------------------------------------
@functools.lru_cache(None)
def views(name: str, n: int, seed_override=None):
    """[(RGBX colour, depth, camera -> world)] of scene `name` at pose(0..n-1)."""
    f = R.FIXTURES[name]
    sc = R.scene(name) if seed_override is None else R.Scene(seed_override, f["blobs"], f["sigma_px"], f["w"])
    return [sc.render_color(R.pose(k), f["w"], f["h"], f["dw"], f["dh"]) + (R.pose(k),) for k in range(n)]


@functools.lru_cache(None)
def detected(name: str, n: int):
    f = R.FIXTURES[name]
    c = R.cfg(f["w"], f["h"], f["dw"], f["dh"])
    out = []
    for color, depth, _ in views(name, n):
        d = R.detect(R.intensity(color, f["w"], f["h"]), depth, c)
        out.append((d["keys"], d["descs"]))
    return out


def pose_error(rel, prev: int, cur: int):
    """(translation m, rotation rad) of rel = camera cur in camera prev against the ground truth."""
    gt = np.linalg.inv(R.pose(prev)) @ R.pose(cur)
    return float(np.linalg.norm(np.asarray(rel, F64)[:3, 3] - gt[:3, 3])), M.rot_diff(rel, gt)


@functools.lru_cache(None)
def chain_reference(name: str, n: int, submap_size: int) -> dict:
    """The restatement's own chain: detect -> match_ref.run per frame inside its submap (Kabsch filter only) -> the
    closing step -> sift poses. dict(sift, counts [per frame {prev local: count}], valid, t_err, r_err of consecutive
    sift poses, submaps [closed dicts with entries])."""
    f = R.FIXTURES[name]
    kinv = R.intrinsics_inv(f["w"], f["h"])
    images = detected(name, n)
    book = Book(submap_size)
    sift = {0: np.eye(4, dtype=F32)}
    counts_log, valid_log, t_err, r_err, submaps, entries = [{}], [True], [], [], [], []
    for k in range(n):
        fr, lf, sm, closes = book.add()
        if lf > 0:
            store = [images[i] for i in book.images]
            out = M.run(store, lf, 0, book.valid, kinv)
            counts = [out["pairs"][p]["filt"]["count"] if p != lf else 0 for p in range(lf + 1)]
            tinv = [rigid_inverse(out["pairs"][p]["filt"]["T"]) if p != lf else None for p in range(lf + 1)]
            c = close_frame(counts, book.valid, lf, 0, len(entries), 1 << 28)
            book.decide(c["valid"])
            if c["valid"]:
                entries += out["entries"]
            sift[fr], _ = sift_step(sift, fr, lf, counts, tinv, c["valid"])
            counts_log.append({p: counts[p] for p in range(lf)})
            valid_log.append(c["valid"])
            te, re = pose_error(np.linalg.inv(sift[fr - 1].astype(F64)) @ sift[fr].astype(F64), fr - 1, fr)
            t_err.append(te)
            r_err.append(re)
        if closes:
            book.close()
            submaps.append(dict(book.closed, entries=entries))
            entries = []
    return dict(sift=sift, counts=counts_log, valid=valid_log, t_err=t_err, r_err=r_err, submaps=submaps)


def case_spread(seed=0, frames=8) -> float:
    """The largest |float32 - float64| element of the third case's integrate transform over random rigid chains of the
    fixture's size (steps of a few cm and mrad around a pose at 2 m): the float32-against-float64 spread."""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(200):
        def rigid(scale_t, scale_r):
            w = rng.normal(size=3) * scale_r
            th = np.linalg.norm(w)
            Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            Rm = np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = Rm, rng.normal(size=3) * scale_t
            return T
        sift = {0: np.eye(4, dtype=F32)}
        for k in range(1, frames):
            sift[k] = mat_mul(sift[k - 1], rigid(0.05, 0.01).astype(F32))
        complete = {k: mat_mul(rigid(2.0, 0.5).astype(F32), sift[k]) for k in range(frames)}
        tinv = [rigid(0.05, 0.01).astype(F32) for _ in range(4)]
        counts = [25, 0, 25, 0]
        lv, f, cur = 2, frames - 1, 3
        a = sift_step(sift, f, cur, counts, tinv, True, complete, lv, F32)[1]
        b = sift_step({k: v.astype(F64) for k, v in sift.items()}, f, cur, counts, [t.astype(F64) for t in tinv], True,
                      {k: v.astype(F64) for k, v in complete.items()}, lv, F64)[1]
        worst = max(worst, float(np.abs(a.astype(F64) - b).max()))
    return worst


@functools.lru_cache(None)
def global_reference(name: str, n: int, submap_size: int) -> dict:
    """The same chain carried on through fuse_ref: every closed submap of chain_reference is fused with the local
    transforms of the restatement's own sift chain (frame -> the submap's first frame; the restatement has no solver),
    and the fused images are matched with match_ref. dict(rel {(prev, cur): camera cur in camera prev}, t_err, r_err of
    key frame 1 in key frame 0 against the ground truth of frames 0 and submap_size)."""
    import fuse_ref as F
    f = R.FIXTURES[name]
    kinv = R.intrinsics_inv(f["w"], f["h"])
    Kc = np.linalg.inv(kinv.astype(F64)).astype(F32)
    images, ch = detected(name, n), chain_reference(name, n, submap_size)
    glob = []
    for sm in ch["submaps"]:
        store = [images[i] for i in sm["frames"]]
        keys = np.concatenate([np.asarray(k, F32).reshape(-1, 4) for k, _ in store])
        descs = np.concatenate([d for _, d in store])
        pos = M.key_points32(keys, kinv)
        corr = np.array([(p, c, pos[a], pos[b]) for p, c, a, b in sm["entries"]], _entryj())
        kidx = np.array([(a, b) for _, _, a, b in sm["entries"]], np.uint32).reshape(-1, 2)
        first = rigid_inverse(ch["sift"][sm["frames"][0]])
        tr = [mat_mul(first, ch["sift"][i]) for i in sm["frames"]]
        out = F.fuse(keys, descs, corr, kidx, tr, Kc, 1024)
        glob.append((out["keys"], out["descs"]))
    run = M.run(glob[:2], 1, 0, [1, 1], kinv)
    filt = run["pairs"][0]["filt"]
    rel = np.linalg.inv(np.asarray(filt["T"], F64))
    te, re = pose_error(rel, 0, submap_size)
    return dict(rel=rel, count=int(filt["count"]), t_err=te, r_err=re, images=glob)


def _entryj():
    from bundlefusion_amd.abi import ENTRYJ_DTYPE
    return ENTRYJ_DTYPE
