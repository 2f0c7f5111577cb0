"""NumPy restatement of the SIFT detector (bf_sift_*): SiftGPU as BundleFusion configures it, stage by
stage: filter tables, the float32 tap-ordered pyramid, the exact key test, caps and limits, orientation, reshape,
descriptor. The exact stages are float32 with the operations in the library's order; the transcendental stages
(orientation, descriptor) run in float64 or float32 (`dtype`), so the restatement's own precision spread can be
measured. Borderline items - decisions a last-bit difference could flip - are marked, as match_ref.py does for its
ratio tests. Also the fixtures: an analytic textured scene, a camera and poses."""
from __future__ import annotations

import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
LEVELS, OCTAVES, GAUSS = 12, 4, 6
PI = 3.14159265358979323846


def cfg(width, height, depth_width=None, depth_height=None, max_keys=1024, feature_count_threshold=150,
        depth_min=0.1, depth_max=4.0, min_key_scale=3.0, dog_threshold=None, edge_threshold=10.0) -> dict:
    return dict(w=width, h=height, dw=depth_width or width, dh=depth_height or height, max_keys=max_keys,
                thr_count=feature_count_threshold, dmin=F32(depth_min), dmax=F32(depth_max), min_scale=F32(min_key_scale),
                dog=F32(0.02) / F32(3.0) if dog_threshold is None else F32(dog_threshold), edge=F32(edge_threshold))


# ---- filter tables (SiftParam::ParseSiftParam, ProgramCU::CreateFilterKernel) ----------------------------------
def _pow(b, e) -> np.float32:
    """pow in double, rounded to float (the library does the same, so no float pow routine is involved)."""
    return F32(math.pow(float(F32(b)), float(F32(e))))


@functools.lru_cache(None)
def tables() -> dict:
    third = F32(1.0) / F32(3.0)
    sigmak = _pow(2.0, third)
    sigma0 = F32(1.6) * _pow(2.0, third)
    dsigma0 = sigma0 * np.sqrt(F32(1.0) - F32(1.0) / (sigmak * sigmak))
    sa, sb = sigma0 * _pow(2.0, F32(-1.0) / F32(3.0)), F32(0.5) / _pow(2.0, 0.0)
    sigmas = [np.sqrt(sa * sa - sb * sb) if float(sa) > float(sb) + 0.001 else F32(0)]
    sigmas += [dsigma0 * _pow(sigmak, F32(i)) for i in range(5)]
    level_sigma = [sigma0 * _pow(2.0, F32(j) / F32(3.0)) for j in range(3)]
    ks = []
    for sigma in sigmas:
        sigma = F32(sigma)
        sz = int(math.ceil(float(F32(4.0) * sigma) - 0.5))
        width = 2 * sz + 1
        if width > 33:
            sz, width = 16, 33
        elif width < 5:
            sz, width = 2, 5
        rv = F32(1.0) / (sigma * sigma)
        k = np.zeros(width, F32)
        ksum = F32(0)
        for i in range(-sz, sz + 1):
            v = F32(math.exp(float(F32(-0.5) * F32(i) * F32(i) * rv)))
            k[i + sz] = v
            ksum = F32(ksum + v)
        k *= F32(1.0) / ksum
        ks.append(k)
    return dict(k=ks, widths=[len(k) for k in ks], sigmas=[F32(s) for s in sigmas], level_sigma=[F32(s) for s in level_sigma])


# ---- intensity (resampleToIntensity + convertToIntensity) ------------------------------------------------------
def intensity(color: np.ndarray, w: int, h: int) -> np.ndarray:
    """color [ch, cw, 4] uint8 -> float32 [h, w]."""
    ch, cw = color.shape[:2]
    sx, sy = F32(cw - 1) / F32(w - 1), F32(ch - 1) / F32(h - 1)
    xi = (np.arange(w, dtype=F32) * sx + F32(0.5)).astype(np.uint32)
    yi = (np.arange(h, dtype=F32) * sy + F32(0.5)).astype(np.uint32)
    c = color[np.minimum(yi, ch - 1)][:, np.minimum(xi, cw - 1)].astype(F32)
    out = (F32(0.299) * c[..., 0] + F32(0.587) * c[..., 1] + F32(0.114) * c[..., 2]) / F32(255.0)
    ok = (yi < ch)[:, None] & (xi < cw)[None, :]
    return np.where(ok, out, F32(0)).astype(F32)


# ---- pyramid (SiftPyramid::BuildPyramid, FilterH / FilterV, DownsampleKernel) -----------------------------------
def _filter(img: np.ndarray, k: np.ndarray) -> np.ndarray:
    """Separable, horizontal then vertical, clamp-to-edge; value = 0, value += data[i] * k[i] for ascending i."""
    hw = len(k) // 2
    h, w = img.shape
    p = img[:, np.clip(np.arange(-hw, w + hw), 0, w - 1)]
    out = np.zeros((h, w), F32)
    for i, c in enumerate(k):
        out += p[:, i:i + w] * F32(c)
    p = out[np.clip(np.arange(-hw, h + hw), 0, h - 1), :]
    out = np.zeros((h, w), F32)
    for i, c in enumerate(k):
        out += p[i:i + h, :] * F32(c)
    return out


def pyramid(img: np.ndarray, ks=None) -> list:
    """g[octave][level], float32; ks: the six coefficient arrays (default: this module's tables)."""
    ks = tables()["k"] if ks is None else ks
    img = np.ascontiguousarray(img, F32)
    g = []
    for o in range(OCTAVES):
        if o == 0:
            lv = [_filter(img, ks[0])]
        else:
            src = g[o - 1][3]
            sh, sw = src.shape
            h, w = sh >> 1, sw >> 1
            lv = [src[(np.arange(h) << 1)][:, np.minimum(np.arange(w) << 1, sw - 1)].copy()]
        for l in range(1, GAUSS):
            lv.append(_filter(lv[l - 1], ks[l]))
        g.append(lv)
    return g


# ---- key test (ComputeKEY_Kernel) ---------------------------------------------------------------------------------
def _round_half_away(x):
    return np.floor(np.asarray(x, F64) + 0.5).astype(np.int64)  # arguments are >= 0 here


def depth_pixel(c: dict, o: int, col, row):
    kls = F32(1 << o)
    dx = _round_half_away((kls * np.asarray(col, F32) + F32(0.5)) * F32(c["dw"] - 1) / F32(c["w"] - 1))
    dy = _round_half_away((kls * np.asarray(row, F32) + F32(0.5)) * F32(c["dh"] - 1) / F32(c["h"] - 1))
    return dx, dy


def raw_keys_level(g4, o: int, depth: np.ndarray, c: dict) -> np.ndarray:
    """g4: Gaussian levels jj ... jj + 3 of the octave. Returns int [n, 2] (col, row) in (row, col) ascending order."""
    h, w = g4[0].shape
    if h < 4 or w < 4:
        return np.zeros((0, 2), np.int64)
    P, C_, N = g4[1] - g4[0], g4[2] - g4[1], g4[3] - g4[2]
    rows, cols = np.arange(1, h - 2), np.arange(1, w - 2)
    R, Cc = np.meshgrid(rows, cols, indexing="ij")
    dx, dy = depth_pixel(c, o, Cc, R)
    ok = (dx >= 0) & (dx < c["dw"]) & (dy >= 0) & (dy < c["dh"])
    d = depth[np.clip(dy, 0, c["dh"] - 1), np.clip(dx, 0, c["dw"] - 1)]
    with np.errstate(invalid="ignore"):
        ok &= (d >= c["dmin"]) & (d <= c["dmax"])

    def at(D, dr, dc):
        return D[1 + dr:h - 2 + dr, 1 + dc:w - 2 + dc]

    v = at(C_, 0, 0)
    ok &= np.abs(v) > c["dog"]
    d10, d12 = at(C_, 0, -1), at(C_, 0, 1)
    nmax, nmin = np.maximum(d10, d12), np.minimum(d10, d12)
    ok &= ~((v <= nmax) & (v >= nmin))

    def cmp3(D, dr):
        nonlocal nmax, nmin, ok
        a, b, e = at(D, dr, -1), at(D, dr, 0), at(D, dr, 1)
        m = v > nmax
        nmax = np.where(m, np.maximum(np.maximum(np.maximum(nmax, a), b), e), nmax)
        nmin = np.where(~m, np.minimum(np.minimum(np.minimum(nmin, a), b), e), nmin)
        ok &= ~(m & (v < nmax)) & ~(~m & (v > nmin))

    cmp3(C_, -1)
    cmp3(C_, 1)
    vx2 = v * F32(2.0)
    fxx = d10 + d12 - vx2
    fyy = at(C_, -1, 0) + at(C_, 1, 0) - vx2
    fxy = F32(0.25) * (at(C_, 1, 1) + at(C_, -1, -1) - at(C_, 1, -1) - at(C_, -1, 1))
    t1 = fxx * fyy - fxy * fxy
    t2 = (fxx + fyy) * (fxx + fyy)
    edge = (c["edge"] + F32(1)) * (c["edge"] + F32(1)) / c["edge"]
    ok &= ~((t1 <= 0) | (t2 > edge * t1))
    for D in (P, N):
        for dr in (-1, 0, 1):
            cmp3(D, dr)
    r, cc = np.nonzero(ok)  # row-major: (row, col) ascending
    return np.stack([cc + 1, r + 1], axis=1).astype(np.int64)


def raw_keys(g, depth, c) -> list:
    return [raw_keys_level(g[L // 3][L % 3:L % 3 + 4], L // 3, depth, c) for L in range(LEVELS)]


# ---- caps and limits -----------------------------------------------------------------------------------------------
def fmax(w: int, h: int) -> int:
    return int(min(max(int(F32(w * h) * F32(0.005)), 32), 4096))


def fmaxs(c: dict) -> list:
    return [fmax(c["w"] >> (L // 3), c["h"] >> (L // 3)) for L in range(LEVELS)]


def limit(counts, thr: int) -> list:
    """LimitFeatureCount, truncate method 0, with the while loop stopped at the last level."""
    num = [int(x) for x in counts]
    total, i = sum(num), 0
    while i < len(num) and total - num[i] > thr:
        total -= num[i]
        num[i] = 0
        i += 1
    return num


def cap_and_limit(raw_counts, fm, thr: int) -> list:
    return limit([min(int(n), int(f)) for n, f in zip(raw_counts, fm)], thr)


def hard_cap(counts, max_keys: int):
    """Coarsest levels whole, the crossing level its first keys. Returns (kept per level, truncated)."""
    keep, cur = [0] * len(counts), 0
    for L in range(len(counts) - 1, -1, -1):
        keep[L] = min(int(counts[L]), max_keys - cur)
        cur += keep[L]
    return keep, sum(int(x) for x in counts) > max_keys


# ---- gradient --------------------------------------------------------------------------------------------------------
def _grad(g: np.ndarray, px, py, dtype):
    dx = (g[py, px + 1] - g[py, px - 1]).astype(dtype)  # float32 differences, as the library takes them
    dy = (g[py + 1, px] - g[py - 1, px]).astype(dtype)
    grd = dtype(0.5) * np.sqrt(dx * dx + dy * dy)
    rot = np.where(grd == 0, dtype(0), np.arctan2(dy, dx)).astype(dtype)
    return grd, rot


def _window(kx, ky, half, w, h, dtype):
    xmin, ymin = max(1.5, math.floor(kx - half) + 0.5), max(1.5, math.floor(ky - half) + 0.5)
    xmax, ymax = min(w - 1.5, math.floor(kx + half) + 0.5), min(h - 1.5, math.floor(ky + half) + 0.5)
    if xmax < xmin or ymax < ymin:
        return np.zeros(0, dtype), np.zeros(0, dtype)
    xs = np.arange(int(round(xmax - xmin + 1))) + xmin
    ys = np.arange(int(round(ymax - ymin + 1))) + ymin
    X, Y = np.meshgrid(xs, ys)
    return X.ravel().astype(dtype), Y.ravel().astype(dtype)


# ---- orientation (ComputeOrientation_Kernel) -----------------------------------------------------------------------
BIN_MARGIN = 2e-5      # bin units: about 14 ulp of an angle near pi times 5.73
VOTE_MARGIN = 1e-4     # relative, on smoothed votes: a float32 sum of a few hundred terms is good to ~2e-5
WEIGHT_FLOOR = 1e-4    # of the largest vote: an uncertain sample lighter than this cannot move a decision
STEP_MARGIN = 1e-3     # of one 16-bit step, at least; see step_margin
VOTE_EPS = 3e-7        # relative float32 error of one smoothed vote: a weight is a sqrt, an exp (1-2 ulp on the device)
#                        and two products, about 4 ulp, and the rounding errors of the short sums do not add coherently


def step_margin(c, m, p) -> float:
    """How far (in 16-bit steps) a float32 evaluation can move a packed orientation: with di = 0.5 (p - m) / D,
    D = 2 c - p - m, vote errors of VOTE_EPS c move p - m by 2 and D by 4 of them, so di by at most
    0.5 (2 + 4 |p - m| / D) VOTE_EPS c / D <= 3 VOTE_EPS c / D bins of 65535 / 36 steps each."""
    d = float(2.0 * c - p - m)
    return max(STEP_MARGIN, (65535.0 / 36.0) * 3.0 * VOTE_EPS * float(c) / d) if d > 0 else 1.0


def orientation(g: np.ndarray, col: int, row: int, sigma, dtype=F64) -> dict:
    """g: the Gaussian level the gradient comes from. Returns dict(us1, us2, packed, border)."""
    h, w = g.shape
    sigma = dtype(sigma)
    kx, ky = dtype(col + 0.5), dtype(row + 0.5)
    gsigma = sigma * dtype(1.5)
    win = abs(sigma) * dtype(1.5) * dtype(2.0)
    thr2 = dtype(F64(win * win) + 0.5)
    factor = dtype(-0.5) / (gsigma * gsigma)
    X, Y = _window(float(kx), float(ky), float(win), w, h, dtype)
    dx, dy = X - kx, Y - ky
    sq = dx * dx + dy * dy
    border = bool(np.any(np.abs(sq - thr2) <= 1e-6 * float(thr2)))
    inside = sq < thr2
    X, Y, sq = X[inside], Y[inside], sq[inside]
    grd, rot = _grad(g, X.astype(np.int64), Y.astype(np.int64), dtype)
    weight = grd * np.exp(sq * factor)
    t = rot * dtype(5.7295779513082320876798154814105)
    idx = np.floor(t).astype(np.int64)
    idx[idx < 0] += 36
    vote = np.zeros(36, dtype)
    np.add.at(vote, idx, weight)
    near_edge = np.abs(t - np.round(t)) <= BIN_MARGIN
    one_third = dtype(1.0 / 3.0)
    for _ in range(6):
        vote = ((np.roll(vote, 1) + vote + np.roll(vote, -1)) * one_third).astype(dtype)
    vmax = max(float(vote.max()), 0.0) if len(vote) else 0.0
    if vmax > 0 and np.any(weight[near_edge] > WEIGHT_FLOOR * vmax):
        border = True
    thr = dtype(vmax) * dtype(0.8)
    m, p = np.roll(vote, 1), np.roll(vote, -1)
    is_peak = (vote > thr) & (vote > m) & (vote > p)

    def near(a, b):
        return np.abs(a - b) <= VOTE_MARGIN * np.maximum(np.abs(a), np.abs(b))

    n_thr, n_m, n_p = near(vote, thr), near(vote, m), near(vote, p)
    maybe = ((vote > thr) | n_thr) & ((vote > m) | n_m) & ((vote > p) | n_p)
    if vmax > 0 and np.any(maybe & (n_thr | n_m | n_p)):
        border = True
    peaks = sorted(np.nonzero(is_peak)[0], key=lambda b: (-float(vote[b]), b))
    for a, b in zip(peaks[:2], peaks[1:3]):  # order of the first two, second against third
        if near(vote[a], vote[b]):
            border = True
    us = [65535, 65535]
    for k, b in enumerate(peaks[:2]):
        c_, m_, p_ = vote[b], vote[(b + 35) % 36], vote[(b + 1) % 36]
        rot_ = dtype(b) + dtype(0.5) * ((p_ - m_) / (dtype(2.0) * c_ - p_ - m_)) + dtype(0.5)
        fr = rot_ / dtype(36.0)
        if fr < 0:
            fr += dtype(1.0)
        s = float(fr * dtype(65535.0))
        if abs(s - round(s)) <= step_margin(c_, m_, p_):
            border = True
        us[k] = int(math.floor(s)) & 0xFFFF
    return dict(us1=us[0], us2=us[1], packed=(us[1] << 16) | us[0], border=border)


# ---- reshape (ReshapeFeatureList, LimitFeatureCount(1), CreateGlobalKeyPointList) --------------------------------
def reshape(lists, packed, c: dict, depth: np.ndarray):
    """lists[L]: int [n, 2] (col, row) after cap and LimitFeatureCount(0); packed[L]: uint32 [n]. Returns dict(keys
    float32 [n, 4] (x, y, scale, depth), entries [(L, raw index, which orientation, orientation float32)], kept [12],
    truncated)."""
    fm, ls = fmaxs(c), tables()["level_sigma"]
    factor = F32(2.0 * PI / 65535.0)
    per_level = []
    for L in range(LEVELS):
        ent = []
        if ls[L % 3] * F32(1 << (L // 3)) >= c["min_scale"]:
            for i, pk in enumerate(np.asarray(packed[L], np.uint32)):
                us1, us2 = int(pk) & 0xFFFF, int(pk) >> 16
                if us1 == 65535:
                    continue
                ent.append((L, i, 0, factor * F32(us1)))
                if us2 != 65535 and us2 != us1:
                    ent.append((L, i, 1, factor * F32(us2)))
        per_level.append(ent[:fm[L]])
    counts = limit([len(e) for e in per_level], c["thr_count"])
    kept, truncated = hard_cap(counts, c["max_keys"])
    entries = [e for L in range(LEVELS) for e in per_level[L][:kept[L]]]
    keys = np.zeros((len(entries), 4), F32)
    for n, (L, i, _, _) in enumerate(entries):
        o, kls = L // 3, F32(1 << (L // 3))
        col, row = lists[L][i]
        x, y = kls * F32(col) + F32(0.5), kls * F32(row) + F32(0.5)
        dx, dy = depth_pixel(c, o, col, row)
        keys[n] = (x, y, kls * ls[L % 3], depth[dy, dx])
    return dict(keys=keys, entries=entries, kept=kept, truncated=truncated)


# ---- descriptor (ComputeDescriptor_Kernel, NormalizeDescriptor_Kernel, ConvertDescriptorToUChar_Kernel) ---------
# of one byte step. A bin is a sum of up to ~200 samples, each good to about 5 float32 ulp (expf, atan2f, the products),
# and the 1-2 ulp of sincosf enter every sample's coordinates coherently: about 1e-5 relative of values 512 v <= 103,
# that is 1e-3; the margin is twice that.
BYTE_MARGIN = 2e-3


def descriptor(g: np.ndarray, col: int, row: int, sigma, ori, dtype=F64) -> dict:
    """Returns dict(bytes uint8 [128], value float64 [128] = 512 v + 0.5, border bool [128], reach256)."""
    h, w = g.shape
    kx, ky, sigma, ori = dtype(col + 0.5), dtype(row + 0.5), dtype(sigma), dtype(F32(ori))
    rpi = dtype(4.0 / PI)
    spt = abs(sigma * dtype(3.0))
    s, c_ = np.sin(ori), np.cos(ori)
    anglef = dtype(float(ori) - 2.0 * PI) if float(ori) > PI else ori
    cspt, sspt, crspt, srspt = c_ * spt, s * spt, c_ / spt, s / spt
    des = np.zeros(128, dtype)
    bsz = float(abs(cspt) + abs(sspt))
    for cell in range(16):
        ox, oy = dtype((cell & 3) - 1.5), dtype((cell >> 2) - 1.5)
        ptx = cspt * ox - sspt * oy + kx
        pty = cspt * oy + sspt * ox + ky
        xmin, ymin = max(1.5, math.floor(float(ptx) - bsz) + 0.5), max(1.5, math.floor(float(pty) - bsz) + 0.5)
        xmax, ymax = min(w - 1.5, math.floor(float(ptx) + bsz) + 0.5), min(h - 1.5, math.floor(float(pty) + bsz) + 0.5)
        if xmax < xmin or ymax < ymin:
            continue
        X, Y = np.meshgrid(np.arange(int(round(xmax - xmin + 1))) + xmin, np.arange(int(round(ymax - ymin + 1))) + ymin)
        X, Y = X.ravel().astype(dtype), Y.ravel().astype(dtype)
        dx, dy = X - ptx, Y - pty
        nx, ny = crspt * dx + srspt * dy, crspt * dy - srspt * dx
        nxn, nyn = np.abs(nx), np.abs(ny)
        ins = (nxn < 1) & (nyn < 1)
        X, Y, nx, ny, nxn, nyn = X[ins], Y[ins], nx[ins], ny[ins], nxn[ins], nyn[ins]
        grd, rot = _grad(g, X.astype(np.int64), Y.astype(np.int64), dtype)
        dnx, dny = nx + ox, ny + oy
        ww = np.exp(dtype(-0.125) * (dnx * dnx + dny * dny))
        weight = ww * (dtype(1.0) - nxn) * (dtype(1.0) - nyn) * grd
        theta = (anglef - rot) * rpi
        theta = np.where(theta < 0, theta + dtype(8.0), theta).astype(dtype)
        fo = np.floor(theta)
        f0 = fo.astype(np.int64) & 7
        np.add.at(des, cell * 8 + f0, (fo + dtype(1.0) - theta) * weight)
        np.add.at(des, cell * 8 + ((f0 + 1) & 7), (theta - fo) * weight)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.minimum(dtype(0.2), des * (dtype(1.0) / np.sqrt(np.sum(des * des, dtype=dtype))))
        v = v * (dtype(1.0) / np.sqrt(np.sum(v * v, dtype=dtype)))
    value = (dtype(512.0) * v).astype(F64) + 0.5
    value = np.nan_to_num(value, nan=0.0)
    ints = value.astype(np.int64)
    return dict(bytes=(ints & 0xFF).astype(np.uint8), value=value, border=np.abs(value - np.round(value)) <= BYTE_MARGIN,
                reach256=bool(np.any(ints >= 256)))


# ---- the whole detector ------------------------------------------------------------------------------------------------
def detect(img, depth, c: dict, dtype=F64, ks=None, descriptors=True, g=None) -> dict:
    """dict(g, raw [12 lists], raw_counts, lists (after cap + limit), ori [12 lists of dicts], packed, keys, entries,
    kept, truncated, descs uint8 [n, 128], key_border [n], byte_border [n, 128], reach256)."""
    depth = np.ascontiguousarray(depth, F32)
    g = pyramid(img, ks) if g is None else g
    raw = raw_keys(g, depth, c)
    raw_counts = [len(r) for r in raw]
    list_counts = cap_and_limit(raw_counts, fmaxs(c), c["thr_count"])
    lists = [raw[L][:list_counts[L]] for L in range(LEVELS)]
    ls = tables()["level_sigma"]
    ori, packed = [], []
    for L in range(LEVELS):
        o, jj = L // 3, L % 3
        if ls[jj] * F32(1 << o) >= c["min_scale"]:
            res = [orientation(g[o][jj + 1], int(cc), int(rr), ls[jj], dtype) for cc, rr in lists[L]]
        else:
            res = [dict(us1=65535, us2=65535, packed=0xFFFFFFFF, border=False) for _ in lists[L]]
        ori.append(res)
        packed.append(np.array([r["packed"] for r in res], np.uint32))
    out = reshape(lists, packed, c, depth)
    out.update(g=g, raw=raw, raw_counts=raw_counts, lists=lists, ori=ori, packed=packed)
    n = len(out["entries"])
    out["key_border"] = np.array([ori[L][i]["border"] for L, i, _, _ in out["entries"]], bool).reshape(n)
    if descriptors:
        ds = [descriptor(g[L // 3][L % 3 + 1], int(lists[L][i][0]), int(lists[L][i][1]), ls[L % 3], a, dtype)
              for L, i, _, a in out["entries"]]
        out["descs"] = np.array([d["bytes"] for d in ds], np.uint8).reshape(n, 128)
        out["byte_border"] = np.array([d["border"] for d in ds], bool).reshape(n, 128)
        out["reach256"] = any(d["reach256"] for d in ds)
    return out


# ---- fixtures: an analytic textured scene -------------------------------------------------------------------------
def camera(w: int, h: int):
    """fx, fy, cx, cy of a w x h image: a 0.9 w focal length, as a 580-pixel lens on 640 x 480."""
    return 0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0


def intrinsics_inv(w: int, h: int) -> np.ndarray:
    fx, fy, cx, cy = camera(w, h)
    K = np.eye(4)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return np.linalg.inv(K).astype(F32)


def pose(k: int, step=0.03, rot=0.004) -> np.ndarray:
    """Camera -> world of view k: a few cm and a few mrad per view."""
    a = rot * k
    T = np.eye(4)
    T[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    T[:3, 3] = [step * k, 0.01 * k, -0.01 * k]
    return T


def surface(x, y):
    """World z of the surface: 0.7 m of relief around z = 2 m."""
    return 2.0 + 0.2 * np.sin(1.3 * x) + 0.15 * np.cos(1.7 * y + 0.5)


class Scene:
    """A world-space texture (a sum of Gaussian blobs over (x, y)) on `surface`, sampled per pixel by ray casting: no
    image interpolation anywhere. `sigma_px`: the blobs' sigma range in pixels of a `ref_width`-wide image at 2 m."""

    def __init__(self, seed: int, blobs: int = 500, sigma_px=(2.5, 14.0), ref_width=160, extent=1.5, lattice_px=None):
        r = np.random.default_rng(seed)
        m_per_px = 2.0 / camera(ref_width, 1)[0]
        if lattice_px is None:
            self.p = r.uniform(-extent, extent, size=(blobs, 2))
        else:  # a jittered lattice instead: isolated blobs, as many keys of one scale as the image can hold
            t = np.arange(-extent, extent, lattice_px * m_per_px)
            X, Y = np.meshgrid(t, t)
            self.p = np.stack([X.ravel(), Y.ravel()], axis=1)
            self.p += r.uniform(-0.1, 0.1, size=self.p.shape) * lattice_px * m_per_px
            blobs = len(self.p)
        self.s = np.exp(r.uniform(np.log(sigma_px[0]), np.log(sigma_px[1]), size=blobs)) * m_per_px
        self.a = r.uniform(0.15, 0.45, size=blobs) * r.choice([-1.0, 1.0], size=blobs)

    def hit(self, T, w, h, at=None):
        """World hit points and camera z of the rays through the pixels of a w x h image whose pixel grid spans the
        image `at` = (iw, ih) (default itself): pixel u maps to u (iw - 1) / (w - 1) there."""
        iw, ih = at or (w, h)
        fx, fy, cx, cy = camera(iw, ih)
        u = np.arange(w) * ((iw - 1) / (w - 1))
        v = np.arange(h) * ((ih - 1) / (h - 1))
        U, V = np.meshgrid(u, v)
        d = np.stack([(U.ravel() - cx) / fx, (V.ravel() - cy) / fy, np.ones(w * h)], axis=1)
        dw = d @ T[:3, :3].T
        c = T[:3, 3]
        t = np.full(w * h, 2.0)
        for _ in range(40):  # fixed point of c_z + t d_z = surface(x(t), y(t)); the surface's slope is below 0.3
            t = (surface(c[0] + t * dw[:, 0], c[1] + t * dw[:, 1]) - c[2]) / dw[:, 2]
        return c + t[:, None] * dw, t  # d has unit z: t is the camera-space depth

    def texture(self, T, w, h) -> np.ndarray:
        """0.5 + the blobs at every pixel's own world hit point, clipped to [0, 1]. A blob is added inside the pixel
        window that holds its 5 sigma disc (beyond it: below 2e-6)."""
        p, _ = self.hit(T, w, h)
        px, py = p[:, 0].reshape(h, w), p[:, 1].reshape(h, w)
        fx, fy, cx, cy = camera(w, h)
        q = np.stack([self.p[:, 0], self.p[:, 1], surface(self.p[:, 0], self.p[:, 1])], axis=1)
        qc = (q - T[:3, 3]) @ T[:3, :3]
        uc, vc = fx * qc[:, 0] / qc[:, 2] + cx, fy * qc[:, 1] / qc[:, 2] + cy
        out = np.full((h, w), 0.5)
        for i in range(len(self.s)):
            r = int(5.0 * self.s[i] * fx / 1.5) + 2
            x0, x1 = max(int(uc[i]) - r, 0), min(int(uc[i]) + r + 1, w)
            y0, y1 = max(int(vc[i]) - r, 0), min(int(vc[i]) + r + 1, h)
            if x0 >= x1 or y0 >= y1:
                continue
            d2 = (px[y0:y1, x0:x1] - self.p[i, 0]) ** 2 + (py[y0:y1, x0:x1] - self.p[i, 1]) ** 2
            out[y0:y1, x0:x1] += self.a[i] * np.exp(-d2 / (2.0 * self.s[i] ** 2))
        return np.clip(out, 0.0, 1.0)

    def render(self, T, w, h, dw=None, dh=None):
        """(intensity float32 [h, w] in [0, 1], depth float32 [dh, dw] in metres)."""
        img = self.texture(T, w, h).astype(F32)
        dw, dh = dw or w, dh or h
        _, z = self.hit(T, dw, dh, at=(w, h))
        return img, z.reshape(dh, dw).astype(F32)

    def render_color(self, T, w, h, dw=None, dh=None):
        """(RGBX uint8 [h, w, 4] grey, depth)."""
        img, z = self.render(T, w, h, dw, dh)
        b = np.round(img * 255.0).astype(np.uint8)
        return np.stack([b, b, b, np.full_like(b, 255)], axis=2), z


def blob_image(w: int, h: int, cx: float, cy: float, sigma: float, amp=0.5) -> np.ndarray:
    """One isotropic Gaussian blob on a flat background."""
    X, Y = np.meshgrid(np.arange(w) + 0.0, np.arange(h) + 0.0)
    return (0.25 + amp * np.exp(-((X - cx) ** 2 + (Y - cy) ** 2) / (2.0 * sigma * sigma))).astype(F32)


# fixture table: scene seed, blob count, blob sigma range (pixels of this image), image and depth size, options
FIXTURES = {
    "small": dict(seed=3, blobs=600, sigma_px=(2.5, 14.0), w=160, h=120, dw=80, dh=60, opts={}),
    "odd": dict(seed=4, blobs=600, sigma_px=(2.5, 14.0), w=172, h=130, dw=172, dh=130, opts={}),
    "medium": dict(seed=18, blobs=600, sigma_px=(2.5, 14.0), w=320, h=240, dw=320, dh=240, opts={}),
    "dense": dict(seed=17, blobs=0, sigma_px=(4.0, 4.6), lattice_px=14, w=160, h=120, dw=160, dh=120, opts={}),
    "hardcap": dict(seed=18, blobs=600, sigma_px=(2.5, 14.0), w=320, h=240, dw=320, dh=240, opts=dict(max_keys=64)),
    "product": dict(seed=7, blobs=2000, sigma_px=(2.5, 14.0), w=640, h=480, dw=640, dh=480, opts={}),
}
PARITY = ("small", "odd", "medium", "dense", "hardcap")  # the fixtures whose orientations and descriptors are compared


def scene(name: str) -> Scene:
    f = FIXTURES[name]
    return Scene(f["seed"], f["blobs"], f["sigma_px"], f["w"], lattice_px=f.get("lattice_px"))


@functools.lru_cache(None)
def fixture(name: str, view: int = 0):
    """(intensity, depth, cfg) of a named fixture."""
    f = FIXTURES[name]
    img, depth = scene(name).render(pose(view), f["w"], f["h"], f["dw"], f["dh"])
    return img, depth, cfg(f["w"], f["h"], f["dw"], f["dh"], **f["opts"])


@functools.lru_cache(None)
def fixture_detect(name: str, dtype_name: str = "f64", descriptors: bool = True):
    img, depth, c = fixture(name)
    return detect(img, depth, c, F64 if dtype_name == "f64" else F32, descriptors=descriptors)


# ---- end to end: three views through the restatement and match_ref --------------------------------------------------
E2E_VIEWS = 3


@functools.lru_cache(None)
def e2e_views():
    """[(RGBX colour uint8 [240, 320, 4], depth float32 [240, 320], camera -> world)] of the medium scene."""
    f = FIXTURES["medium"]
    sc = scene("medium")
    return [sc.render_color(pose(k), f["w"], f["h"]) + (pose(k),) for k in range(E2E_VIEWS)]


def pose_error(T, prev: int, cur: int):
    """(translation error in m, rotation error in rad) of T (prev's camera space -> cur's) against the truth."""
    import match_ref as M
    rel = np.linalg.inv(pose(cur)) @ pose(prev)
    return float(np.linalg.norm(np.asarray(T, F64)[:3, 3] - rel[:3, 3])), M.rot_diff(T, rel)


@functools.lru_cache(None)
def e2e_reference() -> dict:
    """The restatement's own chain: intensity -> detect -> match_ref.run per consecutive pair. dict(images, counts,
    t_err, r_err) with the pose errors against the ground truth."""
    import match_ref as M
    f = FIXTURES["medium"]
    c = cfg(f["w"], f["h"])
    images = []
    for color, depth, _ in e2e_views():
        d = detect(intensity(color, f["w"], f["h"]), depth, c)
        images.append((d["keys"], d["descs"]))
    kinv = intrinsics_inv(f["w"], f["h"])
    counts, t_err, r_err = [], [], []
    for cur in range(1, E2E_VIEWS):
        out = M.run(images[:cur + 1], cur, cur - 1, [True] * (cur + 1), kinv)
        filt = out["pairs"][cur - 1]["filt"]
        counts.append(int(filt["count"]))
        te, re = pose_error(filt["T"], cur - 1, cur)
        t_err.append(te)
        r_err.append(re)
    return dict(images=images, counts=counts, t_err=t_err, r_err=r_err)


# ---- the measured bars of the transcendental stages ------------------------------------------------------------------
def us_diff(a, b):
    """Distance of two packed 16-bit orientations on the circle of 65535 steps."""
    d = np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64))
    return np.minimum(d, 65535 - d)


@functools.lru_cache(None)
def precision_spread() -> dict:
    """The restatement's own float32-against-float64 spread over the parity fixtures, on non-borderline items:
    ori = the largest difference of a packed orientation (16-bit steps), byte_share = the share of descriptor bytes
    that differ, byte_max = the largest byte difference. The GPU bars are 10 x ori and 10 x byte_share."""
    ori, differ, total, byte_max = 0, 0, 0, 0
    for name in PARITY:
        a, b = fixture_detect(name, "f64"), fixture_detect(name, "f32")
        for L in range(LEVELS):
            for ra, rb in zip(a["ori"][L], b["ori"][L]):
                if ra["border"] or rb["border"] or ra["us1"] == 65535:
                    continue
                if (ra["us2"] == 65535) != (rb["us2"] == 65535) or rb["us1"] == 65535:
                    continue  # a presence flip outside the margins would be a restatement bug: test_sift.py asserts none
                ori = max(ori, int(us_diff(ra["us1"], rb["us1"])))
                if ra["us2"] != 65535:
                    ori = max(ori, int(us_diff(ra["us2"], rb["us2"])))
        if a["packed"] and all(np.array_equal(x, y) for x, y in zip(a["packed"], b["packed"])):
            ok = ~(a["byte_border"] | b["byte_border"])
            d = np.abs(a["descs"].astype(np.int64) - b["descs"].astype(np.int64))[ok]
        else:  # orientations differ by a step somewhere: compare descriptors at the float64 run's orientations
            ls = tables()["level_sigma"]
            g, lists = a["g"], a["lists"]
            d = []
            for n, (L, i, _, o) in enumerate(a["entries"]):
                r = descriptor(g[L // 3][L % 3 + 1], int(lists[L][i][0]), int(lists[L][i][1]), ls[L % 3], o, F32)
                ok = ~(a["byte_border"][n] | r["border"])
                d.append(np.abs(a["descs"][n].astype(np.int64) - r["bytes"].astype(np.int64))[ok])
            d = np.concatenate(d) if d else np.zeros(0, np.int64)
        differ += int(np.count_nonzero(d))
        total += int(d.size)
        byte_max = max(byte_max, int(d.max()) if d.size else 0)
    return dict(ori=ori, byte_share=differ / max(total, 1), byte_differ=differ, byte_total=total, byte_max=byte_max)
