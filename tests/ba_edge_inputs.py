"""Inputs of the bundle adjuster's edge tests (test_ba_edges.py, test_ba_edges_gpu.py): correspondence graphs
built pair by pair, so that correspondence counts, row lengths, pair run lengths, row degrees and image counts
land exactly on the constants at which the kernels of csrc/ba_table.h, ba_pcg.h and ba_persist.h branch.
ba_problem.make_problem gives the co-visibility graph of the synthetic room (every image connected, i < j,
pairs contiguous); nothing here uses the scene. NumPy only: the same arrays on every machine.

A problem is the dict gpu_solve / oracle_solve of test_ba_gpu.py take: K, corr (ENTRYJ_DTYPE), rot, trans
(float32 [K, 3] initial poses), valid, plus gt_rot / gt_trans. Poses are drawn as pose vectors and turned into
matrices with the se(3) exponential of LieDerivUtil.h's poseToMatrix restated in float64.

test_ba_edges.py checks, with the oracle alone, that each of these inputs reaches the edge it is named for."""
from __future__ import annotations

import numpy as np

from bundlefusion_amd.abi import ENTRYJ_DTYPE

INVALID = 0xFFFFFFFF

# ---- the kernel constants the cases straddle ---------------------------------------------------------------
WAVE = 64            # k_tile_fill places 64 correspondences per step; pair runs are streamed 64 per step
TILE = 256           # ba_dev.h TILE: correspondences per table-build tile up to 256 images ...
TILE_IMAGES = 256    # ... and tile_for(n) = TILE * ceil(n / 256) above: 512 at 257 images
CH = 512             # ba_dev.h CH: row entries per chunk
ROW_PAIR_ROUND = 128  # pair_row_ap (ba_pcg.h): row-pair entries per round
PP_REGS = 192        # ba_persist.h PP_CPL * 64: partners k_pcg_persist keeps in registers
PP_REFS = 448        # ... + PP_OV * 64: the partners kept as pair refs; beyond, the tail loop
SMALL_N = 64         # k_pcg_small (one workgroup) up to here, the grid routes above
ONE_FINISHER_N = 513   # 2 * WG + 1: one-finisher persistent launch / k_pcg_pairs<2> up to here
FINISHER8_N = 2049     # 8 * WG + 1: k_pcg_pairs<8>'s pcg_finisher<8> keeps its rows in registers up to here and
#                        takes its multi-pass form above. (The four persistent finishers own rows 1 .. 2048 too, but
#                        the persistent launch ends sooner: it has to be co-resident.)
PP_NF = 4              # ba_persist.h: finisher workgroups of the wide persistent launch
PP_SHADOW = 256        # ba_persist.h: a grid beyond this many workgroups gets one row-less workgroup per finisher
PERSIST_CAPACITY = 512  # launchPairPcg's persistCapacity_ on MI355X: 256 CUs x 2 co-resident k_pcg_persist workgroups


def persist_grid(N: int) -> int:
    """launchPairPcg's persistGrid above ONE_FINISHER_N images: PP_NF finishers, one wave per image row but the
    first (4 waves per workgroup), and the row-less workgroups."""
    assert N > ONE_FINISHER_N
    grid = PP_NF + -(-(N - 1) // 4)
    return grid + PP_NF if grid > PP_SHADOW else grid


# the wide persistent launch runs while persist_grid(N) <= PERSIST_CAPACITY: 4 + 504 + 4 = 512 workgroups at 2 017
# images (the fourth finisher nearly full), 513 at 2 018, where the dispatcher takes one launch per iteration
WIDE_PERSIST_N = max(n for n in range(ONE_FINISHER_N + 1, FINISHER8_N + 1) if persist_grid(n) <= PERSIST_CAPACITY)
NLIN_PERSIST = 254    # a persistent tag is epoch * 256 + iteration + 1: nLin >= 255 takes per-iteration launches
CAP = 1000             # maxCorrPerImage = clamp(maxCorr / maxImages, 1000, 4000) with maxCorr = CAP * maxImages


def cap_max_corr(max_images: int) -> int:
    """The max_corr that makes a handle of max_images cap its rows at CAP entries."""
    return CAP * max_images


# ---- named cases -------------------------------------------------------------------------------------------
# A. table build. One list on 6 images (band w = 2, m = 57: 9 pairs x 57 = 513 correspondences), interleaved so
# every prefix touches several rows; its prefixes sit at the 64-lane step and the 256 tile, +-1.
SIX = dict(N=6, m=57, w=2)
PREFIX_COUNTS = (1, 63, 64, 65, 255, 256, 257, 511, 513)
# tile_for: 256 images build with tile 256 (511 / 512 / 513 correspondences = 2, 2, 3 tiles), 257 images with
# tile 512 (1, 1, 2 tiles). Band m = 1, w = 3 listed distance by distance, so a prefix of 511 holds every
# (k, k + 1) and (k, k + 2) and each image keeps a row. (w = 2 gives only 2 N - 3 = 509 / 511 correspondences.)
TILE_N = (256, 257)
TILE_COUNTS = (511, 512, 513)
# B. one graph for row and pair-run lengths, one for row degrees (see rows_problem, degree_problem)
ROW_LENGTHS = (1, 511, 512, 513, 1024, 1025)           # CH and 2 CH, +-1
RUN_LENGTHS = (1, 63, 64, 65, 128, 129)                # WAVE and 2 WAVE, +-1
ROWS_N = 70
ROW_RUNS = {                                            # edge image -> its runs (one per trunk partner)
    10: (1,),
    11: (63, 64, 65, 128, 129, 62),                     # 511
    12: (512,),
    13: (129, 128, 65, 64, 63, 1, 63),                  # 513
    14: (512, 512),                                     # 1024
    15: (1025,),
}
DEGREES = (1, 127, 128, 129, 192, 193, 448, 449)       # ROW_PAIR_ROUND, PP_REGS, PP_REFS, +-1 / +1
DEGREE_CHAIN = 451                                      # images 0..450 in a chain; hubs follow
DEGREE_N = DEGREE_CHAIN + len(DEGREES) - 1              # 458 (the chain's last image has degree 1)
# C. route boundaries: band m = 3, w = 3 (18 432 correspondences at 2 050 images), at SMALL_N, ONE_FINISHER_N,
# WIDE_PERSIST_N and FINISHER8_N, each with the image count after it
ROUTE_N = (64, 65, 513, 514, 2017, 2018, 2049, 2050)
ROUTE_BAND = dict(m=3, w=3)
# cap cascade: row 1 holds 1200 entries and drops the last 200 of (1, 2); row 2 ranks (2, 3) behind all 600 of
# (1, 2), dropped or not, so 100 of (2, 3) go although row 2 keeps only 900 entries
CASCADE = ((0, 1, 600), (1, 2, 600), (2, 3, 500))
CASCADE_DROPS = (0, 200, 100)
# valid[v] = 0: only image 5 is off its ground truth (+1 cm), so with image 5 invalid the GN exit test
# (max |delta| over valid images) passes one step earlier
INVALID_IMAGE = dict(N=8, m=40, w=3, image=5, shift=0.01, schedule=(3, 30))


# ---- poses -------------------------------------------------------------------------------------------------
def pose_matrices(rot: np.ndarray, trans: np.ndarray) -> np.ndarray:
    """poseToMatrix (LieDerivUtil.h:160-207) in float64: R = exp([w]x), t = (I + B [w]x + C [w]x^2) trans."""
    w = np.asarray(rot, np.float64)
    u = np.asarray(trans, np.float64)
    th2 = (w * w).sum(axis=1)
    th = np.sqrt(th2)
    small = th2 < 1e-12
    s = np.where(small, 1.0, th)
    A = np.where(small, 1.0 - th2 / 6.0, np.sin(s) / s)
    B = np.where(small, 0.5 - th2 / 24.0, (1.0 - np.cos(s)) / (s * s))
    Cc = np.where(small, 1.0 / 6.0 - th2 / 120.0, (1.0 - A) / (s * s))
    W = np.zeros((len(w), 3, 3))
    W[:, 0, 1], W[:, 0, 2] = -w[:, 2], w[:, 1]
    W[:, 1, 0], W[:, 1, 2] = w[:, 2], -w[:, 0]
    W[:, 2, 0], W[:, 2, 1] = -w[:, 1], w[:, 0]
    W2 = W @ W
    eye = np.eye(3)[None]
    T = np.zeros((len(w), 4, 4))
    T[:, :3, :3] = eye + A[:, None, None] * W + B[:, None, None] * W2
    V = eye + B[:, None, None] * W + Cc[:, None, None] * W2
    T[:, :3, 3] = np.einsum("nij,nj->ni", V, u)
    T[:, 3, 3] = 1.0
    return T


def poses(N: int, seed: int, drift=(0.003, 0.004)):
    """(gt_rot, gt_trans, rot, trans): seeded ground-truth pose vectors (cameras within ~0.3 m of the origin,
    turned by a few degrees, all facing +z) and the initial poses = ground truth + N(0, drift) per component
    (rad, m). Image 0 is undrifted."""
    rng = np.random.default_rng(seed)
    gt_rot = rng.normal(size=(N, 3)) * 0.04
    gt_trans = rng.normal(size=(N, 3)) * 0.12
    d_rot = rng.normal(size=(N, 3)) * drift[0]
    d_trans = rng.normal(size=(N, 3)) * drift[1]
    d_rot[0] = 0.0
    d_trans[0] = 0.0
    return (gt_rot.astype(np.float32), gt_trans.astype(np.float32),
            (gt_rot + d_rot).astype(np.float32), (gt_trans + d_trans).astype(np.float32))


# ---- correspondences ---------------------------------------------------------------------------------------
def correspondences(triples, gt_rot, gt_trans, seed: int, noise=0.0015) -> np.ndarray:
    """For every (a, b, m) of triples, in that order: m world points in a 1.6 x 1.2 x 0.8 m box 2.5 m ahead of
    the cameras, expressed in camera a (pos_i) and camera b (pos_j, + N(0, noise) per component)."""
    tr = np.asarray(list(triples), np.int64).reshape(-1, 3)
    A = np.repeat(tr[:, 0], tr[:, 2])
    Bi = np.repeat(tr[:, 1], tr[:, 2])
    M = len(A)
    rng = np.random.default_rng(seed)
    P = (rng.uniform(-1.0, 1.0, size=(M, 3)) * [0.8, 0.6, 0.4]) + [0.0, 0.0, 2.5]
    T = pose_matrices(gt_rot.astype(np.float64), gt_trans.astype(np.float64))
    R, t = T[:, :3, :3], T[:, :3, 3]
    pa = np.einsum("nji,nj->ni", R[A], P - t[A])
    pb = np.einsum("nji,nj->ni", R[Bi], P - t[Bi]) + rng.normal(size=(M, 3)) * noise
    out = np.zeros(M, ENTRYJ_DTYPE)
    out["i"], out["j"] = A, Bi
    out["pos_i"], out["pos_j"] = pa, pb
    return out


def band(N: int, m: int, w: int, by_distance=False):
    """(k, k + d, m) for d <= w: image by image, or (by_distance) every (k, k + 1) first, then (k, k + 2), ..."""
    if by_distance:
        return [(k, k + d, m) for d in range(1, w + 1) for k in range(N - d)]
    return [(k, k + d, m) for k in range(N) for d in range(1, w + 1) if k + d < N]


def hub(h: int, partners, m):
    """Row h with one run per partner (degree len(partners)); m an int or one run length per partner."""
    partners = list(partners)
    ms = [m] * len(partners) if np.isscalar(m) else list(m)
    assert len(ms) == len(partners) and h not in partners
    return [(min(h, p), max(h, p), k) for p, k in zip(partners, ms)]


def reorient(corr: np.ndarray, how: str, seed=0) -> np.ndarray:
    """'reverse': every correspondence as (j, i); 'mixed': a seeded half of them, so both orientations occur
    inside one pair's run."""
    out = corr.copy()
    flip = np.ones(len(corr), bool) if how == "reverse" else np.random.default_rng(seed).random(len(corr)) < 0.5
    assert how in ("reverse", "mixed")
    out["i"][flip], out["j"][flip] = corr["j"][flip], corr["i"][flip]
    out["pos_i"][flip], out["pos_j"][flip] = corr["pos_j"][flip], corr["pos_i"][flip]
    return out


def interleave(corr: np.ndarray) -> np.ndarray:
    """Round robin over the pairs: the first correspondence of every pair, then the second of every pair, ..."""
    lo = np.minimum(corr["i"], corr["j"]).astype(np.int64)
    hi = np.maximum(corr["i"], corr["j"]).astype(np.int64)
    key = lo * (1 << 32) + hi
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.r_[0, np.flatnonzero(ks[1:] != ks[:-1]) + 1]
    rank = np.empty(len(corr), np.int64)
    rank[order] = np.arange(len(corr)) - np.repeat(start, np.diff(np.r_[start, len(corr)]))
    return corr[np.lexsort((key, rank))].copy()


def shuffled(corr: np.ndarray, seed=3) -> np.ndarray:
    return corr[np.random.default_rng(seed).permutation(len(corr))].copy()


def invalidated(corr: np.ndarray, idx) -> np.ndarray:
    """corr with the entries idx arriving already invalid (both indices INVALID, as setInvalid leaves them)."""
    out = corr.copy()
    out["i"][idx] = INVALID
    out["j"][idx] = INVALID
    return out


def problem(N: int, triples, seed=1, drift=(0.003, 0.004), noise=0.0015) -> dict:
    gt_rot, gt_trans, rot, trans = poses(N, seed, drift)
    corr = correspondences(triples, gt_rot, gt_trans, seed + 1000, noise)
    return dict(K=N, corr=corr, rot=rot, trans=trans, valid=np.ones(N, np.int32), gt_rot=gt_rot, gt_trans=gt_trans)


def with_corr(prob: dict, corr: np.ndarray) -> dict:
    out = dict(prob)
    out["corr"] = corr
    return out


# ---- the cases ---------------------------------------------------------------------------------------------
def six_problem() -> dict:
    """6 images, 513 correspondences, pairs interleaved."""
    p = problem(SIX["N"], band(SIX["N"], SIX["m"], SIX["w"]), seed=11)
    return with_corr(p, interleave(p["corr"]))


def six_pairs_contiguous() -> dict:
    return problem(SIX["N"], band(SIX["N"], SIX["m"], SIX["w"]), seed=11)


def tile_problem(N: int) -> dict:
    return problem(N, band(N, 1, 3, by_distance=True), seed=12)


PRE_INVALID = {  # on six_problem's 513 correspondences (tile 256, 64 per placement step)
    "every_third": np.arange(0, 513, 3),
    "one_step": np.arange(64, 128),
    "one_tile": np.arange(256, 512),
    "last": np.array([512]),
}


def cap_problem(name: str) -> dict:
    """4 images solved on a handle of cap_max_corr(4): 'exact' a row of CAP entries, 'plus1' CAP + 1,
    'cascade' / 'cascade_shuffled' the CASCADE list in list order and shuffled."""
    triples = {"exact": ((0, 1, 500), (1, 2, 500), (2, 3, 300)), "plus1": ((0, 1, 500), (1, 2, 501), (2, 3, 300)),
               "cascade": CASCADE, "cascade_shuffled": CASCADE}[name]
    p = problem(4, triples, seed=13)
    return with_corr(p, shuffled(p["corr"])) if name == "cascade_shuffled" else p


ROWLESS = ("middle", "last", "first", "two_components", "single")


def rowless_problem(name: str):
    """(problem, images without a row)."""
    N = 6
    full = band(N, 20, 2)
    if name == "middle":
        tr, none = [t for t in full if 3 not in t[:2]], [3]
    elif name == "last":
        tr, none = [t for t in full if 5 not in t[:2]], [5]
    elif name == "first":
        tr, none = [t for t in full if 0 not in t[:2]], [0]
    elif name == "two_components":
        tr, none = [t for t in full if (t[0] < 3) == (t[1] < 3)], []
    else:
        tr, none = [(2, 4, 1)], [0, 1, 3, 5]
    assert name in ROWLESS
    return problem(N, tr, seed=14), none


def orientation_problem(name: str) -> dict:
    p = six_pairs_contiguous()
    corr = {"reverse": lambda c: reorient(c, "reverse"), "mixed": lambda c: reorient(c, "mixed", seed=5),
            "interleaved": interleave}[name](p["corr"])
    return with_corr(p, corr)


def invalid_image_problem(invalid: bool) -> dict:
    c = INVALID_IMAGE
    p = problem(c["N"], band(c["N"], c["m"], c["w"]), seed=15, drift=(0.0, 0.0))
    p["trans"] = p["trans"].copy()
    p["trans"][c["image"]] += np.float32(c["shift"])
    if invalid:
        p["valid"] = p["valid"].copy()
        p["valid"][c["image"]] = 0
    return p


def rows_problem() -> dict:
    """ROWS_N = 70 images (the grid routes). Images 0..9 are a trunk (band m = 8, w = 2); images 10..15 have the
    rows of ROW_RUNS, one run per trunk partner; images 16..69 are a band of their own (m = 3, w = 2) tied to the
    trunk. A seeded half of the correspondences is turned round, so the runs hold both orientations."""
    tr = band(10, 8, 2)
    nxt = 1
    for img, runs in ROW_RUNS.items():
        partners = [1 + (nxt + k) % 9 for k in range(len(runs))]
        nxt += len(runs)
        tr += hub(img, partners, runs)
    tr += [(16 + a, 16 + b, m) for a, b, m in band(ROWS_N - 16, 3, 2)]
    tr += [(1 + k % 9, 16 + k, 4) for k in range(ROWS_N - 16)]
    p = problem(ROWS_N, tr, seed=16)
    return with_corr(p, reorient(p["corr"], "mixed", seed=6))


def degree_problem() -> dict:
    """DEGREE_N = 458 images: a chain 0..450 (m = 2) whose last image keeps degree 1, and one hub per entry of
    DEGREES[1:], tied to chain images 0..d-1 with runs of 1, 2 or 3."""
    tr = band(DEGREE_CHAIN, 2, 1)
    for k, d in enumerate(DEGREES[1:]):
        tr += hub(DEGREE_CHAIN + k, range(d), [1 + (q + k) % 3 for q in range(d)])
    p = problem(DEGREE_N, tr, seed=17)
    return with_corr(p, reorient(p["corr"], "mixed", seed=7))


def route_problem(N: int) -> dict:
    return problem(N, band(N, ROUTE_BAND["m"], ROUTE_BAND["w"]), seed=18)


# ---- the dense term above 513 images ------------------------------------------------------------------------
# The dense term needs cache frames, so this one case does use the synthetic room (ba_problem.make_problem, as
# test_many_images_multipass_finisher's 560 images). Cache sizes tried in this order; DENSE_SIZE is the smallest
# at which the oracle's overlap search finds a pair (test_ba_edges.py asserts that it is).
DENSE_N = 514
DENSE_SIZES = ((20, 15), (40, 30), (80, 60))
DENSE_SIZE = (20, 15)


def dense_problem(size=DENSE_SIZE) -> dict:
    import bundlefusion_amd as bfa
    from ba_problem import make_problem
    W, H = size
    f = 577.87 * W / 640.0
    cam = bfa.depth_camera(W, H, fx=f, fy=f, mx=(W - 1) / 2.0, my=(H - 1) / 2.0)
    return make_problem(K=DENSE_N, stride=1, max_per_pair=4, outliers=0.0, with_cache=True, cache_cam=cam,
                        drift=(0.05, 0.002))


# ---- what a list's table looks like (NumPy restatement, for the tests) -------------------------------------
def survivors(corr: np.ndarray) -> np.ndarray:
    return corr[corr["i"] != INVALID]


def row_lengths(corr: np.ndarray, N: int) -> np.ndarray:
    c = survivors(corr)
    return np.bincount(np.concatenate([c["i"], c["j"]]).astype(np.int64), minlength=N)


def pair_counts(corr: np.ndarray) -> dict:
    """{(a, b): surviving correspondences}, a < b, in (a, b) order."""
    c = survivors(corr)
    lo = np.minimum(c["i"], c["j"]).astype(np.int64)
    hi = np.maximum(c["i"], c["j"]).astype(np.int64)
    keys, n = np.unique(np.stack([lo, hi], axis=1), axis=0, return_counts=True)
    return {(int(a), int(b)): int(k) for (a, b), k in zip(keys, n)}


def row_degrees(corr: np.ndarray, N: int) -> np.ndarray:
    deg = np.zeros(N, np.int64)
    for a, b in pair_counts(corr):
        deg[a] += 1
        deg[b] += 1
    return deg


def cap_replay(corr: np.ndarray, N: int, cap: int) -> np.ndarray:
    """BuildVariablesToCorrespondencesTableDevice in index order: the invalid mask after the build. Both of a
    correspondence's rows count it before the cap test, so a dropped one still takes a rank in its other row."""
    n = np.zeros(N, np.int64)
    out = corr["i"] == INVALID
    for x in np.flatnonzero(~out):
        i, j = int(corr["i"][x]), int(corr["j"][x])
        o0, o1 = n[i], n[j]
        n[i] += 1
        n[j] += 1
        out[x] = not (o0 < cap and o1 < cap)
    return out
