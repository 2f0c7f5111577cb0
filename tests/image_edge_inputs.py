"""Inputs of the image-kernel edge tests (test_image_edges.py, test_image_edges_gpu.py): small sensor frames
for the preprocessing (frames.hip) and the dense-term cache (cache.hip), and a many-pair problem for the
EntryJ producer (corr.hip). NumPy only, no library call: the same arrays on every machine.

test_image_edges.py checks, with the oracle alone, that these inputs put pixels (pairs) on both sides of
every branch the GPU tests rely on."""
from __future__ import annotations

import numpy as np

FX = 577.87  # the 640-wide sensor's focal length; scaled with the image width


def sensor_frame(W: int, H: int, seed: int = 0):
    """(ushort depth [H, W] in mm, RGBX colour [H, W, 4]): a slanted plane 1500 + 6x + 4y with a 400 mm step
    along a slanted line, +-3 mm integer noise, 3 % dropouts (0), one 5x4 hole; uniformly random colour bytes."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    d = 1500 + 6 * xx + 4 * yy
    d[yy > 0.6 * H + 0.2 * xx] -= 400
    d = d + rng.integers(-3, 4, d.shape)
    d[rng.random(d.shape) < 0.03] = 0
    d[H // 3:H // 3 + 4, W // 2:W // 2 + 5] = 0
    c = rng.integers(0, 256, (H, W, 4)).astype(np.uint8)
    return d.astype(np.uint16), c


def flat_frame(W: int, H: int):
    """Depth 2000 mm everywhere and one constant colour: any tap taken from outside the image shows."""
    d = np.full((H, W), 2000, np.uint16)
    c = np.empty((H, W, 4), np.uint8)
    c[...] = (90, 160, 30, 255)
    return d, c


def depth_metres(u16: np.ndarray, shift: float = 1000.0) -> np.ndarray:
    """The sensor conversion (d / depthShift, 0 -> -inf): the cache's float input."""
    return np.where(u16 == 0, np.float32(-np.inf), u16.astype(np.float32) / np.float32(shift)).astype(np.float32)


# ---- preprocessing shapes ---------------------------------------------------------------------------
# The kernels' workgroup tile is 32 x 8; a workgroup takes the unchecked path when its tile and radius-R halo
# lie inside the image: 32 bx - R >= 0, 32 bx + 32 + R <= W, 8 by - R >= 0, 8 by + 8 + R <= H.
def boundary_sizes(R: int):
    """(64 + R) x (16 + R): the smallest image with an interior workgroup (exactly tile (1, 1)); one pixel
    narrower or one lower and there is none."""
    return [(64 + R, 16 + R), (63 + R, 16 + R), (64 + R, 15 + R)]


def interior_tiles(W: int, H: int, R: int) -> int:
    """How many 32 x 8 workgroup tiles take the unchecked path at radius R."""
    n = 0
    for by in range((H + 7) // 8):
        for bx in range((W + 31) // 32):
            n += 32 * bx - R >= 0 and 8 * by - R >= 0 and 32 * bx + 32 + R <= W and 8 * by + 8 + R <= H
    return n


OFF_GRID_SIZES = [(5, 3), (31, 7), (33, 9), (100, 37)]
RESAMPLE_SIZES = [(67, 19), (100, 37)]

# ---- cache shapes: (input W, H), (cache W, H), (colour W, H) -----------------------------------------------
CACHE_TAIL = ((67, 51), (21, 13), (90, 70))       # 273 cache pixels = 4 x 64 + 17; partial 8 x 8 tiles in x and y
CACHE_SHAPES = [((64, 48), (9, 7), (64, 48)),
                ((40, 30), (40, 30), (40, 30)),   # no downsampling
                ((640, 480), (80, 60), (1296, 968))]


# ---- EntryJ producer -----------------------------------------------------------------------------------
CORR_W, CORR_H = 72, 52
# (stride, maxPerPair, minPerPair): N = 54 (< 256), 234 (< 256, maxPerPair at its cap), 140 (maxPerPair 1),
# 408 (two rounds of 256 candidates, the second partial; 72 is no multiple of 5)
CORR_OPTION_SETS = [(8, 25, 5), (4, 64, 1), (5, 1, 1), (3, 64, 1)]
# (cur, start): 1099, 65, 67, 64, 65, 1025, 1024, 1, 0 pairs: both sides of the wave (64) and round (1024) edges
CORR_WINDOWS = [(1099, 0), (1099, 1034), (70, 3), (64, 0), (65, 0), (1025, 0), (1024, 0), (1, 0), (5, 5)]


def corr_intrinsics():
    f = FX * CORR_W / 640
    return f, f, (CORR_W - 1) / 2, (CORR_H - 1) / 2


def corr_problem(n: int = 1100):
    """(images, sel, T, Tinv): four 72 x 52 depth images (a wall at 2 m, the plane 1.5 + 0.01 x, the wall with
    every (3rd row, 2nd column) pixel invalid, all invalid); frame k shows image sel[k] = 5k % 4, the last frame
    the wall; identity rotations with tx = (7k % 41) * 0.08, ty = (3k % 5) * 0.01. The image spans 2.2 m at the wall and
    the frames up to 3.2 m, so pairs have no match (an empty image, or no overlap), maxPerPair matches, or, where
    a few grid columns overlap, something in between: at stride 8 also 1 .. 4, which minPerPair = 5 drops."""
    W, H = CORR_W, CORR_H
    xx = np.mgrid[0:H, 0:W][1].astype(np.float32)
    wall = np.full((H, W), 2.0, np.float32)
    plane = (np.float32(1.5) + np.float32(0.01) * xx).astype(np.float32)
    holes = wall.copy()
    holes[::3, ::2] = -np.inf
    none = np.full((H, W), -np.inf, np.float32)
    idx = np.arange(n)
    sel = (idx * 5) % 4
    sel[-1] = 0
    T = np.stack([np.eye(4, dtype=np.float32)] * n)
    T[:, 0, 3] = ((idx * 7) % 41) * 0.08
    T[:, 1, 3] = ((idx * 3) % 5) * 0.01
    return [wall, plane, holes, none], sel, T, pose_inverse(T)


def pose_inverse(T: np.ndarray) -> np.ndarray:
    """[R | t] -> [R^T | -R^T t] in double, rounded once; a non-finite pose stays non-finite everywhere
    (the project marks an invalid pose with -inf in T and Tinv)."""
    T = np.asarray(T, np.float32)
    out = np.empty_like(T)
    for k in range(len(T)):
        if not np.all(np.isfinite(T[k])):
            out[k] = -np.inf
            continue
        M = T[k].astype(np.float64)
        Ti = np.eye(4)
        Ti[:3, :3] = M[:3, :3].T
        Ti[:3, 3] = -M[:3, :3].T @ M[:3, 3]
        out[k] = Ti.astype(np.float32)
    return out
