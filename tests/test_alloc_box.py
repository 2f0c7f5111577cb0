"""The bound behind the alloc walk's pre-test (bundlefusion_amd/csrc/tsdf.hip alloc_collect): every block a
ray's DDA visits lies in the box spanned by the ray's first block and the block of its far end, so a
16x16-pixel tile's rays stay inside the union of their boxes. Held against the oracle's own walk
(oracle/tsdf.cpp allocPixelWalk): an empty oracle scene integrates a depth image with no colour (alloc and
frustum list only), and the blocks it allocated are the blocks its walks visited inside the frustum.
The end points come from tests/alloc_box.py, a float32 restatement of the walk's first lines."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
from alloc_box import ray_boxes, ray_ends, tile_boxes
from oracle_lib import OracleScene, lib as oracle_lib

N = 16  # image edge: one tile


def _cam():
    # a wide camera: the pixels used (4..11) and their blocks sit well inside the frustum test's 0.95 margin
    return bfa.depth_camera(N, N, fx=40.0, fy=40.0, mx=7.0, my=8.0, zmin=0.1, zmax=8.0)


def _params(voxel, truncation=0.06, trunc_scale=0.02, blocks=1024):
    return bfa.hash_params(voxel_size=voxel, num_buckets=blocks // 2 + 1, num_blocks=blocks, truncation=truncation, trunc_scale=trunc_scale,
                           max_integration_distance=8.0)


def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _pose(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


AXIS_ROTS = [np.eye(3), np.diag([1.0, -1.0, -1.0]),  # +z, -z
             np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]]), np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]]),  # +x, -x
             np.array([[1.0, 0, 0], [0, 0, 1], [0, -1, 0]]), np.array([[1.0, 0, 0], [0, 0, -1], [0, 1, 0]])]  # +y, -y


def _visited(ora, T, depth, cam):
    """blocks the oracle's walks of this image visit (inside the frustum), from an empty scene"""
    oracle_lib().or_scene_reset(C.c_void_p(ora.h))
    ora.integrate(T, depth, None, cam)
    v = ora.export_visible()
    assert len(v) < ora.params.numSDFBlocks - 1, "the test scene's heap ran out"
    return {(int(e["x"]), int(e["y"]), int(e["z"])) for e in v}


def _cases(rng, n_random, voxel):
    """(pose, depth, pixel) of single rays: random ones, then axis-parallel ones through the principal point"""
    for _ in range(n_random):
        yield (_pose(_rot(rng), rng.uniform(-3.0, 3.0, size=3)), float(rng.uniform(0.3, 6.0)),
               (int(rng.integers(4, 12)), int(rng.integers(4, 12))))
    for R in AXIS_ROTS:
        for _ in range(12):
            # on the block grid's lines, beside them, and anywhere
            t = rng.integers(-40, 40, size=3) * (8 * voxel) + rng.choice([0.0, -0.5 * voxel, 0.37 * voxel])
            yield _pose(R, t), float(rng.uniform(0.3, 6.0)), (7, 8)


@pytest.mark.parametrize("voxel", [0.004, 0.002])
@pytest.mark.parametrize("truncation, trunc_scale", [(0.06, 0.02), (0.003, 0.0)])
def test_ray_walk_stays_in_the_box_of_its_end_blocks(voxel, truncation, trunc_scale):
    """Single rays: (0.06, 0.02) is the bench's band (walks of up to ~25 blocks at 2 mm), (0.003, 0) a 6 mm
    ray whose first and last block mostly coincide."""
    cam, p = _cam(), _params(voxel, truncation, trunc_scale)
    ora = OracleScene(p)
    rng = np.random.default_rng(int(voxel * 1e4) + int(truncation * 1e4))
    n = same = negative = axis = blocks = 0
    for T, d, (x, y) in _cases(rng, 900, voxel):
        depth = np.full((N, N), -np.inf, np.float32)
        depth[y, x] = d
        active, b0, b1 = ray_ends(T, depth, cam, p)
        assert active[y, x] and active.sum() == 1
        lo, hi = ray_boxes(active, b0, b1)
        lo, hi = lo[y, x], hi[y, x]
        seen = _visited(ora, T, depth, cam)
        # the restated end points are the oracle's: its walk starts in the first block
        assert tuple(int(v) for v in b0[y, x]) in seen, (T, d, x, y)
        for b in seen:
            assert all(lo[a] <= b[a] <= hi[a] for a in range(3)), (b, lo, hi, T, d, x, y)
        n += 1
        blocks += len(seen)
        same += bool(np.all(b0[y, x] == b1[y, x]))
        negative += bool(np.any(lo < 0))
        axis += int(np.sum(b0[y, x] == b1[y, x]) >= 2 and (x, y) == (7, 8))
    assert n == 900 + 72 and negative > 300 and axis >= 60
    if truncation < 0.01:
        assert same > 300, same
    else:
        assert blocks > 4 * n, blocks


@pytest.mark.parametrize("voxel", [0.004, 0.002])
def test_tile_walks_stay_in_the_tile_box(voxel):
    """Whole 16x16 tiles (smooth depth, a step edge, holes): every visited block lies in the tile's box."""
    p = _params(voxel, blocks=16384)
    ora = OracleScene(p)
    rng = np.random.default_rng(7 + int(voxel * 1e4))
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float32)
    total = 0
    # a narrow camera (a few mm per pixel, the bench's footprint), so a tile's walks fit the test heap
    ncam = bfa.depth_camera(N, N, fx=577.87, fy=577.87, mx=7.5, my=7.5, zmin=0.1, zmax=8.0)
    for k in range(40):
        T = _pose(_rot(rng), rng.uniform(-3.0, 3.0, size=3)) if k % 4 else _pose(AXIS_ROTS[(k // 4) % 6], rng.uniform(-2, 2, size=3))
        d0 = rng.uniform(0.3, 6.0)
        depth = (d0 + 0.002 * d0 * (rng.normal() * xx + rng.normal() * yy)).astype(np.float32)
        if k % 3 == 1:
            depth[:, 9:] += np.float32(0.15)  # a step edge through the tile
        if k % 3 == 2:
            depth[rng.random((N, N)) < 0.3] = -np.inf
        depth = np.clip(depth, 0.3, 6.0).astype(np.float32) + np.where(np.isinf(depth), -np.inf, 0).astype(np.float32)
        active, b0, b1 = ray_ends(T, depth, ncam, p)
        (lo, hi), = tile_boxes(active, b0, b1).values()
        seen = _visited(ora, T, depth, ncam)
        assert seen
        for b in seen:
            assert all(lo[a] <= b[a] <= hi[a] for a in range(3)), (b, lo, hi, k)
        total += len(seen)
    assert total > 40 * 10
