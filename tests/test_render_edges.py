"""The inputs of test_render_edges_gpu.py (render_edge_inputs.py) reach the edges they are named for: checked
here with the CPU oracle (oracle/tsdf.cpp) alone.

A bit-exact GPU comparison proves nothing about a branch its input never takes: a room near the origin cannot
tell a broken un-keyed block lookup from a working one, and a render without a pixel in its last partial tile
cannot tell a dropped tile edge from a kept one. Every assertion below is a condition on an input, not a
tolerance on a kernel; a change to the synthetic scene that empties one of the GPU tests fails here first."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bundlefusion_amd as bfa
import render_edge_inputs as R
from oracle_lib import OracleScene, blocks_of
from test_mc import wall_scene


@functools.lru_cache(maxsize=None)
def world(offset):
    o = OracleScene(R.room_params())
    cam = R.room_camera()
    for T, d, c in R.room_frames(offset):
        o.integrate(T, d, c, cam)
    o.garbageCollect()
    return o


def render(o, T, W, H, by_height=False):
    cam, rp = R.view(W, H, by_height)
    res = o.raycast(T, cam, rp, want_intervals=True)
    return res, rp


def block_coords(o):
    return np.array(sorted(blocks_of(o.export()[0])), np.int64)


def test_room_is_the_one_the_existing_tests_use():
    assert 4000 < len(block_coords(world(0.0))) < 5500


@pytest.mark.parametrize("offset", R.OFFSETS[1:])
def test_offset_worlds_straddle_the_key_range(offset):
    b = block_coords(world(offset))
    k = R.keyed(b)
    assert k.sum() >= 1000 and (~k).sum() >= 1000, (k.sum(), (~k).sum())
    if offset > 0:
        assert b[:, 0].min() < R.KEY_HI < b[:, 0].max()
        assert np.any(b[:, 0] == R.KEY_HI) and np.any(b[:, 0] == R.KEY_HI + 1)   # both sides of the upper end
    else:
        assert np.any(b[:, 0] == R.KEY_LO) and np.any(b[:, 0] == R.KEY_LO - 1)   # both sides of -4096
        assert b[:, 0].max() < 0
    # y and z stay inside the range: x alone decides
    assert np.all((b[:, 1:] >= R.KEY_LO) & (b[:, 1:] <= R.KEY_HI))
    # the shifted room is the same room: the render pose sees as much of it
    res, rp = render(world(offset), R.render_pose(offset), R.ROOM_W, R.ROOM_H)
    assert np.isfinite(res[0]).mean() > 0.98
    near, far = R.clamped(res[4], res[5], rp)
    assert near.sum() == 0 and far.sum() == 0


@pytest.mark.parametrize("W,H", R.RENDER_SIZES)
def test_render_sizes_hit_their_last_row_and_column(W, H):
    res, rp = render(world(0.0), R.render_pose(), W, H)
    hit = np.isfinite(res[0])
    assert hit.mean() >= 0.7
    assert hit[:, -1].sum() >= 1
    if (W, H) != (17, 17):   # 17x17: no hit in the last row (the floor is not reached), 13 in the last column
        assert hit[-1].sum() >= 1
    near, far = R.clamped(res[4], res[5], rp)
    assert near.sum() == 0 and far.sum() == 0     # no clamped depth: the raw intervals must be equal too


@pytest.mark.parametrize("W,H", R.TALL_SIZES)
def test_tall_renders_hit_the_first_and_last_tile_row(W, H):
    res, rp = render(world(0.0), R.render_pose(), W, H, by_height=True)
    hit = np.isfinite(res[0])
    rows = -(-H // R.SPLAT_TILE_H)
    assert rows == (256 if H == 2048 else 257)
    assert hit[: R.SPLAT_TILE_H].sum() >= 100 and hit[(rows - 1) * R.SPLAT_TILE_H:].sum() >= 100
    if H > 2048:
        assert hit[2048:].sum() >= 100
    near, far = R.clamped(res[4], res[5], rp)
    assert near.sum() == 0 and far.sum() == 0


def test_inside_pose_has_blocks_before_the_near_plane():
    res, rp = render(world(0.0), R.inside_pose(), R.ROOM_W, R.ROOM_H)
    near, far = R.clamped(res[4], res[5], rp)
    assert near.sum() >= 1000 and far.sum() == 0
    assert np.isfinite(res[0]).mean() > 0.9


def test_thresholds_reject_more_and_more():
    o = world(0.0)
    with ThreadPoolExecutor(4) as ex:   # the oracle call releases the interpreter lock and only reads the scene
        totals = list(ex.map(lambda f: o.extract_mesh(bfa.mc_params(R.VS, thresh_factor=f))[1], R.THRESH_FACTORS))
    assert totals[0] > 100000
    assert all(a > b for a, b in zip(totals, totals[1:])), totals
    assert totals[-2] > 0 and totals[-1] == 0, totals


@pytest.mark.parametrize("depth,on", [(1.0, False), (1.005, True)])
def test_wall_vertices_on_and_off_the_corner_lattice(depth, on):
    p, cam, d, c = wall_scene(R.VS, depth=depth)
    o = OracleScene(p)
    I = np.eye(4, dtype=np.float32)
    o.integrate(I, d, c, cam)
    o.integrate(I, d, c, cam)
    tris, total = o.extract_mesh(bfa.mc_params(R.VS))
    assert total == len(tris) > 10000
    lat = R.on_corner_lattice(tris[..., 2])
    assert lat.all() if on else not lat.any()     # all from vertexInterp's no-interpolation returns, or none


def test_first_heap_blocks_emit_unequal_counts():
    o = world(0.0)
    h = o.export()[0]
    occ = h[h["ptr"] != bfa.abi.FREE_ENTRY]
    first = occ[np.argsort(occ["ptr"])][:8]
    counts, padded = [], []
    for e in first:
        blk = (e["x"], e["y"], e["z"])
        counts.append(o.extract_mesh(bfa.mc_params(R.VS, box=R.block_box(blk)))[1])
        padded.append(o.extract_mesh(bfa.mc_params(R.VS, box=R.block_box(blk, 0.25)))[1])
    assert counts == padded                       # the inclusive box edge keeps exactly the block's own voxels
    assert len(set(counts)) > 1 and max(counts) > 0, counts
    assert sum(counts) >= 8                        # room for caps on, before and after a block boundary
