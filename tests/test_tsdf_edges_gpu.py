"""The HIP voxel-hash TSDF against the CPU oracle at its fast-path, sign, depth and tile edges: the crafted cases of
tsdf_edge_inputs.py (test_tsdf_edges.py proves with the oracle alone that each sits on its edge), driven through
tsdf_compare.Pair. The criterion is test_tsdf_gpu.py's: the block set, bits of sdf, weight and colour, the heap
free count, no error flag, and the device counters the oracle keeps too. No tolerance.

Every case runs op by op (compared after every op and after the garbage collection) and again as one apply_ops
batch. The branches the cases pin (csrc/tsdf.hip):
  a  voxel_pixel2b / proj_needs_exact: projections exactly on, and 2^-13 / 2^-14 px beside, the pixel boundary
  b  block_may_update_halves_q's rectangle and f2i toward zero at the left / top image edge; b_rect_hi: a block
     whose corner the cull computes below -1.5 px of a voxel the oracle puts in column 0 (RECT_HI's 2^-6 px)
  c  the band cull's fine, coarse, very-close and camera-plane paths; a tile without integrable depth
  d  ray_walk_from_ends: rayDir == 0, bp - rayMin == 0, rays inside one block
  e  world_to_block_rcp / vvox_to_block / owned around the origin, unsharded and as either of two shards
  f  -inf, +inf, 0.0, -0.0, negative, denormal, NaN, the maximum distance and its predecessor, the sensor range
  g  67x45, 13x9, 8x8, 1x1 and 17x16 images: partial 8- and 16-pixel tiles in depth_tile_wave, pack_dc, alloc_collect
  h  integrationWeightMax 1, 2, 3: batch_integrate's cap as an integer min of float bits, emptied voxels
  i  fx = 2^21 (rFx == 0) and voxel size 2^21 (rVoxelSize == 0): the IEEE forms of ray_walk_ends. The third
     IEEE condition, |w| > 2^100, is not run: normalize3 overflows there in the reference too.
  j  k_apply_ops's work distribution: applyXcdRun 1, 64, 32768 x applyRounds 1, 64
  k  one batch with a colour-less op between two coloured ones on the same frame"""
import numpy as np
import pytest

import bundlefusion_amd as bfa
import tsdf_edge_inputs as E
from test_tsdf_gpu import ORACLE_STATS
from tsdf_compare import Pair

pytestmark = pytest.mark.gpu

# one scan serves a whole batch: `scanned` and `visible` count it once where the oracle's op-by-op run counts every
# op's; the batch's frustum list is the last op's, which numVisible / numOccupied compare instead
PER_SCAN = ("scanned", "visible")


def check_counters(pair, batch):
    assert pair.gpu.errorFlags() == 0
    assert pair.gpu.getHeapFreeCount() == pair.ora.getHeapFreeCount()
    assert pair.gpu.numVisible() == pair.ora.numOccupied()
    gs, os_ = pair.gpu.stats(), pair.ora.stats()
    for f in ORACLE_STATS:
        if batch and f in PER_SCAN:
            continue
        assert gs[f] == os_[f], f"stats field {f}: gpu {gs[f]} != oracle {os_[f]}"


def run_case(case, batch, **scene_opts):
    pair = Pair(case.params, case.cam, **dict(case.scene_opts, **scene_opts))
    dev = [(bfa.DeviceArray.from_host(d), bfa.DeviceArray.from_host(c)) for d, c in case.frames]
    if batch:
        for op in case.ops:
            d, c = case.frames[op.frame]
            pair.ora.integrate(op.T, d, c if op.colour else None, case.cam, deintegrate=op.deint)
        pair.gpu.apply_ops([(op.T, dev[op.frame][0], dev[op.frame][1] if op.colour else None, op.deint) for op in case.ops],
                           case.cam)
        pair.compare()
    else:
        for op in case.ops:
            d, c = case.frames[op.frame]
            dd, cc = dev[op.frame]
            (pair.gpu.deIntegrate if op.deint else pair.gpu.integrate)(op.T, dd, cc if op.colour else None, case.cam)
            pair.ora.integrate(op.T, d, c if op.colour else None, case.cam, deintegrate=op.deint)
            pair.compare()
    check_counters(pair, batch)
    pair.gc()
    n = pair.compare()
    check_counters(pair, batch)
    return pair, n


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_edge_case(name, batch):
    run_case(E.make(name), batch)


def test_scaled_scene_has_the_unscaled_block_set():
    """i. Every length times 2^28 is an exact scaling, so the block set (which the oracle keeps: test_tsdf_edges.py)
    is the unscaled case's on the device too, block for block, with equal weights and sdf scaled by 2^28. A
    fixed metric constant of the kernels (the band cull's 1 mm slack, its 1e-3 camera-plane test) that made the
    scaled run differ would show here or in test_edge_case."""
    from oracle_lib import blocks_of
    small, _ = run_case(E.make("a_pixel_boundary"), True)
    big, _ = run_case(E.make("i_voxel_size_2p21"), True)
    hs, _, _, vs = small.gpu.export()
    hb, _, _, vb = big.gpu.export()
    bs, bb = blocks_of(hs), blocks_of(hb)
    assert set(bs) == set(bb) and len(bs) >= 100
    keys = sorted(bs)
    i_s = (np.array([bs[k] for k in keys])[:, None] + np.arange(512)[None, :]).ravel()
    i_b = (np.array([bb[k] for k in keys])[:, None] + np.arange(512)[None, :]).ravel()
    assert (vs["weight"][i_s] == vb["weight"][i_b]).all() and (vs["color"][i_s] == vb["color"][i_b]).all()
    assert (vs["sdf"][i_s] * np.float32(E.SCALE_BIG) == vb["sdf"][i_b]).all()


@pytest.mark.parametrize("rounds", E.WORK_ROUNDS)
@pytest.mark.parametrize("xcd_run", E.WORK_XCD_RUNS)
@pytest.mark.parametrize("scene", E.WORK_SCENES)
def test_work_distribution(scene, xcd_run, rounds):
    """j. One 10-op batch under every work-list run length and grid: bit-identical to the oracle with equal
    voxelsUpdated (check_counters), whatever wave a block lands on."""
    case = E.case_work_distribution(scene)
    pair, n = run_case(case, True, apply_xcd_run=xcd_run, apply_rounds=rounds)
    assert pair.gpu.stats()["voxelsUpdated"] == pair.ora.stats()["voxelsUpdated"]
    assert pair.gpu.stats()["batchOps"] == len(case.ops)
