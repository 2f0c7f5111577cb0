"""The inputs of test_tsdf_edges_gpu.py (tsdf_edge_inputs.py) sit on the edges they are named for: checked here
with the CPU oracle (oracle/tsdf.cpp), alloc_box's restatement of the ray ends and float64 NumPy alone.

A parity test proves nothing about a branch its input never takes. Every assertion below is a coverage condition
on an input, not a tolerance on a kernel: a change to a generator that empties one of the GPU tests fails here
first. The counts are minimum conditions, not measurements."""
import functools

import numpy as np
import pytest

import tsdf_edge_inputs as E
from alloc_box import ray_ends, tile_boxes
from oracle_lib import OracleScene, blocks_of, matrix_inverse

F = np.float32


def run_oracle(case, n_ops=None, gc=False, frames=None, shard="case"):
    """The oracle scene after the case's first n_ops ops (all by default)."""
    opts = case.scene_opts
    sh = None
    if shard == "case" and opts.get("shard_count", 1) > 1:
        sh = (opts["shard_count"], opts["shard_index"], opts["shard_chunk"])
    s = OracleScene(case.params, shard=sh)
    frames = case.frames if frames is None else frames
    for op in case.ops[:n_ops]:
        d, c = frames[op.frame]
        s.integrate(op.T, d, c if op.colour else None, case.cam, deintegrate=op.deint)
    if gc:
        s.garbageCollect()
    return s


@functools.lru_cache(maxsize=None)
def first_op(name):
    """(case, blocks {(x, y, z): ptr}, voxels) after the case's first op."""
    case = E.make(name)
    h, _, _, vox = run_oracle(case, 1).export()
    return case, blocks_of(h), vox


def voxel_facts(case, blocks, vox, op=0):
    """Per voxel of the oracle's blocks: float64 projection, the pixel rule's decision, the oracle's weight."""
    keys = sorted(blocks)
    v = E.block_voxel_coords(keys)
    o = case.ops[op]
    pc, sx, sy = E.project64(case, o.T, v)
    rule = E.pixel_rule(case, case.frames[o.frame][0], pc, sx, sy)
    ptr = np.array([blocks[k] for k in keys])
    w = vox["weight"][ptr[:, None] + np.arange(512)[None, :]]
    return dict(keys=keys, v=v, pc=pc, sx=sx, sy=sy, weight=w, **rule)


def test_generators_repeat():
    for name in E.CASES:
        a, b = E.make(name), E.make(name)
        assert len(a.ops) == len(b.ops) and all((x.T == y.T).all() for x, y in zip(a.ops, b.ops))
        assert all(np.array_equal(x[0], y[0], equal_nan=True) and (x[1] == y[1]).all() for x, y in zip(a.frames, b.frames))
        W, H = a.cam.imageWidth, a.cam.imageHeight
        assert W <= 72 and H <= 72 and a.params.hashNumBuckets <= 1 << 14


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_scene_sizes(name):
    """A few hundred blocks at the most, far below the pool and the table; nothing overflows in the oracle."""
    case = E.make(name)
    s = run_oracle(case)
    n = len(blocks_of(s.export()[0]))
    assert n <= 700 and n <= case.params.numSDFBlocks // 2
    assert s.stats()["allocOverflow"] == 0


@pytest.mark.parametrize("name", ["a_pixel_boundary", "d_dda", f"i_focal_{int(E.FOCAL_BIG)}", "i_voxel_size_2p21"])
def test_lattice_rig_is_exact_in_float32(name):
    """The lattice cases' values are exact in float32: the oracle's inverse pose is the exact inverse, every voxel
    centre's camera position and fx x / fy y equal the float64 ones, and wherever the float64 screen coordinate is a
    multiple of 2^-13 px the float32 one (quotient, + m) equals it."""
    case, blocks, _ = first_op(name)
    v = E.block_voxel_coords(sorted(blocks))
    for op in case.ops:
        Ti = matrix_inverse(op.T)
        assert (Ti.astype(np.float64) == np.linalg.inv(op.T.astype(np.float64))).all()
        pc64, sx64, sy64 = E.project64(case, op.T, v)
        pc32, sx32, sy32 = E.project32(case, Ti, v)
        assert (pc32.astype(np.float64) == pc64).all()
        for s64, s32 in ((sx64, sx32), (sy64, sy32)):
            grid = np.isfinite(s64) & (np.abs(s64) < 1024) & (s64 * 8192 == np.round(s64 * 8192))
            assert grid.sum() >= 64
            assert (s32[grid].astype(np.float64) == s64[grid]).all()
            # everywhere else the float32 coordinate is the float64 one to rounding
            ok = np.isfinite(s64)
            assert np.abs(s32[ok] - s64[ok]).max() <= 2.0 ** -23 * (np.abs(s64[ok]).max() + float(case.cam.mx) + 64)


def test_a_voxels_project_onto_the_pixel_boundary():
    """a. At least 64 in-band voxel centres of the unshifted pose have x + 0.5 or y + 0.5 exactly integral; at
    least 64 of them at a depth that is no power of two (the reciprocal of z is then inexact: the fast quotient
    can land on the other side of the integer, so the IEEE re-division decides the pixel)."""
    case, blocks, vox = first_op("a_pixel_boundary")
    assert 100 <= len(blocks) <= 700
    f = voxel_facts(case, blocks, vox)
    tx, ty = f["sx"] + 0.5, f["sy"] + 0.5
    on_x, on_y = f["band"] & (tx == np.round(tx)), f["band"] & (ty == np.round(ty))
    assert (on_x | on_y).sum() >= 64
    z = f["pc"][..., 2]
    pow2 = np.log2(z) == np.round(np.log2(z))
    assert ((on_x | on_y) & ~pow2).sum() >= 64
    # the oracle updated exactly the voxels the float64 rule puts in the band (weight 1 after one op)
    assert ((f["weight"] == 1.0) == f["band"]).all()
    # the shifted poses move every screen coordinate by 2^-13 px at z = 0.5 and 2^-14 px at z = 1.0: the exactness
    # bound of voxel_pixel2b, eps_c = (3 (max(W, H) + 2) + max(mx, my) + 3) 2^-21 = 1.38 2^-14, lies between, so
    # the boundary voxels of the far plane re-divide and those of the near plane must be right without
    eps_c = (3 * (48 + 2) + 23.5 + 3) * 2.0 ** -21
    assert 2.0 ** -14 < eps_c < 2.0 ** -13
    for k in (1, 2):
        _, sx, _ = E.project64(case, case.ops[k].T, f["v"])
        for depth, shift in ((0.5, 2.0 ** -13), (1.0, 2.0 ** -14)):
            at = on_x & (z == depth)
            assert at.sum() >= 64 and (np.abs(sx[at] - f["sx"][at]) == shift).all()


def test_b_voxels_on_both_sides_of_every_image_edge():
    """b. Oracle-updated voxels in (-1.5, -0.5] (column / row 0 by truncation toward zero), and voxels in
    [W - 0.5, W + 0.5) / [H - 0.5, H + 0.5) that must stay untouched; 16 each at the least."""
    case, blocks, vox = first_op("b_image_border")
    W, H = case.cam.imageWidth, case.cam.imageHeight
    f = voxel_facts(case, blocks, vox)
    d = case.frames[0][0]
    assert np.isfinite(d).all()  # the surface runs off all four edges: no invalid pixel
    # 1e-4 px away from the interval ends: the float32 coordinate decides there, not the float64 one
    m = 1e-4
    left = (f["sx"] > -1.5 + m) & (f["sx"] <= -0.5) & (f["weight"] != 0)
    top = (f["sy"] > -1.5 + m) & (f["sy"] <= -0.5) & (f["weight"] != 0)
    assert left.sum() >= 16 and top.sum() >= 16
    assert (f["ux"][left] == 0).all() and (f["uy"][top] == 0).all()
    right = (f["sx"] >= W - 0.5 + m) & (f["sx"] < W + 0.5) & (f["sy"] > 0) & (f["sy"] < H - 1)
    bottom = (f["sy"] >= H - 0.5 + m) & (f["sy"] < H + 0.5) & (f["sx"] > 0) & (f["sx"] < W - 1)
    assert right.sum() >= 16 and bottom.sum() >= 16
    assert (f["weight"][right] == 0).all() and (f["weight"][bottom] == 0).all()
    # some of the column-0 / row-0 voxels are their block's extreme corner: the half's rectangle ends there
    assert (f["weight"] != 0).sum() > 1000


def test_b_rect_hi_corner_is_below_the_voxel_it_bounds():
    """b. The placed block: allocated by the first op; the second op's oracle projects its extreme corner voxel
    into (-1.5, -0.5] in float32 and updates it, while the band cull's own float32 arithmetic (restated:
    E.cull_corners) puts every corner below -1.5: floor(xhi + 1.5) < 0 would drop the block, RECT_HI keeps it."""
    case = E.make("b_rect_hi")
    blk, v = case.facts["block"], np.array(case.facts["voxel"])
    i = v - np.array(blk) * 8
    idx = int(i[0] + 8 * i[1] + 64 * i[2])
    assert set(i.tolist()) <= {0, 7}
    weights = []
    for n in (1, 2):
        h, _, _, vox = run_oracle(case, n).export()
        b = blocks_of(h)
        assert blk in b and len(b) <= 300
        weights.append(float(vox["weight"][b[blk] + idx]))
    assert weights == [1.0, 2.0]
    Ti = matrix_inverse(case.ops[1].T)
    _, sx32, _ = E.project32(case, Ti, v)
    assert sx32.dtype == F and F(-1.5) < sx32 <= F(-0.5) and int(F(sx32 + F(0.5))) == 0
    xhi = max(c[0] for c in E.cull_corners(case, Ti, blk))
    assert xhi.dtype == F and np.floor(xhi + F(1.5)) < 0 <= np.floor(xhi + F(1.5 + E.RECT_HI_SLACK))
    assert float(sx32) - float(xhi) > 4e-6  # several times the reciprocal's ulp at these 36 px
    # the block's centre passes the second op's frustum test, so the op's list holds the block
    _, cx, _ = E.project64(case, case.ops[1].T, np.array(blk) * 8 + 3.5)
    assert (2 * cx - 71) / 71 * 0.95 > -1


def test_c_band_cull_takes_every_path():
    """c. From the oracle's blocks: footprints within 3x3 fine tiles, within 3x3 coarse tiles, wider still, and
    blocks with a corner at z <= 1e-3; an 8-pixel tile without integrable depth beside one with."""
    case, blocks, vox = first_op("c_band_cull")
    assert float(case.cam.sensorDepthWorldMin) == float(F(0.01))
    kinds = E.cull_footprints(case, case.ops[0].T, sorted(blocks))
    count = {k: int((kinds == k).sum()) for k in ("fine", "coarse", "wide", "plane", "off")}
    assert count["fine"] >= 1 and count["coarse"] >= 1 and count["wide"] >= 1 and count["plane"] >= 1, count
    d = case.frames[0][0]
    assert {float(v) for v in np.unique(d[np.isfinite(d)])} == {float(F(v)) for v in (0.05, 0.12, 0.3, 1.5)}
    assert np.all(d[:, 0:8] == -np.inf) and np.all(np.isfinite(d[:, 8:16]))
    # blocks of every path hold updated voxels (the kept paths must not lose them)
    f = voxel_facts(case, blocks, vox)
    upd = (f["weight"] != 0).any(axis=1)
    for k in ("fine", "coarse", "wide", "plane"):
        assert (upd & (kinds == k)).any(), k
    # voxels behind the camera plane exist in the allocated blocks
    assert (f["pc"][..., 2] <= 0).sum() >= 16


def test_d_dda_degenerate_rays():
    """d. From alloc_box.ray_ends: rays with rayDir.x == 0, with .y == 0 and with both, rays that start on a block
    face (bp - rayMin == 0 on z) and rays whose first and last block coincide."""
    case = E.make("d_dda")
    p, cam = case.params, case.cam
    T, d = case.ops[1].T, case.frames[0][0]
    assert case.ops[0].frame == 1 and case.ops[1].frame == 0
    active, b0, b1, r0, r1 = ray_ends(T, d, cam, p, want_points=True)
    assert active.all()
    dirv = (r1 - r0).astype(F)  # normalize3 scales by a finite positive factor: zero components stay zero
    x0, y0 = dirv[..., 0] == 0, dirv[..., 1] == 0
    assert (x0 & ~y0).sum() >= 1 and (y0 & ~x0).sum() >= 1 and (x0 & y0).sum() == 1
    assert x0[:, 16].all() and y0[12, :].all()
    # bp = block_to_world(id + clamp(step, 0, 1)) - voxelSize / 2, in float32
    vs = F(p.virtualVoxelSize)
    step = np.sign(dirv)
    bp = ((b0 + np.clip(step, 0, 1)).astype(F) * F(8) * vs - F(0.5) * vs).astype(F)
    on_face = (bp - r0).astype(F) == 0
    assert on_face[..., 2][:, :17].all() and not on_face[..., 2][:, 17:].any()
    assert (r0[:, :17, 2] == F(-64.5 / 128)).all() and (b0[:, :17, 2] == -9).all()
    same = (b0 == b1).all(axis=-1)
    assert same.sum() >= 1 and same[:, 17:].any() and not same[:, :17].any()
    # coordinates of both signs on x and y
    assert (b0[..., 0] < 0).any() and (b0[..., 0] >= 0).any() and (b0[..., 1] < 0).any() and (b0[..., 1] >= 0).any()
    # the lone rays: each crosses from block -9 to -8 in z, and no other ray of its frame reaches either block
    la, l0, l1, q0, q1 = ray_ends(T, case.frames[1][0], cam, p, want_points=True)
    assert la.sum() == len(E.LONE_RAYS) == 3
    seen = set()
    for (x, y), zero in zip(E.LONE_RAYS, ((True, True), (True, False), (False, True))):
        assert la[y, x] and (l0[y, x, 2], l1[y, x, 2]) == (-9, -8) and (l0[y, x, :2] == l1[y, x, :2]).all()
        lone_dir = q1[y, x] - q0[y, x]
        assert (lone_dir[0] == 0, lone_dir[1] == 0) == zero
        assert tuple(l0[y, x, :2]) not in seen
        seen.add(tuple(l0[y, x, :2]))
    assert len(first_op("d_dda")[1]) == 6  # the first op is the lone rays': two blocks each
    assert len(blocks_of(run_oracle(case, 2).export()[0])) >= 16


def test_e_blocks_straddle_the_origin():
    """e. Blocks -1 and 0 on every axis, (-1,-1,-1) and (0,0,0); a ray end with a coordinate exactly 0.0; the
    two shards partition the unsharded block set and both own blocks next to the origin."""
    case, blocks, _ = first_op("e_origin")
    keys = np.array(sorted(blocks))
    for ax in range(3):
        assert {-1, 0} <= set(keys[:, ax].tolist())
    assert (-1, -1, -1) in blocks and (0, 0, 0) in blocks
    active, b0, b1, r0, r1 = ray_ends(case.ops[0].T, case.frames[0][0], case.cam, case.params, want_points=True)
    assert active.all() and ((r0 == 0.0) | (r1 == 0.0)).any()
    assert (r0[:, 24, 0] == 0.0).all() and (r1[:, 24, 0] == 0.0).all()
    shards = [first_op(f"e_origin_shard{i}")[1] for i in range(2)]
    assert not set(shards[0]) & set(shards[1]) and set(shards[0]) | set(shards[1]) == set(blocks)
    near = [{k for k in s if max(abs(v) for v in k) <= 1} for s in shards]
    assert len(near[0]) >= 4 and len(near[1]) >= 4
    # the chunk rounding's tie: block 1's corner over the chunk size is 0.5 exactly
    assert F(8) * F(case.params.virtualVoxelSize) / F(E.ORIGIN_CHUNK) == F(0.5)


@pytest.mark.parametrize("name", ["f_depth_validity", "f_depth_validity_no_colour"])
def test_f_depth_groups(name):
    """f. Every group is in the image; each valid group allocates blocks on its own and no other group does; with
    colour, in-band voxels project onto the 0.0, -0.0 and denormal columns and stay untouched there only if the
    depth says so (the oracle's rule: d == -inf or d >= max is skipped, 0.0 is a depth like any other)."""
    case = E.make(name)
    d = case.frames[0][0]
    for g, (gname, v, _) in enumerate(E.DEPTH_GROUPS):
        col = d[:, 4 * g:4 * g + 4]
        assert np.array_equal(col, np.full_like(col, F(v)), equal_nan=True), gname
        assert np.signbit(col).all() == bool(np.signbit(F(v)))
    assert np.isnan(d).sum() == 4 * d.shape[0] and (d == np.inf).sum() == 4 * d.shape[0]
    sub = F(1e-40)
    assert 0 < sub < np.finfo(F).tiny
    assert F(E.DEPTH_MAX) == F(case.params.maxIntegrationDistance)
    assert F(case.cam.sensorDepthWorldMax) < F(0.95) < F(E.DEPTH_MAX) and F(case.cam.sensorDepthWorldMin) == F(E.SENSOR_MIN)
    for gname, _, allocates in E.DEPTH_GROUPS:
        s = run_oracle(case, 1, frames=[(E.depth_group_image(only=gname), case.frames[0][1])])
        n = len(blocks_of(s.export()[0]))
        assert (n > 0) == allocates, (gname, n)
    s = run_oracle(case, 1)
    h, _, _, vox = s.export()
    blocks = blocks_of(h)
    f = voxel_facts(case, blocks, vox)
    if name.endswith("no_colour"):
        assert (f["weight"] == 0).all() and len(blocks) > 20
        return
    assert ((f["weight"] != 0) == f["band"]).mean() > 0.999  # float64 rule = oracle away from ties
    group = np.where(f["on"], f["ux"] // 4, -1).astype(int)
    names = [g[0] for g in E.DEPTH_GROUPS]
    for gname in ("zero", "minus_zero", "denormal"):
        g = names.index(gname)
        assert ((group == g) & (f["weight"] != 0)).sum() >= 4, gname  # |0 - z| < truncation: updated
    for gname in ("minus_inf", "plus_inf", "nan", "max_distance", "negative"):
        g = names.index(gname)
        assert not ((group == g) & (f["weight"] != 0)).any(), gname  # never updated, whatever lands there
    for gname in ("nan", "negative"):  # voxels nearer than the truncation land there
        assert ((group == names.index(gname)) & (np.abs(f["pc"][..., 2]) < 0.06)).sum() >= 4, gname


@pytest.mark.parametrize("size", sorted(E.OFF_GRID))
def test_g_tile_counts(size):
    """g. The stated counts of 8-pixel and 16-pixel tiles, partial on both axes (but for 8x8: one full fine tile
    inside a partial 16-pixel one), every 16-pixel tile with active rays."""
    W, H = size
    case = E.make(f"g_off_grid_{W}x{H}")
    fine, coarse = case.facts["fine"], case.facts["coarse"]
    assert fine == (-(-W // E.DEPTH_TILE), -(-H // E.DEPTH_TILE)) and coarse == (-(-W // E.ALLOC_TILE), -(-H // E.ALLOC_TILE))
    assert {(67, 45): (54, 15), (13, 9): (4, 1), (8, 8): (1, 1), (1, 1): (1, 1), (17, 16): (6, 2)}[size] == \
        (fine[0] * fine[1], coarse[0] * coarse[1])
    assert W % 16 != 0 or H % 16 != 0
    if size != (8, 8):
        assert W % 8 != 0 and (H % 8 != 0 or size == (17, 16))
    boxes = tile_boxes(*ray_ends(case.ops[0].T, case.frames[0][0], case.cam, case.params))
    assert len(boxes) == coarse[0] * coarse[1]
    n = len(first_op(case.name)[1])
    if size == (1, 1):
        assert n == 0  # width - 1 = 0 in the frustum test: see case_off_grid
    else:
        assert n >= 3


@pytest.mark.parametrize("cap", [1, 2, 3])
def test_h_weights_reach_the_cap_and_voxels_empty(cap):
    case = E.make(f"h_weight_cap_{cap}")
    assert case.params.integrationWeightMax == cap
    assert [o.deint for o in case.ops] == [False] * 5 + [True] * 3 + [False]
    h, _, _, vox = run_oracle(case, 5).export()
    ptr = np.array(sorted(blocks_of(h).values()))
    idx = (ptr[:, None] + np.arange(512)[None, :]).ravel()
    w5 = vox["weight"][idx]
    assert w5.max() == cap and (w5 == cap).sum() >= 64 and set(np.unique(w5).tolist()) == {0.0, float(cap)}
    v8 = run_oracle(case, 8).export()[3][idx]
    emptied = (w5 == cap) & (v8["weight"] == 0)
    assert emptied.sum() >= 64
    assert (v8["sdf"][emptied] == 0).all() and (v8["color"][emptied] == 0).all()
    v9 = run_oracle(case, 9).export()[3][idx]
    assert (v9["weight"][emptied] == 1).all()


def test_i_reciprocals_are_out_of_range():
    """i. recip_or_zero (csrc/tsdf.hip) admits [2^-20, 2^20]: both focal lengths and the scaled voxel size lie
    beyond; the scaled case's block set is the unscaled case's block for block, its weights equal and its sdf
    the unscaled ones times 2^28."""
    for f in (E.FOCAL_BIG, 3.0 * 2.0 ** 20):
        case, blocks, vox = first_op(f"i_focal_{int(f)}")
        assert float(case.cam.fx) == f == float(case.cam.fy) and f > 2.0 ** 20
        assert (case.cam.imageWidth, case.cam.imageHeight) == (24, 24)
        assert 2.0 ** -20 <= float(case.params.virtualVoxelSize) <= 2.0 ** 20
        assert 12 <= len(blocks) and (vox["weight"] != 0).sum() >= 1000
    big, small = E.make("i_voxel_size_2p21"), E.make("a_pixel_boundary")
    assert float(big.params.virtualVoxelSize) == 2.0 ** 21 > 2.0 ** 20
    assert float(big.cam.fx) == E.LAT_F
    for k in range(1, len(big.ops) + 1):
        hb, _, _, vb = run_oracle(big, k).export()
        hs, _, _, vs = run_oracle(small, k).export()
        bb, bs = blocks_of(hb), blocks_of(hs)
        assert set(bb) == set(bs) and len(bb) >= 100
        keys = sorted(bb)
        ib = (np.array([bb[q] for q in keys])[:, None] + np.arange(512)[None, :]).ravel()
        is_ = (np.array([bs[q] for q in keys])[:, None] + np.arange(512)[None, :]).ravel()
        assert (vb["weight"][ib] == vs["weight"][is_]).all() and (vb["color"][ib] == vs["color"][is_]).all()
        assert (vb["sdf"][ib] == vs["sdf"][is_] * F(E.SCALE_BIG)).all()


def test_j_work_lists():
    """j. 10 ops each; a few hundred blocks, none, and fewer than 8."""
    n = {}
    for scene in E.WORK_SCENES:
        case = E.case_work_distribution(scene)
        assert len(case.ops) == 10 and sum(o.deint for o in case.ops) == 3
        s = run_oracle(case)
        n[scene] = len(blocks_of(s.export()[0]))
        assert s.stats()["voxelsUpdated"] > 0 or scene == "1x1"
    assert n["67x45"] >= 100 and n["1x1"] == 0 and 1 <= n["one_ray"] < 8, n
    assert E.WORK_XCD_RUNS == (1, 64, 32768) and E.WORK_ROUNDS == (1, 64)


def test_k_mixed_colour_batch():
    case = E.make("k_mixed_colour")
    assert [o.colour for o in case.ops] == [True, False, True] and {o.frame for o in case.ops} == {0}
    # the colour-less op allocates blocks of its own and updates nothing
    n1 = len(blocks_of(run_oracle(case, 1).export()[0]))
    s2 = run_oracle(case, 2)
    assert len(blocks_of(s2.export()[0])) > n1
    assert s2.stats()["voxelsUpdated"] == run_oracle(case, 1).stats()["voxelsUpdated"]
