"""Inputs of the voxel-hash TSDF's edge tests (test_tsdf_edges.py, test_tsdf_edges_gpu.py): crafted frames that
sit on the branches csrc/tsdf.hip keeps its bit-exactness through, instead of rendered frames of the synthetic
room that reach them by chance. NumPy only (case_rect_hi also takes the oracle's float32 matrix inverse and
alloc_box's ray ends for its search): the same arrays on every machine.

A case is a Case record: camera, hash params, frames (depth, colour), a list of ops (pose, frame, with colour or
without, direction), scene options and the edge it is meant to hit. test_tsdf_edges.py checks with the oracle and
the float64 restatements below that each case really sits on its edge.

The lattice rig: voxel size 2^-7 m, fx = fy = 64, identity rotation, depths and translations dyadic. A voxel
centre (i, j, k) 2^-7 then has camera coordinates that are exact in float32 (|i| < 2^9 voxels, translations down
to 2^-20 m: at most 21 significant bits), fx x is exact (a power of two), and wherever fx x / z is a multiple of
2^-13 px the IEEE quotient, the sum with mx (k + 0.5 or integral) and the + 0.5 of the pixel rule are exact too:
a voxel can be placed exactly on the pixel rule's decision boundary. test_tsdf_edges.py redoes these projections
in float64 and compares."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import bundlefusion_amd as bfa

F = np.float32
LAT_VS = 2.0 ** -7
LAT_F = 64.0
SCALE_BIG = 2.0 ** 28       # case i: voxel size 2^21 m, beyond the reciprocal's range [2^-20, 2^20]
FOCAL_BIG = 2.0 ** 21       # case i: focal length beyond that range
DEPTH_TILE, DEPTH_TILE2, ALLOC_TILE = 8, 16, 16   # csrc/tsdf.hip


@dataclass
class Op:
    T: np.ndarray           # camera -> world, float32 [4, 4]
    frame: int = 0
    colour: bool = True     # False: the op passes no colour image (allocates, updates nothing)
    deint: bool = False


@dataclass
class Case:
    name: str
    edge: str
    cam: object
    params: object
    frames: list            # [(depth float32 [H, W], colour uint8 [H, W, 4])]
    ops: list
    scene_opts: dict = field(default_factory=dict)
    facts: dict = field(default_factory=dict)


# ---- building blocks ---------------------------------------------------------------------------------------
def pose(R=None, t=(0.0, 0.0, 0.0)) -> np.ndarray:
    T = np.eye(4)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = t
    return T.astype(F)


def rotation(axis, deg: float) -> np.ndarray:
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(deg)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def shifted(T: np.ndarray, dt) -> np.ndarray:
    """T moved by dt along the camera's own axes."""
    out = T.astype(np.float64)
    out[:3, 3] += out[:3, :3] @ np.asarray(dt, np.float64)
    return out.astype(F)


def colour_image(W: int, H: int, seed: int) -> np.ndarray:
    c = np.random.default_rng(seed).integers(0, 256, size=(H, W, 4), dtype=np.uint8)
    c[..., 3] = 255
    return c


def tilted_plane(W: int, H: int, d0: float, dx: float, dy: float) -> np.ndarray:
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    return (d0 + dx * x + dy * y).astype(F)


def small_hash(**kw):
    return bfa.hash_params(num_buckets=kw.pop("num_buckets", 1 << 13), num_blocks=kw.pop("num_blocks", 2048), **kw)


GENERAL_POSE = pose(rotation((1.0, 2.0, 0.5), 20.0), (0.3, -0.2, 0.1))


def three_ops(T, dt=(0.004, -0.003, 0.002)):
    """integrate, integrate from a moved pose, de-integrate the first"""
    return [Op(T), Op(shifted(T, dt)), Op(T, deint=True)]


# ---- the cases ---------------------------------------------------------------------------------------------
def case_pixel_boundary(scale: float = 1.0, name="a_pixel_boundary") -> Case:
    """a. Lattice rig, mx = 23.5, my = 19.5, fronto-parallel planes at z = 0.5 (left half) and z = 1.0 (right
    half): at z = 0.5 a voxel's screen x is i - 128 tx + mx, at the other levels of the band 64 i / (64 + n) + ...,
    integral + 0.5 for every i the level's denominator divides. Poses: this one and +-2^-20 m along camera
    x and y (2^-13 px at z = 0.5, 2^-14 px at z = 1: either side of voxel_pixel2b's exactness bound). With
    scale = 2^28 every length is scaled exactly (case i: no reciprocal of the voxel size)."""
    s = scale
    W, H = 48, 40
    cam = bfa.depth_camera(W, H, fx=LAT_F, fy=LAT_F, mx=23.5, my=19.5, zmin=0.125 * s, zmax=4.0 * s)
    p = small_hash(voxel_size=LAT_VS * s, truncation=0.0625 * s, trunc_scale=2.0 ** -6, max_integration_distance=3.0 * s)
    d = np.full((H, W), 0.5 * s, F)
    d[:, W // 2:] = 1.0 * s
    t0 = np.array([2.0 ** -3, -2.0 ** -4, 0.0]) * s
    e = 2.0 ** -20 * s
    # two more, +-2^-25 m: 2^-18 / 2^-19 px beside the boundary, the size of the fast quotient's own error (an
    # ulp of a coordinate of 16 to 32 px is 2^-19), still exact in float32 (|x|, |y| < 0.5 m: 24 bits)
    e2 = 2.0 ** -25 * s
    poses = [pose(t=t0), pose(t=t0 + [e, e, 0.0]), pose(t=t0 - [e, e, 0.0]), pose(t=t0 + [e2, e2, 0.0]), pose(t=t0 - [e2, e2, 0.0])]
    ops = [Op(T) for T in poses] + [Op(poses[0], deint=True), Op(poses[3], deint=True)]
    return Case(name, "voxel_pixel2b / proj_needs_exact: projections exactly on the pixel rule's boundary",
                cam, p, [(d, colour_image(W, H, 1))], ops, facts=dict(scale=s))


def case_image_border() -> Case:
    """b. A tilted plane that runs off all four image edges under a general pose: blocks hang over every edge,
    so voxels project into (-1.5, -0.5] (column / row 0 by truncation toward zero) and into [W - 0.5, W + 0.5)
    (no column)."""
    W, H = 64, 48
    cam = bfa.depth_camera(W, H, fx=60.0, fy=60.0)
    p = small_hash(voxel_size=0.01)
    d = tilted_plane(W, H, 0.55, 0.003, 0.002)
    return Case("b_image_border", "RECT_HI growth of the band cull's rectangle, f2i toward zero at the left / top edge",
                cam, p, [(d, colour_image(W, H, 2))], three_ops(GENERAL_POSE))


RECT_HI_SLACK = 2.0 ** -6  # csrc/tsdf.hip RECT_HI = 1.5 + 2^-6


def _fma32(a, b, c):
    return F(np.float64(a) * np.float64(b) + np.float64(c))


def cull_corners(case: Case, Tinv32, block) -> list:
    """block_may_update_halves_q's eight corner projections in its own float32 operation order (cull_op_consts'
    folded rows, the fma chain of the corner voxel, the column sums, fma(px, rz, mx)), with the hardware reciprocal
    (1 ulp) taken as the correctly rounded one: per corner (screen x, screen y, px * rz before the fma rounds)."""
    cam, vs, t = case.cam, F(case.params.virtualVoxelSize), np.asarray(Tinv32, F).reshape(16)
    q = np.zeros(21, F)
    for c in range(4):
        q[c], q[4 + c], q[8 + c] = F(cam.fx) * t[c], F(cam.fy) * t[4 + c], t[8 + c]
    ext = vs * F(7)
    for c in range(3):
        for r in range(3):
            q[12 + 3 * c + r] = ext * q[4 * r + c]
    c0 = (np.asarray(block, np.int64) * 8).astype(F) * vs
    p0 = [_fma32(q[4 * r], c0[0], _fma32(q[4 * r + 1], c0[1], _fma32(q[4 * r + 2], c0[2], q[4 * r + 3]))) for r in range(3)]
    out = []
    for k in range(8):
        px, py, pz = p0
        for c in range(3):
            if (k >> c) & 1:
                px, py, pz = F(px + q[12 + 3 * c]), F(py + q[13 + 3 * c]), F(pz + q[14 + 3 * c])
        rz = F(F(1.0) / pz)
        out.append((_fma32(px, rz, F(cam.mx)), _fma32(py, rz, F(cam.my)), float(px) * float(rz)))
    return out


RECT_COLS, RECT_ROWS = 4, (26, 30)   # case_rect_hi: the image's valid region
RECT_SHIFT = 0.072                    # 3 px at 0.6 m and fx = 25


def case_rect_hi() -> Case:
    """b. The left edge of the band cull's rectangle, placed. A block lying wholly left of the image is reached
    by no ray, so an earlier op (the camera 3 px further left) allocates it; the frustum test's 0.95 leaves
    1.87 px beside a 72-pixel image for its centre, hence voxels of 1/24 px (1 mm at 0.6 m, fx = 25). The camera
    stands metres from the origin: the cull's folded rows fx r0 . c0 + fx t and the oracle's xform both cancel
    terms of a few hundred pixels, so their screen x of one voxel differ by ~1e-5 px. Poses are drawn from a
    seeded generator until, for some block, the cull's own arithmetic (cull_corners) puts the extreme corner
    voxel more than 8e-6 px left of where the oracle's puts it; mx (a free parameter, added last on both
    sides) then places that voxel just above x = -1.5 for the oracle (column 0, in band, updated) and below it
    for the cull. With RECT_HI = 1.5 the cull drops the block; its 2^-6 px keep it. facts: block and voxel."""
    from alloc_box import ray_ends
    from oracle_lib import matrix_inverse
    W, H = 72, 56
    p = small_hash(voxel_size=0.001, truncation=0.006, trunc_scale=0.0)
    d = np.full((H, W), -np.inf, F)
    d[RECT_ROWS[0]:RECT_ROWS[1], :RECT_COLS] = 0.6
    for seed in range(200):
        rng = np.random.default_rng(100 + seed)
        T = pose(rotation(rng.normal(size=3), rng.uniform(10.0, 30.0)), rng.uniform(-8.0, 8.0, size=3))
        TA = shifted(T, (-RECT_SHIFT, 0.0, 0.0))
        Ti = matrix_inverse(T)
        cam = bfa.depth_camera(W, H, fx=25.0, fy=25.0)
        case = Case("b_rect_hi", "RECT_HI: a corner the cull computes below -1.5 px of a voxel the oracle puts in column 0",
                    cam, p, [(d, colour_image(W, H, 12))], [Op(TA), Op(T), Op(TA, deint=True)])
        act, b0, b1 = ray_ends(TA, d, cam, p)
        ends = np.concatenate([b0[:, 1:3][act[:, 1:3]], b1[:, 1:3][act[:, 1:3]]])
        for blk in sorted({tuple(int(v) for v in b) for b in ends}):
            cam.mx = (W - 1) / 2.0
            corners = cull_corners(case, Ti, blk)
            k = int(np.argmax([c[0] for c in corners]))
            if not -2.3 <= corners[k][0] <= -0.7:
                continue
            v = np.asarray(blk, np.int64) * 8 + 7 * np.array([(k >> c) & 1 for c in range(3)])
            pc32, _, _ = project32(case, Ti, v)
            q32 = F(pc32[0] * F(cam.fx)) / pc32[2]
            if corners[k][2] - float(q32) > -8e-6:
                continue
            mx = F(F(-1.5) - q32)
            while not F(q32 + mx) > F(-1.5):
                mx = np.nextafter(mx, F(np.inf))
            cam.mx = float(mx)
            if not all(c[2] + float(mx) < -1.5 - 4e-6 for c in cull_corners(case, Ti, blk)):
                continue
            pc, sx, sy = project64(case, T, v)
            rule = pixel_rule(case, d, pc[None], sx[None], sy[None])
            if not (rule["band"][0] and rule["ux"][0] == 0):
                continue
            # the block's centre inside the frustum test's 0.95 margin, by 0.02 px
            _, cx, _ = project64(case, T, np.asarray(blk, np.float64) * 8 + 3.5)
            if not cx > -(W - 1) / 2.0 * (1 / 0.95 - 1) + 0.02:
                continue
            case.facts = dict(block=blk, voxel=tuple(int(x) for x in v), seed=seed)
            return case
    raise AssertionError("no pose puts the cull's corner below the oracle's voxel")


CULL_STRIPES = ((0, 8, -np.inf), (8, 24, 1.5), (24, 40, 0.3), (40, 56, 0.12), (56, 72, 0.05))


def case_band_cull() -> Case:
    """c. Near plane 0.01 m, quarter-resolution focal length, depth stripes at 1.5, 0.3, 0.12 and 0.05 m: an
    8 cm block covers 8, 39, 96 pixels or the whole image, and the nearest blocks reach behind the camera. The
    first 8 columns hold no depth at all (a fine tile without integrable depth beside one with)."""
    W, H = 72, 56
    f = 577.87 / 4
    cam = bfa.depth_camera(W, H, fx=f, fy=f, zmin=0.01, zmax=4.0)
    p = small_hash(voxel_size=0.01, num_blocks=4096)
    d = np.empty((H, W), F)
    for x0, x1, v in CULL_STRIPES:
        d[:, x0:x1] = v
    T = pose(rotation((0.3, 1.0, 0.2), 8.0), (0.036, 0.034, 0.015))
    return Case("c_band_cull", "block_may_update_halves_q: fine, coarse, very-close and camera-plane paths, empty tile",
                cam, p, [(d, colour_image(W, H, 3))], three_ops(T, dt=(0.003, 0.002, -0.002)))


LONE_RAYS = ((16, 12), (16, 4), (28, 12))  # (x, y): rayDir x and y zero, x zero, y zero


def case_dda() -> Case:
    """d. Lattice rig, mx = 16, my = 12 (the centre column / row / pixel look along a camera axis), camera at
    z = -1 looking along +z, truncation 2 voxels, no truncation scale. Left of column 17 the depth is 65.5 / 128:
    rayMin.z = -64.5 voxels, the upper face of block -9, which the rounding (half away from zero) assigns to
    block -9: bp.z - rayMin.z == 0. Right of it the depth is 67 / 128: the ray runs from -63 to -59 voxels,
    inside block -8."""
    W, H = 33, 25
    cam = bfa.depth_camera(W, H, fx=LAT_F, fy=LAT_F, mx=16.0, my=12.0, zmin=0.125, zmax=4.0)
    p = small_hash(voxel_size=LAT_VS, truncation=2.0 ** -6, trunc_scale=0.0)
    d = np.full((H, W), 65.5 / 128, F)
    d[:, 17:] = 67.0 / 128
    # a second frame of three lone rays at depth 0.5 (from -66 to -62 voxels: blocks -9 and -8), integrated first:
    # the centre pixel, one on the centre column and one on the centre row, 8 or more pixels = voxels apart, so the
    # second block of each is reached by that ray alone
    lone = np.full((H, W), -np.inf, F)
    for x, y in LONE_RAYS:
        lone[y, x] = 0.5
    T = pose(t=(0.0, 0.0, -1.0))
    ops = [Op(T, frame=1), Op(T), Op(pose(t=(2.0 ** -7, 0.0, -1.0))), Op(T, deint=True)]
    return Case("d_dda", "ray_walk_from_ends: rayDir == 0 and bp - rayMin == 0, one-block rays",
                cam, p, [(d, colour_image(W, H, 4)), (lone, colour_image(W, H, 14))], ops)


ORIGIN_CHUNK = 0.16  # 16 voxels: blocks -1, 0 and 1 lie in three chunks (borders at +-(k + 0.5) chunk)


def case_origin(shard=None) -> Case:
    """e. The world plane z = 0 seen from 0.6 m at 37 degrees (cos 0.8, sin 0.6), principal point on a pixel,
    camera x = world x: the centre column's ray ends have x == 0.0 exactly, and the blocks straddle the origin in
    every octant. shard = index: the same with shardCount 2 and 16-voxel chunks, for which the corner of block
    +-1 lies exactly on the chunk rounding's tie (0.08 / 0.16 = 0.5)."""
    W, H = 48, 40
    cam = bfa.depth_camera(W, H, fx=60.0, fy=60.0, mx=24.0, my=20.0)
    p = small_hash(voxel_size=0.01)
    R = np.array([[1.0, 0.0, 0.0], [0.0, 0.8, 0.6], [0.0, -0.6, 0.8]])
    c = -0.6 * R[:, 2]
    T = pose(R, c)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    dirs = np.stack([(x - 24.0) / 60.0, (y - 20.0) / 60.0, np.ones_like(x, np.float64)], axis=-1) @ R.T
    d = (-c[2] / dirs[..., 2]).astype(F)
    opts, name = {}, "e_origin"
    if shard is not None:
        opts = dict(shard_count=2, shard_index=shard, shard_chunk=float(F(ORIGIN_CHUNK)))
        name = f"e_origin_shard{shard}"
    return Case(name, "world_to_block_rcp / vvox_to_block / owned at coordinates -1, 0 and 0.0",
                cam, p, [(d, colour_image(W, H, 5))], three_ops(T), scene_opts=opts)


DEPTH_MAX = 1.0
SENSOR_MIN, SENSOR_MAX = 0.05, 0.9
# column groups of 4 pixels: (name, depth, a ray of it allocates). The denormal is a depth like any other to the
# walk (not 0, not -inf): its ray runs from -0.06 to 0.06 m and reaches the block on the optical axis.
DEPTH_GROUPS = (
    ("minus_inf", -np.inf, False), ("plus_inf", np.inf, False), ("max_distance", DEPTH_MAX, False), ("nan", np.nan, False),
    ("negative", -0.5, False), ("zero", 0.0, False), ("sensor_min", SENSOR_MIN, True), ("minus_zero", -0.0, False),
    ("denormal", 1e-40, True), ("plain", 0.5, True),
    ("below_max_distance", float(np.nextafter(F(DEPTH_MAX), F(0.0))), True), ("beyond_sensor_max", 0.95, True),
)


def depth_group_image(only=None) -> np.ndarray:
    H = 12
    d = np.full((H, 4 * len(DEPTH_GROUPS)), -np.inf, F)
    for g, (name, v, _) in enumerate(DEPTH_GROUPS):
        if only is None or only == name:
            d[:, 4 * g:4 * g + 4] = F(v)
    return d


def case_depth_validity(colour=True) -> Case:
    """f. One image with a column group per kind of depth (DEPTH_GROUPS). maxIntegrationDistance 1.0, sensor
    range [0.05, 0.9], focal length 12.5: the sensor_min group allocates the block around the optical axis a few
    centimetres ahead of the camera, whose voxels project onto the neighbouring groups, so the voxel pass meets
    the 0.0, -0.0 and denormal depths with in-band voxels."""
    d = depth_group_image()
    H, W = d.shape
    cam = bfa.depth_camera(W, H, fx=12.5, fy=12.5, zmin=SENSOR_MIN, zmax=SENSOR_MAX)
    p = small_hash(voxel_size=0.01, max_integration_distance=DEPTH_MAX)
    T = pose(rotation((0.2, 1.0, -0.4), 5.0), (0.036, 0.034, -0.03))
    ops = three_ops(T, dt=(0.003, -0.002, 0.004))
    if not colour:
        ops = [Op(o.T, colour=False, deint=o.deint) for o in ops]
    return Case("f_depth_validity" if colour else "f_depth_validity_no_colour",
                "depth validity: the walk's d == -inf / 0 / >= max against dc_depth_word's and depth_tile_wave's",
                cam, p, [(d, colour_image(W, H, 6))], ops)


# g. (W, H) -> (8-pixel tiles, 16-pixel tiles) per axis
OFF_GRID = {(67, 45): ((9, 6), (5, 3)), (13, 9): ((2, 2), (1, 1)), (8, 8): ((1, 1), (1, 1)), (1, 1): ((1, 1), (1, 1)),
            (17, 16): ((3, 2), (2, 1))}


def case_off_grid(W: int, H: int) -> Case:
    """g. A tilted plane on an image off the 8- and 16-pixel tile grids. At 1x1 the frustum test divides by
    width - 1 = 0 (cameraToKinectProj, as the reference does): a block whose centre does not project to x = 0
    exactly is outside, so nothing is allocated; the case pins that both sides agree on that."""
    cam = bfa.depth_camera(W, H, fx=50.0, fy=50.0)
    p = small_hash(voxel_size=0.01)
    d = tilted_plane(W, H, 0.5, 0.004, 0.006)
    fine, coarse = OFF_GRID[(W, H)]
    return Case(f"g_off_grid_{W}x{H}", "depth_tile_wave / pack_dc / alloc_collect on partial 8- and 16-pixel tiles",
                cam, p, [(d, colour_image(W, H, 7))], three_ops(GENERAL_POSE), facts=dict(fine=fine, coarse=coarse))


def case_weight_cap(weight_max: int) -> Case:
    """h. integrationWeightMax 1, 2 or 3: the same frame integrated five times, de-integrated three times and
    integrated again."""
    W, H = 24, 20
    cam = bfa.depth_camera(W, H, fx=50.0, fy=50.0)
    p = small_hash(voxel_size=0.01, weight_max=weight_max)
    d = tilted_plane(W, H, 0.5, 0.004, 0.006)
    T = GENERAL_POSE
    ops = [Op(T)] * 5 + [Op(T, deint=True)] * 3 + [Op(T)]
    return Case(f"h_weight_cap_{weight_max}", "batch_integrate's weight cap as an integer min of float bits; emptied voxels",
                cam, p, [(d, colour_image(W, H, 8))], ops, facts=dict(weight_max=weight_max))


def case_big_focal(f: float = FOCAL_BIG) -> Case:
    """i. fx = fy = 2^21 (no usable reciprocal: ray_walk_ends divides in IEEE) on 24x24 pixels: voxels of 2^-20 m
    at 2 m, where a pixel is one voxel wide; lattice values throughout. 3 * 2^20 is the same with a focal length
    whose reciprocal is not a power of two."""
    W = H = 24
    cam = bfa.depth_camera(W, H, fx=f, fy=f, mx=11.5, my=11.5, zmin=0.125, zmax=4.0)
    p = small_hash(voxel_size=2.0 ** -20, truncation=2.0 ** -17, trunc_scale=0.0, max_integration_distance=4.0)
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    d = (2.0 + (x // 2 + y // 4) * 2.0 ** -20).astype(F)
    T = pose(t=(2.0 ** -18, -2.0 ** -19, 0.0))
    ops = [Op(T), Op(pose(t=(2.0 ** -18 + 2.0 ** -21, -2.0 ** -19, 2.0 ** -20))), Op(T, deint=True)]
    return Case(f"i_focal_{int(f)}", "ray_walk_ends with rFx == 0", cam, p, [(d, colour_image(W, H, 9))], ops)


def case_big_voxels() -> Case:
    """i. Case a with every length times 2^28: rVoxelSize == 0, world_to_block in IEEE. (|w| > 2^100, the third
    IEEE condition, is out of reach: normalize3 overflows there in the reference as well.)"""
    c = case_pixel_boundary(SCALE_BIG, name="i_voxel_size_2p21")
    c.edge = "ray_walk_ends with rVoxelSize == 0"
    return c


WORK_XCD_RUNS = (1, 64, 32768)
WORK_ROUNDS = (1, 64)


WORK_SCENES = ("67x45", "1x1", "one_ray")


def case_work_distribution(scene: str) -> Case:
    """j. One 10-op batch on an off-grid scene: 67x45 (a few hundred work-list blocks), 1x1 (none: see
    case_off_grid) and the 8x8 image with one valid pixel (one ray's blocks: fewer than 8)."""
    if scene == "one_ray":
        c = case_off_grid(8, 8)
        d = np.full((8, 8), -np.inf, F)
        d[4, 3] = c.frames[0][0][4, 3]
        c.frames = [(d, c.frames[0][1])]
    else:
        W, H = (int(v) for v in scene.split("x"))
        c = case_off_grid(W, H)
    T = GENERAL_POSE
    P = [T] + [shifted(T, (0.002 * k, -0.001 * k, 0.0015 * k)) for k in range(1, 5)]
    seq = ((0, 0), (1, 0), (2, 0), (0, 1), (3, 0), (1, 1), (0, 0), (4, 0), (2, 1), (1, 0))
    c.ops = [Op(P[k], deint=bool(de)) for k, de in seq]
    c.name = f"j_work_distribution_{scene}"
    c.edge = "k_apply_ops: XCD-run position mapping and rounds grid"
    return c


def case_mixed_colour() -> Case:
    """k. One batch on one frame: coloured, colour-less, coloured."""
    c = case_off_grid(17, 16)
    T = GENERAL_POSE
    c.ops = [Op(T), Op(shifted(T, (0.05, 0.0, 0.03)), colour=False), Op(shifted(T, (-0.002, 0.003, 0.0)))]
    c.name = "k_mixed_colour"
    c.edge = "an op without colour between two with, sharing one depth image"
    return c


CASES = {
    "a_pixel_boundary": case_pixel_boundary,
    "b_image_border": case_image_border,
    "b_rect_hi": case_rect_hi,
    "c_band_cull": case_band_cull,
    "d_dda": case_dda,
    "e_origin": case_origin,
    "e_origin_shard0": lambda: case_origin(0),
    "e_origin_shard1": lambda: case_origin(1),
    "f_depth_validity": case_depth_validity,
    "f_depth_validity_no_colour": lambda: case_depth_validity(False),
    **{f"g_off_grid_{w}x{h}": (lambda w=w, h=h: case_off_grid(w, h)) for w, h in OFF_GRID},
    **{f"h_weight_cap_{m}": (lambda m=m: case_weight_cap(m)) for m in (1, 2, 3)},
    f"i_focal_{int(FOCAL_BIG)}": case_big_focal,
    f"i_focal_{3 << 20}": lambda: case_big_focal(3.0 * 2.0 ** 20),
    "i_voxel_size_2p21": case_big_voxels,
    "k_mixed_colour": case_mixed_colour,
}


def make(name: str) -> Case:
    c = CASES[name]()
    assert c.name == name, (c.name, name)
    return c


# ---- host-side facts (float64 restatements; the tests' coverage conditions) ---------------------------------
_IDX = np.arange(512)
_OFF = np.stack([_IDX % 8, (_IDX % 64) // 8, _IDX // 64], axis=-1)


def block_voxel_coords(blocks) -> np.ndarray:
    """int64 [n, 512, 3]: the voxel coordinates of blocks [n, 3], in the block's storage order"""
    return np.asarray(blocks, np.int64).reshape(-1, 1, 3) * 8 + _OFF[None]


def project64(case: Case, T, vox) -> tuple:
    """integrateDepthMapKernel's projection of voxel coordinates vox [..., 3] in float64 from the float32
    parameters: camera position [..., 3], screen x, screen y."""
    cam, vs = case.cam, float(F(case.params.virtualVoxelSize))
    Ti = np.linalg.inv(np.asarray(T, np.float64).reshape(4, 4))
    pc = (np.asarray(vox, np.float64) * vs) @ Ti[:3, :3].T + Ti[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = pc[..., 0] * float(cam.fx) / pc[..., 2] + float(cam.mx)
        sy = pc[..., 1] * float(cam.fy) / pc[..., 2] + float(cam.my)
    return pc, sx, sy


def project32(case: Case, Tinv32, vox) -> tuple:
    """The same in float32 in the oracle's operation order (xform, then x * fx / z + mx), given the oracle's
    float32 inverse pose."""
    cam, vs = case.cam, F(case.params.virtualVoxelSize)
    e = np.asarray(Tinv32, F).reshape(4, 4)
    w = np.asarray(vox).astype(F) * vs
    pc = [(((e[r, 0] * w[..., 0] + e[r, 1] * w[..., 1]) + e[r, 2] * w[..., 2]) + e[r, 3] * F(1.0)) for r in range(3)]
    assert all(c.dtype == F for c in pc)
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = pc[0] * F(cam.fx) / pc[2] + F(cam.mx)
        sy = pc[1] * F(cam.fy) / pc[2] + F(cam.my)
    return np.stack(pc, axis=-1), sx, sy


def pixel_rule(case: Case, depth, pc, sx, sy) -> dict:
    """The voxel pass's decision per voxel from float64 projections: column / row = (int)(s + 0.5) truncated
    toward zero, on screen, the depth it reads, in band (|d - z| < truncation + truncScale d, d valid)."""
    W, H = case.cam.imageWidth, case.cam.imageHeight
    p = case.params
    with np.errstate(invalid="ignore"):
        ux, uy = np.trunc(sx + 0.5), np.trunc(sy + 0.5)
        on = np.isfinite(ux) & np.isfinite(uy) & (ux >= 0) & (ux < W) & (uy >= 0) & (uy < H)
        d = np.full(sx.shape, -np.inf)
        d[on] = np.asarray(depth, np.float64)[uy[on].astype(int), ux[on].astype(int)]
        valid = on & (d != -np.inf) & (d < float(F(p.maxIntegrationDistance)))
        band = valid & (np.abs(d - pc[..., 2]) < float(F(p.truncation)) + float(F(p.truncScale)) * d)
    return dict(ux=ux, uy=uy, on=on, depth=d, band=band)


def cull_footprints(case: Case, T, blocks) -> np.ndarray:
    """block_may_update_halves_q's path per block, restated in float64: 'plane' (a corner at z <= 1e-3: kept),
    'off' (rectangle off screen), 'fine' (within 3x3 8-pixel tiles), 'coarse' (3x3 16-pixel tiles), 'wide' (kept)."""
    W, H = case.cam.imageWidth, case.cam.imageHeight
    b = np.asarray(blocks, np.int64).reshape(-1, 3)
    corners = np.array([[(k >> c) & 1 for c in range(3)] for k in range(8)]) * 7
    pc, sx, sy = project64(case, T, b[:, None, :] * 8 + corners[None])
    out = []
    for k in range(len(b)):
        if not pc[k, :, 2].min() > 1e-3:
            out.append("plane")
            continue
        fx0, fx1 = np.floor(sx[k].min() - 0.5), np.floor(sx[k].max() + 1.5)
        fy0, fy1 = np.floor(sy[k].min() - 0.5), np.floor(sy[k].max() + 1.5)
        if fx1 < 0 or fy1 < 0 or fx0 > W - 1 or fy0 > H - 1:
            out.append("off")
            continue
        x0, x1, y0, y1 = int(max(fx0, 0)), int(min(fx1, W - 1)), int(max(fy0, 0)), int(min(fy1, H - 1))
        if x1 // DEPTH_TILE - x0 // DEPTH_TILE <= 2 and y1 // DEPTH_TILE - y0 // DEPTH_TILE <= 2:
            out.append("fine")
        elif x1 // DEPTH_TILE2 - x0 // DEPTH_TILE2 <= 2 and y1 // DEPTH_TILE2 - y0 // DEPTH_TILE2 <= 2:
            out.append("coarse")
        else:
            out.append("wide")
    return np.array(out)
