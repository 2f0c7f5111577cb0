"""The raycaster (csrc/raycast.hip) and mesh extraction (csrc/mc.hip) against the oracle at their tile, list and key
edges, on the inputs of render_edge_inputs.py (test_render_edges.py proves on the CPU that each reaches its edge).

Raycast: image sizes off the 64x8 splat tile and the 16x16 render tile, heights at and above the last one with
tile-row lists, the full-scan fallback, a camera inside the allocated band, and worlds whose blocks lie on both
sides of the LDS block table's key range. Every render is compared bit for bit: the no-ray masks, the clamped
interval ends (equal even where the oracle's clamped depth test ties: whichever rectangle wins, the clamp value
results), the raw interval ends where the oracle shows that nothing clamps, and depth, camera-space point,
colour and normal of every pixel (given equal intervals the march is the same float32 expression sequence on both
sides).

Mesh extraction: the same offset worlds, rejecting thresholds, surfaces on the cube-corner lattice, boxes whose
faces pass through voxel centres, every split of the triangle cap around the first blocks (nothing written behind
the cap), and the two-level scan run alone beyond 1024 chunks."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import bundlefusion_amd as bfa
import render_edge_inputs as R
from oracle_lib import OracleScene
from test_mc import canon, wall_scene
from tsdf_compare import compare_states

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
GRID = dict(default={}, overflow={"splat_row_cap": 1})   # scene options: tile-row lists, forced full-scan fallback


class World:
    """One volume on the oracle and on any number of GPU scenes (by scene options), with the oracle's renders
    kept: each reference is computed once and shared."""

    def __init__(self, offset=0.0):
        self.offset = offset
        self.params, self.cam = R.room_params(), R.room_camera()
        frames = R.room_frames(offset)
        self.dev = [(T, bfa.DeviceArray.from_host(d), bfa.DeviceArray.from_host(c)) for T, d, c in frames]
        self.ora = OracleScene(self.params)
        for T, d, c in frames:
            self.ora.integrate(T, d, c, self.cam)
        self.ora.garbageCollect()
        self.scenes, self.refs = {}, {}

    def gpu(self, name="default"):
        """The GPU scene of that name, built on first use (GRID's options; any other name: a further default scene)."""
        if name not in self.scenes:
            s = bfa.SceneRepHashSDF(self.params, **GRID.get(name, {}))
            for T, dd, cc in self.dev:
                s.integrate(T, dd, cc, self.cam)
            s.garbageCollect()
            self.scenes[name] = s
        return self.scenes[name]

    def oracle_render(self, pose_name, W, H, by_height=False, grad=False):
        key = (pose_name, W, H, by_height, grad)
        if key not in self.refs:
            cam, rp = R.view(W, H, by_height, use_gradients=grad)
            self.refs[key] = self.ora.raycast(self.pose(pose_name), cam, rp, want_intervals=True)
        return self.refs[key]

    def pose(self, pose_name):
        return R.inside_pose() if pose_name == "inside" else R.render_pose(self.offset)

    def render(self, scene, pose_name, W, H, by_height=False, grad=False):
        """The GPU render compared with the oracle's (check_render); returns the GPU's outputs."""
        cam, rp = R.view(W, H, by_height, use_gradients=grad)
        g = self.gpu(scene).raycast(self.pose(pose_name), cam, rp, want_intervals=True)
        o = self.oracle_render(pose_name, W, H, by_height, grad)
        check_render(g, o, rp, f"offset {self.offset}, {scene} scene, {pose_name} pose, {W}x{H}{', gradients' if grad else ''}")
        return g


@pytest.fixture(scope="module")
def room():
    return World(0.0)


@pytest.fixture(scope="module", params=R.OFFSETS[1:])
def far_world(request):
    return World(request.param)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def pixels(mask, *arrays):
    ys, xs = np.nonzero(mask)
    return [(int(x), int(y)) + tuple(a[y, x].tolist() for a in arrays) for y, x in list(zip(ys, xs))[:12]]


def check_render(g, o, rp, what):
    gd, g4, gn, gc, gmin, gmax = g
    od, o4, on, oc, omin, omax = o
    # 1. the same pixels have no ray
    g_none, glo, ghi = R.intervals(gmin, gmax, rp)
    o_none, olo, ohi = R.intervals(omin, omax, rp)
    bad = g_none != o_none
    assert not bad.any(), f"{what}: no-ray masks differ at {bad.sum()} pixels (x, y, gpu min/max, oracle min/max): " \
                          f"{pixels(bad, gmin, gmax, omin, omax)}"
    # 2. the clamped interval ends, bit for bit
    bad = (u32(glo) != u32(olo)) | (u32(ghi) != u32(ohi))
    assert not bad.any(), f"{what}: clamped intervals differ at {bad.sum()} pixels (x, y, gpu lo/hi, oracle lo/hi): " \
                          f"{pixels(bad, glo, ghi, olo, ohi)}"
    # 3. the raw ends, where no rectangle's depth is clamped (no tie in the oracle's depth test)
    near, far = R.clamped(omin, omax, rp)
    if not near.any():
        bad = u32(gmin) != u32(omin)
        assert not bad.any(), f"{what}: raw rayMin differs at {bad.sum()} pixels: {pixels(bad, gmin, omin)}"
    if not far.any():
        bad = u32(gmax) != u32(omax)
        assert not bad.any(), f"{what}: raw rayMax differs at {bad.sum()} pixels: {pixels(bad, gmax, omax)}"
    # 4. every output of every pixel (as bits: -inf equals -inf)
    same = u32(gd) == u32(od)
    for a, b in ((g4, o4), (gc, oc), (gn, on)):
        same &= np.all(u32(a) == u32(b), axis=-1)
    print(f"{what}: exact-match fraction {same.mean():.6f} of {same.size} pixels, hit fraction {np.isfinite(od).mean():.4f}")
    bad = ~same
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} pixels differ (x, y, gpu depth, oracle depth, gpu lo/hi): " \
                          f"{pixels(bad, gd, od, glo, ghi)}"
    assert np.isfinite(od).any()


def same_bits(a, b):
    return all(np.array_equal(u32(x), u32(y)) for x, y in zip(a, b))


# ---- raycast ---------------------------------------------------------------------------------------------------
def test_render_sizes_on_one_scene(room):
    """Every size in turn on one scene (the splat buffers grow and are reused; the row-list buffers come with the
    first render), then the first size again: the same bits as the first time."""
    first = room.render("default", "room", *R.RENDER_SIZES[0])
    for W, H in R.RENDER_SIZES[1:]:
        room.render("default", "room", W, H)
    again = room.render("default", "room", *R.RENDER_SIZES[0])
    assert same_bits(first, again)


@pytest.mark.parametrize("W,H", [(65, 9), (129, 25), (160, 120)])
def test_full_scan_fallback_off_the_tile_grid(room, W, H):
    room.render("overflow", "room", W, H)


def test_tall_renders_with_and_without_row_lists(room):
    """2048 rows fill tile row 255 of the row lists; 2056 rows drop the lists (every tile scans every rectangle);
    a small render afterwards takes the lists again."""
    for W, H in R.TALL_SIZES:
        g = room.render("tall", "room", W, H, by_height=True)
        assert np.isfinite(g[0][-R.SPLAT_TILE_H:]).sum() >= 100
    room.render("tall", "room", 65, 9)


@pytest.mark.parametrize("scene", list(GRID))
@pytest.mark.parametrize("W,H", [(160, 120), (65, 9)])
def test_camera_inside_the_allocated_band(room, scene, W, H):
    g = room.render(scene, "inside", W, H)
    if (W, H) == (160, 120):   # the near-plane branch ran on the device too
        _, rp = R.view(W, H)
        assert R.clamped(g[4], g[5], rp)[0].sum() >= 1000


def test_offset_world_volumes_match(far_world):
    assert compare_states(far_world.params, far_world.gpu(), far_world.ora) > 4000


@pytest.mark.parametrize("W,H,grad", [(160, 120, False), (65, 9, False), (160, 120, True)])
def test_offset_world_renders(far_world, W, H, grad):
    far_world.render("default", "room", W, H, grad=grad)


# ---- mesh extraction ---------------------------------------------------------------------------------------------
def assert_same_mesh(gpu, ora, mc, at_least=0):
    g, gt = gpu.extract_mesh(mc)
    o, ot = ora if isinstance(ora, tuple) else ora.extract_mesh(mc)
    assert gt == ot == len(o) == len(g), (gt, ot, len(o), len(g))
    assert gt >= at_least
    assert np.array_equal(canon(g), canon(o))
    return gt


def test_offset_world_meshes(far_world):
    assert_same_mesh(far_world.gpu(), far_world.ora, bfa.mc_params(R.VS), at_least=100000)


def test_thresholds_that_reject(room):
    factors = R.THRESH_FACTORS[1:]
    with ThreadPoolExecutor(len(factors)) as ex:   # the oracle call releases the interpreter lock and only reads
        refs = list(ex.map(lambda f: room.ora.extract_mesh(bfa.mc_params(R.VS, thresh_factor=f)), factors))
    totals = [assert_same_mesh(room.gpu(), ref, bfa.mc_params(R.VS, thresh_factor=f)) for f, ref in zip(factors, refs)]
    assert totals[0] > totals[1] > totals[2] == 0, totals


@pytest.mark.parametrize("depth", R.WALL_DEPTHS)
def test_walls_on_and_off_the_corner_lattice(depth):
    p, cam, d, c = wall_scene(R.VS, depth=depth)
    gpu, ora = bfa.SceneRepHashSDF(p), OracleScene(p)
    dd, cc = bfa.DeviceArray.from_host(d), bfa.DeviceArray.from_host(c)
    I = np.eye(4, dtype=np.float32)
    for _ in range(2):
        gpu.integrate(I, dd, cc, cam)
        ora.integrate(I, d, c, cam)
    g, _ = gpu.extract_mesh(bfa.mc_params(R.VS))
    assert_same_mesh(gpu, ora, bfa.mc_params(R.VS), at_least=10000)
    lat = R.on_corner_lattice(g[..., 2])
    assert lat.all() if depth == 1.005 else not lat.any()


@pytest.fixture(scope="module")
def first_blocks(room):
    """The first allocated heap blocks of the GPU scene and the oracle's triangles of each (its box, faces through
    the centres of its first and last voxel: isInBoxAA keeps a voxel on the boundary), in the oracle's (voxel,
    triTable) order. Which block a heap slot holds follows the allocation schedule and varies run to run, so the
    list is the first eight extended until three of its blocks emit triangles (the counts are then neither all
    equal nor all zero, and there are block boundaries to put a cap on)."""
    blocks = room.gpu().export_blocks()
    first, lists = [], []
    for b in blocks[blocks[:, 3] != 0][:96]:
        first.append(b)
        lists.append(room.ora.extract_mesh(bfa.mc_params(R.VS, box=R.block_box(b)))[0])
        counts = [len(t) for t in lists]
        if len(first) >= 8 and sum(c > 0 for c in counts) >= 3 and len(set(counts)) > 1:
            break
    else:
        raise AssertionError(f"the first {len(first)} heap blocks emit too few triangles: {counts}")
    return first, lists


def test_inclusive_box_edges(room, first_blocks):
    first, lists = first_blocks
    for b, ref in zip(first, lists):
        n = assert_same_mesh(room.gpu(), (ref, len(ref)), bfa.mc_params(R.VS, box=R.block_box(b)))
        padded = bfa.mc_params(R.VS, box=R.block_box(b, 0.25))   # the same voxels: none lies within a quarter voxel outside
        assert room.gpu().extract_mesh(padded)[1] == room.ora.extract_mesh(padded)[1] == n


def test_cap_splits_blocks_and_voxels_and_writes_nothing_behind_it(room, first_blocks):
    first, lists = first_blocks
    L, scene = bfa.lib(), room.gpu()
    full, total = scene.extract_mesh(bfa.mc_params(R.VS))
    assert len(full) == total > 100000
    # heap order: the first blocks' triangles lead the output, block by block, in the oracle's order
    head = np.concatenate(lists)
    assert np.array_equal(u32(full[: len(head)]), u32(head))
    bounds = np.cumsum([len(t) for t in lists]).tolist()
    # a cap inside a voxel: two consecutive triangles of one voxel (a triangle's corners lie on the edges of the cube
    # around its voxel's centre, so its centroid rounds to that voxel)
    vox = np.rint(head[..., :3].astype(np.float64).mean(axis=1) / R.VS).astype(np.int64)
    twin = np.nonzero(np.all(vox[1:] == vox[:-1], axis=1))[0]
    assert len(twin) > 0
    caps = {0, 1, int(twin[0]) + 1, total - 1, total, total + 1}
    for b in bounds:
        caps |= {b - 1, b, b + 1}
    buf = bfa.DeviceArray((total + 8, 18), np.uint32)
    blank = np.full((total + 8, 18), SENTINEL, np.uint32)
    ref = u32(full).reshape(total, 18)
    for cap in sorted(c for c in caps if c >= 0):
        buf.upload(blank)
        n, tot = C.c_uint32(), C.c_uint32()
        mc = bfa.mc_params(R.VS, max_triangles=cap)
        bfa.check(L.bf_scene_extract_mesh(scene.h, C.byref(mc), buf.ptr, C.byref(n), C.byref(tot)))
        keep = min(cap, total)
        assert (n.value, tot.value) == (keep, total), cap
        got = buf.download()
        assert np.array_equal(got[:keep], ref[:keep]), cap
        assert np.all(got[keep:] == SENTINEL), cap     # nothing behind the cap


@pytest.mark.parametrize("values", ["counts", "wrapping"])
def test_two_level_scan_beyond_1024_chunks(values):
    """bf_debug_mc_scan: the block offset chunkSum[i / 1024] + prefix[i] and the total at chunkSum[nChunks], at
    lengths around one chunk, around 1024 chunks (k_mc_scan_top's second round) and in its third round."""
    L, Ch = bfa.lib(), 1024
    lengths = [1, Ch - 1, Ch, Ch + 1, Ch * Ch - 1, Ch * Ch, Ch * Ch + 1, 2 * Ch * Ch + Ch + 3]
    nmax = lengths[-1]
    rng = np.random.default_rng(7)
    if values == "counts":   # at most 5 triangles per voxel: 2560 per block
        host = rng.integers(0, 2561, nmax, dtype=np.uint64).astype(np.uint32)
    else:                    # full range: the sums wrap
        host = rng.integers(0, 1 << 32, nmax, dtype=np.uint64).astype(np.uint32)
    d_counts = bfa.DeviceArray.from_host(host)
    cmax = -(-nmax // Ch) + 1
    d_prefix, d_chunk = bfa.DeviceArray(nmax + 8, np.uint32), bfa.DeviceArray(cmax + 8, np.uint32)
    blank_p, blank_c = np.full(nmax + 8, SENTINEL, np.uint32), np.full(cmax + 8, SENTINEL, np.uint32)
    incl = np.cumsum(host, dtype=np.uint32)
    excl = np.concatenate([np.zeros(1, np.uint32), incl[:-1]])
    for n in lengths:
        d_prefix.upload(blank_p)
        d_chunk.upload(blank_c)
        bfa.check(L.bf_debug_mc_scan(d_counts.ptr, C.c_uint32(n), d_prefix.ptr, d_chunk.ptr))
        prefix, chunk = d_prefix.download(), d_chunk.download()
        nch = -(-n // Ch)
        got = chunk[np.arange(n) // Ch] + prefix[:n]      # uint32: wraps like the kernel's sum
        bad = np.nonzero(got != excl[:n])[0]
        assert len(bad) == 0, f"n {n}: {len(bad)} offsets differ, the first at {bad[0]}"
        assert chunk[nch] == incl[n - 1], n
        assert np.all(prefix[n:] == SENTINEL) and np.all(chunk[nch + 1:] == SENTINEL), n
