"""The image kernels off the tile grid: frames.hip (erode, bilateral filter, resample), cache.hip (the dense-term
cache) and corr.hip (the EntryJ producer) against the CPU oracle (oracle/frames.cpp), bit for bit, at the sizes
where their tiles, tails, scans and template instantiations change path. The inputs (image_edge_inputs.py) are
checked by test_image_edges.py to have pixels and pairs on both sides of every branch used here.

No tolerance anywhere: the oracle restates the reference's staged passes expression by expression and both
sides are built without floating-point contraction."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
from bundlefusion_amd import io as bio
from bundlefusion_amd.cache import CUDACache, cache_options
from bundlefusion_amd.corr import corr_from_depth, corr_options
from image_edge_inputs import (CACHE_SHAPES, CACHE_TAIL, CORR_H, CORR_OPTION_SETS, CORR_W, CORR_WINDOWS, FX,
                               OFF_GRID_SIZES, RESAMPLE_SIZES, boundary_sizes, corr_intrinsics, corr_problem,
                               depth_metres, flat_frame, pose_inverse, sensor_frame)
from oracle_lib import cache_store_frame, corr_from_depth as or_corr, preprocess

pytestmark = pytest.mark.gpu

BF_ERR_ARG, BF_ERR_CAPACITY = -2, -3


def same_bits(got, want, what):
    g = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    w = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    assert g.shape == w.shape, what
    bad = np.nonzero(g != w)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} bytes differ, first at byte {bad[0]}"


# ---- preprocessing -------------------------------------------------------------------------------------
def run_gpu(pp, u16, rgbx, iwh):
    dd = bfa.DeviceArray.from_host(u16)
    dc = bfa.DeviceArray.from_host(rgbx)
    od = bfa.DeviceArray((iwh[1], iwh[0]), np.float32)
    oc = bfa.DeviceArray((iwh[1], iwh[0], 4), np.uint8)
    pp.run(dd, dc, od, oc)
    return od.download(), oc.download()


def check_preprocess(opts, u16, rgbx, iwh=None, what=""):
    H, W = u16.shape
    ch, cw = rgbx.shape[:2]
    iwh = iwh or (W, H)
    gd, gc = run_gpu(bio.Preprocessor((W, H), (cw, ch), iwh, opts), u16, rgbx, iwh)
    od, oc = preprocess(opts, u16, rgbx, iwh)
    same_bits(gd, od, f"depth {what} {W}x{H} -> {iwh}")
    same_bits(gc, oc, f"colour {what} {cw}x{ch} -> {iwh}")
    return gd


@pytest.mark.parametrize("R", range(8))
def test_erode_interior_boundary(R):
    """k_erode<R> at the smallest image with an interior workgroup and at the two next to it that have none;
    on the flat frame a tap from outside the image would be counted (with the fraction 0.004, a single one)."""
    for W, H in boundary_sizes(R):
        u16, col = sensor_frame(W, H, R)
        out = check_preprocess(bio.preprocess_options(structure=R, depth_filter=False), u16, col, what=f"erode<{R}>")
        assert R == 0 or 0 < np.isfinite(out).sum() < (u16 > 0).sum()
        fu, fc = flat_frame(W, H)
        for frac in (0.3, 0.004):
            o = bio.preprocess_options(structure=R, depth_filter=False, erode_fraction=frac)
            check_preprocess(o, fu, fc, what=f"flat erode<{R}> fraction {frac}")


@pytest.mark.parametrize("R", range(1, 8))
def test_gauss_interior_boundary(R):
    """k_gauss<R> (sigmaD = R / 2: radius ceil(2 sigmaD) = R) likewise; with sigmaR = 100 every valid tap is
    weighted, so a stray 0.0f from outside the image moves the result."""
    for W, H in boundary_sizes(R):
        u16, col = sensor_frame(W, H, R)
        check_preprocess(bio.preprocess_options(erode=False, sigma_d=R / 2), u16, col, what=f"gauss<{R}>")
        wide = bio.preprocess_options(erode=False, sigma_d=R / 2, sigma_r=100.0)
        check_preprocess(wide, u16, col, what=f"gauss<{R}> sigmaR 100")
        check_preprocess(wide, *flat_frame(W, H), what=f"flat gauss<{R}> sigmaR 100")


@pytest.mark.parametrize("W,H", OFF_GRID_SIZES)
def test_preprocess_off_grid(W, H):
    u16, col = sensor_frame(W, H, 11)
    check_preprocess(bio.preprocess_options(), u16, col, what="defaults")
    big = bio.preprocess_options(structure=7, sigma_d=3.5)   # radius 7: larger than the 5x3 image
    check_preprocess(big, u16, col, what="radius 7")
    check_preprocess(bio.preprocess_options(structure=7, sigma_d=3.5, sigma_r=100.0), *flat_frame(W, H), what="flat radius 7")


@pytest.mark.parametrize("W,H", RESAMPLE_SIZES)
def test_preprocess_resampling(W, H):
    u16, _ = sensor_frame(W, H, 5)
    col = sensor_frame(W + 11, H + 6, 6)[1]          # a colour size of its own
    o = bio.preprocess_options()
    for iwh in ((W // 2 + 1, H // 2 + 1), (W + 9, H + 5)):     # down, up
        check_preprocess(o, u16, col, iwh, what="resample")
    # colour at the integration size (copied) while depth is resampled
    check_preprocess(o, u16, sensor_frame(W + 9, H + 5, 7)[1], (W + 9, H + 5), what="colour copied")
    # depth at the integration size (copied / written directly) while colour is resampled
    check_preprocess(o, u16, col, (W, H), what="depth copied")


@pytest.mark.parametrize("iwh", [(640, 480), (320, 240)])
def test_preprocess_sens_shape(iwh):
    u16, _ = sensor_frame(640, 480, 2)
    col = sensor_frame(1296, 968, 3)[1]
    check_preprocess(bio.preprocess_options(), u16, col, iwh, what=".sens")


def test_preprocess_keeps_no_state_between_frames():
    W, H, iwh = 67, 19, (34, 10)
    o = bio.preprocess_options()
    pp = bio.Preprocessor((W, H), (W, H), iwh, o)
    (a16, ac), (b16, bc) = sensor_frame(W, H, 21), sensor_frame(W, H, 22)
    run_gpu(pp, a16, ac, iwh)
    gd, gc = run_gpu(pp, b16, bc, iwh)
    od, oc = preprocess(o, b16, bc, iwh)
    same_bits(gd, od, "depth of the second frame")
    same_bits(gc, oc, "colour of the second frame")
    assert not np.array_equal(od.view(np.uint32), preprocess(o, a16, ac, iwh)[0].view(np.uint32))


def preproc_create(dwh, cwh, iwh, opts):
    h = C.c_void_p()
    rc = bfa.lib().bf_preproc_create(C.c_uint32(dwh[0]), C.c_uint32(dwh[1]), C.c_uint32(cwh[0]), C.c_uint32(cwh[1]),
                                     C.c_uint32(iwh[0]), C.c_uint32(iwh[1]), C.byref(opts), C.byref(h))
    if rc == 0:
        assert bfa.lib().bf_preproc_destroy(h) == 0
    else:
        assert not h.value
    return rc


def test_preprocess_argument_errors():
    ok = bio.preprocess_options()
    s = (20, 10)
    assert preproc_create(s, s, s, ok) == 0
    for bad in (bio.preprocess_options(structure=8), bio.preprocess_options(sigma_d=3.6),
                bio.preprocess_options(depth_shift=0.0)):
        assert preproc_create(s, s, s, bad) == BF_ERR_ARG
    for dwh, cwh, iwh in (((0, 10), s, s), ((20, 0), s, s), (s, s, (0, 10)), (s, s, (20, 0)),
                          # a resample divides by (size - 1): sizes of 1 are refused where one runs ...
                          (s, s, (1, 10)), (s, s, (20, 1)), ((1, 10), s, s), ((20, 1), s, s), ((1, 1), (1, 1), (2, 2)),
                          ((1, 1), (4, 4), (1, 1)), ((20, 1), (4, 4), (20, 1)),
                          # ... and a colour size with a zero in it
                          (s, (0, 10), s), (s, (20, 0), s)):
        assert preproc_create(dwh, cwh, iwh, ok) == BF_ERR_ARG, (dwh, cwh, iwh)
        assert b"size" in bfa.lib().bf_last_error()
    # equal sizes are copied: legal at any size
    for dwh, cwh, iwh in (((1, 1), (1, 1), (1, 1)), ((1, 7), (1, 7), (1, 7)), ((20, 1), (0, 0), (20, 1)),
                          (s, (1, 1), (2, 2)), (s, (0, 0), (7, 5))):
        assert preproc_create(dwh, cwh, iwh, ok) == 0, (dwh, cwh, iwh)
    u16 = np.full((1, 1), 1234, np.uint16)
    col = np.full((1, 1, 4), 77, np.uint8)
    out = check_preprocess(ok, u16, col, what="1x1")
    assert out[0, 0] == np.float32(1234) / np.float32(1000)
    # created without a colour size: a colour image is refused, depth alone runs
    pp = bio.Preprocessor(s, (0, 0), s, ok)
    u16, col = sensor_frame(*s)
    dd, dc = bfa.DeviceArray.from_host(u16), bfa.DeviceArray.from_host(col)
    od, oc = bfa.DeviceArray((s[1], s[0]), np.float32), bfa.DeviceArray((s[1], s[0], 4), np.uint8)
    with pytest.raises(bfa.BFError) as ei:
        pp.run(dd, dc, od, oc)
    assert ei.value.code == BF_ERR_ARG
    pp.run(dd, None, od, None)
    same_bits(od.download(), preprocess(ok, u16, None, s)[0], "depth without colour")


def test_preprocess_rejected_create_leaves_the_library_usable():
    """bf_preproc_create destroys its stream when the options are refused. 64 refusals and a valid create after
    them document that path; they do not prove that nothing leaks."""
    s = (20, 10)
    bad = bio.preprocess_options(structure=8)
    for _ in range(64):
        assert preproc_create(s, s, s, bad) == BF_ERR_ARG
    check_preprocess(bio.preprocess_options(), *sensor_frame(*s), what="after 64 refusals")


# ---- cache ---------------------------------------------------------------------------------------------
CACHE_KEYS = ("depth", "campos", "normals", "normalsU8", "intensity", "intensityDeriv")


def cache_case(inp, out, col, seed=0, max_frames=1, **kw):
    (iW, iH), (W, H), (cW, cH) = inp, out, col
    f = FX * iW / 640
    o = cache_options(iW, iH, f, f, (iW - 1) / 2, (iH - 1) / 2, max_frames, width=W, height=H, **kw)
    d = depth_metres(sensor_frame(iW, iH, seed)[0])
    c = sensor_frame(cW, cH, seed + 100)[1]
    return o, d, c


def store(cache, d, c):
    dd, cc = bfa.DeviceArray.from_host(d), bfa.DeviceArray.from_host(c)
    i = cache.storeFrame(dd, cc, c.shape[1], c.shape[0])
    cache.synchronize()
    return i


def check_cache_frame(cache, i, o, d, c, what):
    g, r = cache.download(i), cache_store_frame(o, d, c)
    for k in CACHE_KEYS:
        same_bits(g[k], r[k], f"{what}: frame {i} {k}")
    return g, r


@pytest.mark.parametrize("shape", [CACHE_TAIL] + CACHE_SHAPES)
def test_cache_off_grid_shapes(shape):
    o, d, c = cache_case(*shape)
    cache = CUDACache(o)
    assert store(cache, d, c) == 0
    g, r = check_cache_frame(cache, 0, o, d, c, str(shape))
    K, Ki = cache.intrinsics()
    same_bits(K, r["K"], "K")
    same_bits(Ki, r["Kinv"], "Kinv")
    assert np.isfinite(g["normals"][..., 0]).any() and not np.isfinite(g["normals"][..., 0]).all()


@pytest.mark.parametrize("k", range(9))
def test_cache_every_radius(k):
    """sigma 0 (no filter: radius -1) and 0.5 .. 3.5 (radius ceil(2 sigma) = 1 .. 7) for both kernels, paired
    off: eight stores reach k_cache_geometry<-1, 1 .. 7> and k_cache_intensity<-1, 1 .. 7>, the ninth runs
    both unfiltered. Radius 0 needs sigma in (0, 0]: no option selects it."""
    sig = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5]
    ds, cs = (sig[k], sig[7 - k]) if k < 8 else (0.0, 0.0)
    o, d, c = cache_case(*CACHE_TAIL, seed=k, depth_sigma_d=ds, color_sigma=cs)
    cache = CUDACache(o)
    store(cache, d, c)
    check_cache_frame(cache, 0, o, d, c, f"depthSigmaD {ds} colorSigma {cs}")


def test_cache_frames_do_not_bleed():
    """273 pixels per frame: frame f ends 17 pixels into a workgroup of 64, whose other 47 lanes would land in
    frame f + 1."""
    frames = [cache_case(*CACHE_TAIL, seed=s, max_frames=3) for s in (31, 32, 33)]
    o = frames[0][0]
    cache = CUDACache(o)
    for k, (_, d, c) in enumerate(frames):
        assert store(cache, d, c) == k
        for j in range(k + 1):        # every earlier frame is still what it was (frame 0 after A and B, ...)
            check_cache_frame(cache, j, o, frames[j][1], frames[j][2], f"after {k + 1} stores")
    assert cache.getNumFrames() == 3
    with pytest.raises(bfa.BFError) as ei:
        store(cache, frames[0][1], frames[0][2])
    assert ei.value.code == BF_ERR_CAPACITY
    for j in range(3):
        check_cache_frame(cache, j, o, frames[j][1], frames[j][2], "after the refused store")


def test_cache_argument_errors():
    f = FX * 67 / 640

    def create(iW=67, iH=51, W=21, H=13, max_frames=1, **kw):
        o = cache_options(iW, iH, f, f, (iW - 1) / 2, (iH - 1) / 2, max_frames, width=W, height=H, **kw)
        h = C.c_void_p()
        rc = bfa.lib().bf_cache_create(C.byref(o), C.byref(h))
        if rc == 0:
            bfa.lib().bf_cache_destroy(h)
        return rc

    assert create() == 0
    for kw in (dict(W=1), dict(H=1), dict(iW=1), dict(iH=1), dict(W=1025, H=1024), dict(max_frames=0),
               dict(depth_sigma_d=3.6), dict(color_sigma=3.6)):
        assert create(**kw) == BF_ERR_ARG, kw
    assert create(W=1024, H=1024, iW=8, iH=8) == 0       # 2^20 pixels is the limit itself
    o, d, c = cache_case(*CACHE_TAIL)
    cache = CUDACache(o)
    dd, cc = bfa.DeviceArray.from_host(d), bfa.DeviceArray.from_host(c)
    for cw, ch in ((1, 70), (90, 1)):
        with pytest.raises(bfa.BFError) as ei:
            cache.storeFrame(dd, cc, cw, ch)
        assert ei.value.code == BF_ERR_ARG
    assert cache.getNumFrames() == 0                      # a refused store takes no slot
    assert store(cache, d, c) == 0
    check_cache_frame(cache, 0, o, d, c, "after refused stores")


# ---- EntryJ producer -----------------------------------------------------------------------------------
class CorrProblem:
    """corr_problem(n) on the device: four depth buffers, a pointer per frame, the poses."""

    def __init__(self, n, T=None):
        self.images, self.sel, T0, _ = corr_problem(n)
        self.T = T0 if T is None else T
        self.Tinv = pose_inverse(self.T)
        self.depths = [self.images[s] for s in self.sel]
        self.dev = [bfa.DeviceArray.from_host(a) for a in self.images]
        self.ptrs = [self.dev[s].ptr.value for s in self.sel]
        self.dT, self.dTi = bfa.DeviceArray.from_host(self.T), bfa.DeviceArray.from_host(self.Tinv)

    def gpu(self, cur, start, o, cap):
        return corr_from_depth(self.ptrs, self.dT, self.dTi, cur, start, o, cap)

    def oracle(self, cur, start, o, cap):
        return or_corr(self.depths, self.T, self.Tinv, cur, start, o, cap)

    def check(self, cur, start, o, cap=None):
        cap = (cur - start) * o.maxPerPair + 1 if cap is None else cap
        g, gt = self.gpu(cur, start, o, cap)
        r, rt = self.oracle(cur, start, o, cap)
        assert gt == rt, (cur, start, gt, rt)
        same_bits(g, r, f"EntryJ of ({cur}, {start})")
        return g, gt


def corr_opts(stride, max_pp, min_pp):
    return corr_options(CORR_W, CORR_H, *corr_intrinsics(), stride=stride, max_per_pair=max_pp, min_per_pair=min_pp)


@pytest.fixture(scope="module")
def corr1100():
    return CorrProblem(1100)


@pytest.mark.parametrize("stride,max_pp,min_pp", CORR_OPTION_SETS)
@pytest.mark.parametrize("cur,start", CORR_WINDOWS)
def test_corr_pair_counts(corr1100, cur, start, stride, max_pp, min_pp):
    g, total = corr1100.check(cur, start, corr_opts(stride, max_pp, min_pp))
    if cur - start >= 64:
        assert 0 < total < (cur - start) * max_pp
    if cur == start:
        assert total == 0 and len(g) == 0


def test_corr_output_cap(corr1100):
    o = corr_opts(8, 25, 5)
    full, total = corr1100.check(1099, 0, o)
    assert total == len(full) > 1024
    for cap in (10, total - 1, total, 0):
        g, gt = corr1100.check(1099, 0, o, cap)
        assert gt == total and len(g) == min(cap, total)
        same_bits(g, full[:cap], f"the first {cap} records")


def test_corr_run_to_run(corr1100):
    o = corr_opts(4, 64, 1)
    a, ta = corr1100.gpu(1099, 0, o, 1099 * 64)
    b, tb = corr1100.gpu(1099, 0, o, 1099 * 64)
    assert ta == tb and a.tobytes() == b.tobytes()


def test_corr_degenerate_poses():
    n, o = 70, corr_opts(8, 25, 1)
    T = corr_problem(n)[2]
    base, total = CorrProblem(n).check(69, 0, o)
    bad = next(k for k in range(10, 69) if (base["i"] == k).sum() > 0)
    Tb = T.copy()
    Tb[bad] = -np.inf                    # an invalid pose: no match with that frame as i
    g, gt = CorrProblem(n, Tb).check(69, 0, o)
    assert gt == total - (base["i"] == bad).sum() and not (g["i"] == bad).any()
    Tc = T.copy()
    Tc[69] = -np.inf                     # ... and none at all when it is cur
    assert CorrProblem(n, Tc).check(69, 0, o)[1] == 0
    for dx in (0.0, 40.0, -40.0):        # pj.z ~ 1e-6: the projected pixel is far outside, then beyond +-2^31
        Tz = T.copy()
        Tz[69, 2, 3] = np.float32(2.0 - 1e-6)
        Tz[69, 0, 3] += np.float32(dx)
        p = CorrProblem(n, Tz)
        assert p.check(69, 0, o)[1] == 0
        assert p.check(68, 0, o)[1] > 0


def test_corr_argument_errors(corr1100):
    p = corr1100
    ptrs = bfa.DeviceArray.from_host(np.asarray(p.ptrs, np.uint64))
    out = bfa.DeviceArray((16,), bfa.abi.ENTRYJ_DTYPE)

    def call(o, cur=5, start=0, outp=out.ptr, cap=16):
        n, total = C.c_uint32(), C.c_uint32()
        return bfa.lib().bf_corr_from_depth(ptrs.ptr, p.dT.ptr, p.dTi.ptr, C.c_uint32(cur), C.c_uint32(start), C.byref(o),
                                            outp, C.c_uint32(cap), C.byref(n), C.byref(total))

    def opts(stride=8, max_pp=25):
        return corr_options(CORR_W, CORR_H, *corr_intrinsics(), stride=stride, max_per_pair=max_pp)

    assert call(opts()) == 0
    for o in (opts(max_pp=0), opts(max_pp=65), opts(stride=0), opts(stride=73), opts(stride=53)):
        assert call(o) == BF_ERR_ARG
    assert call(opts(), cur=3, start=4) == BF_ERR_ARG
    assert call(opts(), outp=None, cap=16) == BF_ERR_ARG
    assert call(opts(), outp=None, cap=0) == 0            # counting only
    assert call(opts(stride=52, max_pp=64)) == 0          # the limits themselves: a 1 x 1 grid
