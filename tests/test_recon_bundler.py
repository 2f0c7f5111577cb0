"""CPU checks of the pose-free loop's entry points (bf_recon_attach_bundler, _set_frame_bundling, _bundler_frame,
_bundling_stats): the header declares and the library exports them, every null argument is refused with BF_ERR_ARG before
anything is dereferenced or any device call is made, and BFReconBundling has the size the library gives it."""
import ctypes as C

import bundlefusion_amd as bfa
from bundlefusion_amd import abi
from bundlefusion_amd.recon import bundler_cache_intrinsics
from test_bundler import options

BF_ERR_ARG = -2
FUNCTIONS = ["bf_recon_attach_bundler", "bf_recon_set_frame_bundling", "bf_recon_bundler_frame", "bf_recon_bundling_stats"]


def test_header_declares_and_library_exports_the_four_names():
    declared = set(abi.header_functions())
    L = C.CDLL(abi.LIB_PATH)
    for name in FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
    # the sets of bf_bundler_* / bf_retry_* names are pinned elsewhere: every new name is a bf_recon_ one
    assert all(n.startswith("bf_recon_") for n in FUNCTIONS)


def test_null_arguments_are_refused_without_a_device():
    L = bfa.lib()
    word = (C.c_uint64 * 32)()  # stands for a handle or an image: never dereferenced, every call below is refused first
    p = C.cast(word, C.c_void_p)
    u = C.c_uint32
    for r, b in ((None, p), (p, None), (None, None)):
        assert L.bf_recon_attach_bundler(r, b) == BF_ERR_ARG
        assert b"null" in L.bf_last_error()
    for r, c, df, dr in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None), (None, None, None, None)):
        assert L.bf_recon_set_frame_bundling(r, u(0), c, u(320), u(240), df, dr) == BF_ERR_ARG
        assert b"null" in L.bf_last_error()
    rec, st = abi.BFBundlerFrame(), abi.BFReconBundling()
    for r, out in ((None, C.byref(rec)), (p, None), (None, None)):
        assert L.bf_recon_bundler_frame(r, u(0), out) == BF_ERR_ARG
        assert b"null" in L.bf_last_error()
    for r, out in ((None, C.byref(st)), (p, None), (None, None)):
        assert L.bf_recon_bundling_stats(r, out) == BF_ERR_ARG
        assert b"null" in L.bf_last_error()


def test_struct_size_matches_the_library_and_the_abi_version_stays():
    L = bfa.lib()
    n = C.c_size_t()
    assert L.bf_abi_struct_size(b"BFReconBundling", C.byref(n)) == 0
    assert n.value == C.sizeof(abi.BFReconBundling) == 64
    assert L.bf_abi_version() == abi.ABI_VERSION == 4
    # no existing struct gained a field
    assert L.bf_abi_struct_size(b"BFReconOptions", C.byref(n)) == 0 and n.value == C.sizeof(abi.BFReconOptions)
    assert L.bf_abi_struct_size(b"BFReconStats", C.byref(n)) == 0 and n.value == C.sizeof(abi.BFReconStats)
    assert [k for k, _ in abi.BFReconOptions._fields_][-1] == "bundlingPriority"
    assert [k for k, _ in abi.BFReconStats._fields_][-1] == "renders"


def test_cache_intrinsics_of_the_bundler_options():
    """The float32 scaling CUDACache::CUDACache applies (fx, fy by size ratio, mx, my by (size - 1) ratio)."""
    o = options("medium", 3)
    fx, fy, mx, my = bundler_cache_intrinsics(o)
    assert (o.cache.width, o.cache.height, o.cache.inputWidth, o.cache.inputHeight) == (80, 60, 320, 240)
    assert fx == 288.0 * 0.25 and fy == 288.0 * 0.25
    assert abs(mx - 159.5 * 79 / 319) < 1e-5 and abs(my - 119.5 * 59 / 239) < 1e-5
