"""CPU checks of the bundler (bf_bundler_*): the ABI surface, every host rejection (none needs a device), and the NumPy
restatement (tests/bundler_ref.py): its closing step, its chain over the GPU tests' fixture against the ground truth, and
the float32-against-float64 spread of the three transform cases, the basis of the GPU bar for the third."""
import ctypes as C

import numpy as np

import bundlefusion_amd as bfa
import bundler_ref as B
import sift_ref as R
from bundlefusion_amd import abi

BF_ERR_ARG = -2
BUNDLER_FUNCTIONS = [
    "bf_bundler_create", "bf_bundler_destroy", "bf_bundler_reset", "bf_bundler_synchronize", "bf_bundler_timer_start",
    "bf_bundler_timer_stop", "bf_bundler_process_frame", "bf_bundler_set_complete_trajectory", "bf_bundler_submap",
    "bf_bundler_fuse_submap", "bf_bundler_invalid_submap", "bf_bundler_global", "bf_bundler_matcher", "bf_bundler_cache",
    "bf_bundler_sift", "bf_bundler_intensity", "bf_bundler_stats", "bf_bundler_debug_reclose"]
# The third case's float32-against-float64 spread measured by test_three_cases_agree_with_float64 (largest element
# difference over 200 random rigid chains): 4.13e-07. The GPU bar (tests/test_bundler_gpu.py) is 10 x the value measured
# in the same run, not this constant.
CASE3_SPREAD_SEEN = 4.13e-07


def options(name="medium", submap_size=3, max_keyframes=4, **kw):
    f = R.FIXTURES[name]
    fx, fy, cx, cy = R.camera(f["w"], f["h"])
    kinv = R.intrinsics_inv(f["w"], f["h"])
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    sx, sy = f["dw"] / f["w"], f["dh"] / f["h"]
    return bfa.bundler_options(
        bfa.sift_options(f["w"], f["h"], f["dw"], f["dh"], **f["opts"]), bfa.matcher_options(0, 1024, kinv),
        bfa.matcher_options(0, 1024, kinv), bfa.cache.cache_options(f["dw"], f["dh"], fx * sx, fy * sy, cx * sx, cy * sy, 0),
        K, submap_size=submap_size, max_keyframes=max_keyframes, **kw)


def test_header_declares_and_library_exports_the_bundler():
    declared = set(abi.header_functions())
    L = C.CDLL(abi.LIB_PATH)
    for name in BUNDLER_FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert sorted(n for n in declared if n.startswith("bf_bundler_")) == sorted(BUNDLER_FUNCTIONS)


def test_struct_sizes_and_abi_version():
    L = bfa.lib()
    for cls in (abi.BFBundlerOptions, abi.BFBundlerFrame, abi.BFBundlerSubmap, abi.BFBundlerKeyframe, abi.BFBundlerStats,
                abi.BFSiftOptions):
        n = C.c_size_t()
        assert L.bf_abi_struct_size(cls.__name__.encode(), C.byref(n)) == 0
        assert n.value == C.sizeof(cls), cls.__name__
    assert C.sizeof(abi.BFSiftOptions) == 48 and C.sizeof(abi.BFBundlerFrame) == 168
    assert L.bf_abi_version() == 4
    from bundlefusion_amd.bundler import Bundler, bundler_options
    assert bfa.Bundler is Bundler and bfa.bundler_options is bundler_options


def _create(o):
    h = C.c_void_p()
    rc = bfa.lib().bf_bundler_create(C.byref(o), C.byref(h))
    assert not h.value
    return rc, bfa.lib().bf_last_error()


def test_every_rejection_is_on_the_host():
    """No device is needed: each call fails before any device work."""
    L = bfa.lib()
    h = C.c_void_p()
    assert L.bf_bundler_create(None, C.byref(h)) == BF_ERR_ARG and b"null" in L.bf_last_error()
    assert L.bf_bundler_create(C.byref(options()), None) == BF_ERR_ARG

    def with_(path, value, **kw):
        o = options(**kw)
        obj = o
        for p in path[:-1]:
            obj = getattr(obj, p)
        if isinstance(path[-1], tuple):
            getattr(obj, path[-1][0])[path[-1][1]] = value
        else:
            setattr(obj, path[-1], value)
        return o

    cases = [
        (with_(("submapSize",), 0), b"submapSize"), (with_(("maxKeyframes",), 1), b"maxKeyframes"),
        (with_(("sift", "width"), 16), b"sift image size"), (with_(("sift", "maxKeys"), 1025), b"1024"),
        (with_(("cache", "width"), 1), b"cache and input sizes"), (with_(("cache", "width"), 20000), b"2^20"),
        (with_(("cache", "depthSigmaD"), 9.0), b"radius"), (with_(("cache", "inputWidth"), 100), b"depth size"),
        (with_(("local", "maxKeysPerImage"), 0), b"capacity"), (with_(("global_", "ratioMax"), float("nan")), b"non-finite"),
        (with_(("local", "maxImages"), 7), b"local.maxImages"), (with_(("global_", "maxImages"), 7), b"global.maxImages"),
        (with_(("verify", "sensorDepthMin"), 5.0), b"sensorDepthMax"), (with_(("maxLocalCorr",), (1 << 28) + 1), b"2^28"),
    ]
    o = options()
    o.colorIntrinsics[5] = float("inf")
    cases.append((o, b"colorIntrinsics"))
    for sigma in (0.0, -1.0, float("nan"), float("inf"), 3.6):
        cases.append((options(filter_intensity=True, intensity_sigma_d=sigma), b"intensitySigmaD"))
    for o, msg in cases:
        rc, err = _create(o)
        assert rc == BF_ERR_ARG and msg in err, (rc, err, msg)
    r, s, k, st = abi.BFBundlerFrame(), abi.BFBundlerSubmap(), abi.BFBundlerKeyframe(), abi.BFBundlerStats()
    u, p = C.c_uint32(), C.c_void_p()
    for rc in (L.bf_bundler_process_frame(None, None, u, u, None, None, C.byref(r)), L.bf_bundler_submap(None, C.byref(s)),
               L.bf_bundler_fuse_submap(None, None, C.byref(k)), L.bf_bundler_invalid_submap(None), L.bf_bundler_reset(None),
               L.bf_bundler_global(None, None, None, None, None, None), L.bf_bundler_matcher(None, u, C.byref(p)),
               L.bf_bundler_cache(None, u, C.byref(p)), L.bf_bundler_sift(None, C.byref(p)), L.bf_bundler_stats(None, C.byref(st)),
               L.bf_bundler_set_complete_trajectory(None, None, u, u), L.bf_bundler_synchronize(None),
               L.bf_bundler_intensity(None, C.byref(p)), L.bf_bundler_debug_reclose(None, C.byref(r)),
               L.bf_bundler_timer_start(None, None), L.bf_bundler_timer_stop(None, None, None)):
        assert rc == BF_ERR_ARG and b"null" in L.bf_last_error()
    assert L.bf_bundler_destroy(None) == 0


def test_gauss_restatement():
    """Known answers: a constant image stays constant to an ulp of the normalisation, the weights are gaussD's, the window
    clips at the borders (radius 4 and 2)."""
    w = B.gauss_weights(2.0)
    assert w.shape == (9, 9) and w[4, 4] == 1.0 and w[4, 5] == np.float32(np.exp(-np.float64(np.float32(1.0) / np.float32(8.0))))
    assert B.gauss_weights(0.7).shape == (5, 5)
    img = np.full((12, 17), 0.375, np.float32)
    assert np.abs(B.gauss_intensity(img, 2.0) - 0.375).max() <= 1e-6
    rng = np.random.default_rng(1)
    img = rng.uniform(0, 1, (9, 11)).astype(np.float32)
    out = B.gauss_intensity(img, 0.7)
    wt = B.gauss_weights(0.7).astype(np.float64)
    assert abs(out[0, 0] - (wt[2:, 2:] * img[:3, :3]).sum() / wt[2:, 2:].sum()) <= 1e-6  # the corner sees a 3 x 3 window
    assert abs(out[4, 5] - (wt * img[2:7, 3:8]).sum() / wt.sum()) <= 1e-6


def test_close_restatement_order_and_capacity():
    """Counts 0 / 25 / 0 / 1 before cur = 4: the bases, the last matched frame and the capacity rule."""
    c = B.close_frame([0, 25, 0, 1, 0], [1, 1, 1, 1, 0], 4, 0, 10, 100)
    assert c["valid"] and c["last"] == 3 and c["added"] == 26 and c["total"] == 36
    assert c["bases"] == {0: 0, 1: 0, 2: 25, 3: 25}
    c = B.close_frame([0, 25, 0, 1, 0], [1, 1, 1, 0, 0], 4, 0, 10, 100)
    assert c["last"] == 1  # image 3 is invalid: the highest VALID prev with a count
    c = B.close_frame([0, 25, 0, 1, 0], [1, 1, 1, 1, 0], 4, 0, 10, 35)  # one below the need
    assert c["overflow"] and not c["valid"] and c["added"] == 0 and c["total"] == 10 and c["last"] == B.NONE
    c = B.close_frame([0, 0, 0, 0, 0], [1, 1, 1, 1, 0], 4, 0, 10, 100)
    assert not c["valid"] and not c["overflow"] and c["total"] == 10
    book = B.Book(3)
    seen = [book.add() for _ in range(4)]
    assert seen[3] == (3, 3, 0, True) and seen[1] == (1, 1, 0, False)
    for _ in range(3):
        book.decide(False)
    book.close()
    assert book.closed["frames"] == [0, 1, 2, 3] and not book.closed["is_valid"] and book.images == [3] and book.valid == [1]
    assert book.add() == (4, 1, 1, False)


def test_three_cases_agree_with_float64():
    """The chain step in float32 against its float64 evaluation: cases one and two are one product each (a few ulp of
    the entries), case three is four products and an inverse. Prints the spread the GPU bar is built on."""
    spread = B.case_spread()
    print(f"case three: float32 against float64 spread {spread:.3g} (seen {CASE3_SPREAD_SEEN:.3g}); GPU bar 10 x = {10 * spread:.3g}")
    assert 0.0 < spread <= 5e-6  # four float32 products of entries of size <= 4: a few 1e-7 each
    sift = {k: B.mat_mul(np.eye(4), R.pose(k).astype(np.float32)) for k in range(6)}
    complete = {k: B.mat_mul(R.pose(7).astype(np.float32), sift[k]) for k in range(6)}
    tinv = [(np.linalg.inv(R.pose(4)) @ R.pose(5)).astype(np.float32)] * 2
    for lv, case in ((0, 1), (5, 2), (2, 3)):
        s32, t32 = B.sift_step(sift, 5, 1, [25, 0], tinv, True, complete, lv)
        s64, t64 = B.sift_step(sift, 5, 1, [25, 0], tinv, True, complete, lv, B.F64)
        assert np.abs(s32 - s64).max() <= 1e-6 and np.abs(t32 - t64).max() <= (1e-6 if case < 3 else 10 * spread)
        if case == 1:
            assert t32.tobytes() == s32.tobytes()
        if case == 3:  # offset = inv(sift[2]) sift[4]; complete[2] offset = pose(7) sift[4]: the same pose as case two's
            _, t2 = B.sift_step(sift, 5, 1, [25, 0], tinv, True, complete, 5)
            assert np.abs(t32 - t2).max() <= 10 * spread
    s, t = B.sift_step(sift, 5, 1, [0, 0], tinv, False)
    assert s.tobytes() == sift[4].tobytes() and np.all(np.isneginf(t))


def test_restatement_chain_meets_the_ground_truth():
    """medium scene, pose(0..6), submapSize 3: two submaps of four frames sharing frame 3; every local pair keeps 25
    matches, every frame is valid; the consecutive sift poses against the ground truth."""
    ch = B.chain_reference("medium", 7, 3)
    for k in range(1, 7):
        print(f"frame {k}: counts {ch['counts'][k]}, translation error {ch['t_err'][k - 1]:.5f} m, "
              f"rotation error {ch['r_err'][k - 1]:.6f} rad")
    assert all(ch["valid"]) and all(c == 25 for k in range(1, 7) for c in ch["counts"][k].values())
    assert sum(len(ch["counts"][k]) for k in range(1, 7)) == 12
    assert max(ch["t_err"]) <= 0.0019 + 5e-5 and max(ch["r_err"]) <= 0.0028 + 5e-5
    assert [s["frames"] for s in ch["submaps"]] == [[0, 1, 2, 3], [3, 4, 5, 6]]
    assert all(s["is_valid"] and len(s["entries"]) == 150 for s in ch["submaps"])
