"""CPU checks of the matcher's surface-area and dense-verify filters: the ABI surface, argument checks that need no
device, known answers of the NumPy restatement (tests/match_verify_ref.py) and the conditions the GPU tests' fixtures
must meet (no borderline pair for surface area; <= 1 % borderline pixels per verified pair, and every asserted verdict
farther from its thresholds than those pixels could move it)."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
import match_ref as mr
import match_verify_ref as vr
from bundlefusion_amd import abi
from bundlefusion_amd.cache import cache_options
from oracle_lib import cache_store_frame

BF_ERR_ARG = -2
NEW_FUNCTIONS = ["bf_match_filter_surface_area", "bf_match_filter_dense_verify", "bf_match_verify_stats",
                 "bf_match_and_filter", "bf_match_debug_set_filtered"]
KINV = mr.intrinsics_inv()


def test_header_declares_and_library_exports_the_new_entries():
    declared = set(abi.header_functions())
    L = C.CDLL(abi.LIB_PATH)
    for name in NEW_FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name


def test_struct_size_and_defaults():
    L = bfa.lib()
    n = C.c_size_t()
    assert L.bf_abi_struct_size(b"BFMatchVerifyOptions", C.byref(n)) == 0
    assert n.value == C.sizeof(abi.BFMatchVerifyOptions) == 32
    assert L.bf_abi_version() == 4
    from bundlefusion_amd.match import CacheFrames, match_verify_options
    assert bfa.match_verify_options is match_verify_options and bfa.CacheFrames is CacheFrames
    o = bfa.match_verify_options()
    got = [o.surfAreaPcaThresh, o.projCorrDistThres, o.projCorrNormalThres, o.verifySiftErrThresh, o.verifySiftCorrThresh,
           o.sensorDepthMin, o.sensorDepthMax]
    want = [vr.OPTS[k] for k in ("area", "dist", "normal", "err", "corr", "dmin", "dmax")]
    assert np.allclose(got, want, rtol=1e-7)
    text = open(abi.HEADER_PATH.replace("bf.h", "types.h")).read()
    for v in ("[0.032]", "[0.15]", "[0.97]", "[0.075]", "[0.02]", "[0.1]", "[4.0]"):
        assert v in text, v


def test_bad_arguments_without_device():
    L = bfa.lib()
    K = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel().tolist())
    last, u = C.c_uint32(), C.c_uint32
    # a null handle
    assert L.bf_match_filter_surface_area(None, u(0), u(0), None) == BF_ERR_ARG and b"null" in L.bf_last_error()
    assert L.bf_match_filter_dense_verify(None, u(0), u(0), None, u(0), u(80), u(60), K, None) == BF_ERR_ARG
    assert b"null" in L.bf_last_error()
    assert L.bf_match_verify_stats(None, u(0), None, None) == BF_ERR_ARG and b"null" in L.bf_last_error()
    assert L.bf_match_and_filter(None, u(0), u(0), None, u(0), u(0), u(0), None, None, C.byref(last)) == BF_ERR_ARG
    assert b"null" in L.bf_last_error()
    assert L.bf_match_debug_set_filtered(None, u(0), u(0), None) == BF_ERR_ARG
    # thresholds: negative or NaN, checked before anything else
    for field, value in (("surfAreaPcaThresh", -0.1), ("projCorrDistThres", float("nan")), ("projCorrNormalThres", -1.0),
                         ("verifySiftErrThresh", float("nan")), ("verifySiftCorrThresh", -0.02),
                         ("sensorDepthMin", float("inf")), ("sensorDepthMax", -4.0)):
        o = bfa.match_verify_options()
        setattr(o, field, value)
        assert L.bf_match_filter_surface_area(None, u(0), u(0), C.byref(o)) == BF_ERR_ARG
        assert b"threshold" in L.bf_last_error(), field
        assert L.bf_match_filter_dense_verify(None, u(0), u(0), None, u(0), u(80), u(60), K, C.byref(o)) == BF_ERR_ARG
        assert b"threshold" in L.bf_last_error(), field
        assert L.bf_match_and_filter(None, u(0), u(0), None, u(0), u(0), u(0), None, C.byref(o), C.byref(last)) == BF_ERR_ARG
        assert b"threshold" in L.bf_last_error(), field
    o = bfa.match_verify_options(sensor_depth_min=2.0, sensor_depth_max=1.0)
    assert L.bf_match_filter_surface_area(None, u(0), u(0), C.byref(o)) == BF_ERR_ARG and b"sensorDepthMax" in L.bf_last_error()
    # W * H out of range
    for W, H in ((0, 60), (80, 0), (1025, 1024), (1 << 20, 2)):
        assert L.bf_match_filter_dense_verify(None, u(0), u(0), None, u(0), u(W), u(H), K, None) == BF_ERR_ARG
        assert b"W * H" in L.bf_last_error(), (W, H)
    assert L.bf_match_filter_dense_verify(None, u(0), u(0), None, u(0), u(1024), u(1024), K, None) == BF_ERR_ARG
    assert b"null matcher" in L.bf_last_error()  # 2^20 pixels is in range
    assert L.bf_match_filter_dense_verify(None, u(0), u(0), None, u(0), u(80), u(60), None, None) == BF_ERR_ARG
    assert b"intrinsics" in L.bf_last_error()


# ---- known answers of the restatement: surface area ------------------------------------------------------------
def _pair_of_patches(w, h):
    k0, k1 = vr.patch_keys(w, h, 5, 5, (0.1, 0.05, 2.0)), vr.patch_keys(w, h, 5, 5, (-0.1, 0.0, 2.0))
    return np.concatenate([k0, k1]), np.stack([np.arange(25), 25 + np.arange(25)], 1)


def test_ref_small_patch_rejected():
    keys, idx = _pair_of_patches(0.1, 0.1)
    r = vr.surface_area_pair(keys, idx, KINV)
    assert r["reject"] and np.all(r["area"] < 0.032)
    assert np.all(r["area"] <= 2 * 0.1 * 0.1 + 1e-6)  # whatever the box orientation: at most the diagonal squared


def test_ref_large_patch_kept_with_its_area():
    keys, idx = _pair_of_patches(0.3, 0.2)
    r = vr.surface_area_pair(keys, idx, KINV)
    assert not r["reject"] and not r["border"]
    assert np.all(np.abs(r["area"] - 0.06) < 0.01 * 0.06), r["area"]
    assert np.all(np.abs(r["area64"] - 0.06) < 0.01 * 0.06)


def test_ref_collinear_points_have_area_zero():
    k = vr.patch_keys(0, 0, 0, 0, (0.0, 0.0, 2.5), pts=vr.LINE, spin=0.0)
    keys, idx = np.concatenate([k, k]), np.stack([np.arange(9), 9 + np.arange(9)], 1)
    r = vr.surface_area_pair(keys, idx, KINV)
    assert np.all(r["area"] == 0.0) and np.all(r["area64"] == 0.0) and r["reject"]


def test_ref_jacobi_columns_are_the_eigenvectors_and_the_reference_takes_rows():
    """The finding DESIGN.md records: jacobi's v holds the eigenvectors in its columns; eigenSystem hands out its rows."""
    rng = np.random.default_rng(8)
    B = rng.normal(size=(3, 3))
    A = B @ B.T
    ok, d, v = vr.jacobi3(A, np.float64)
    assert ok and np.abs(A @ v - v * d).max() < 1e-12  # A v_k = d_k v_k, column by column
    assert np.abs(A @ v.T - v.T * d).max() > 1e-2      # the rows are not eigenvectors
    ok, ev3, ev = vr.eigen_system3(A, np.float64)
    order = np.argsort(-np.abs(d), kind="stable")
    assert np.array_equal(ev3, d[order]) and np.array_equal(ev, v[order])  # rows, moved along by the sort
    # a tilted plane: rows and columns give different areas, so the sweep order matters for parity
    images, lists = vr.area_fixture()
    keys = np.concatenate([k for k, _ in images])
    a_rows = vr.surface_area_pair(keys, lists[1], KINV)["area64"]
    a_cols = vr.surface_area_pair(keys, lists[1], KINV, rows=False)["area64"]
    assert np.all(np.abs(a_cols - 0.9 * 0.5) < 0.01 * 0.45) and np.all(a_rows < 0.95 * a_cols)


# ---- known answers of the restatement: dense verify --------------------------------------------------------------
def test_ref_plane_under_true_and_wrong_transform():
    W, H = 80, 60
    K = vr.cache_intrinsics(W, H)

    def wall(T):  # a wall at world z = 1.2 that fills the view
        f = vr.render_room(T, W, H, K)  # geometry only: replace by the one plane
        u, v = np.meshgrid(np.arange(W), np.arange(H))
        R, c = T[:3, :3], T[:3, 3]
        dirs = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones((H, W))], -1)
        t = (1.2 - c[2]) / (dirs @ R.T)[..., 2]
        pos = dirs * t[..., None]
        f["depth"] = pos[..., 2].astype(np.float32)
        f["campos"] = np.concatenate([pos, np.ones((H, W, 1))], -1).astype(np.float32)
        n = np.broadcast_to(R.T @ np.array([0.0, 0.0, -1.0]), (H, W, 3))
        f["normals"] = np.concatenate([n, np.zeros((H, W, 1))], -1).astype(np.float32)
        return f

    Ta, Tb = vr.pose(), vr.pose(0.4, 0.0, 0.0, 0.05)
    fa, fb = wall(Ta), wall(Tb)
    T = np.linalg.inv(Tb) @ Ta  # a -> b
    r = vr.dense_pair(fa, fb, T.astype(np.float32), np.linalg.inv(T).astype(np.float32), K)
    # covered fraction: pixels of a whose projection lands in b, and the other way round
    cov = 0.0
    for f, M in ((fa, T), (fb, np.linalg.inv(T))):
        p = f["campos"].reshape(-1, 4).astype(np.float64) @ M.T
        x, y = K[0, 0] * p[:, 0] / p[:, 2] + K[0, 2], K[1, 1] * p[:, 1] / p[:, 2] + K[1, 2]
        cov += np.mean((np.round(x) >= 0) & (np.round(x) < W) & (np.round(y) >= 0) & (np.round(y) < H))
    assert not r["reject"]
    assert abs(float(r["corr"]) - 0.5 * cov) < 0.01, (r["corr"], cov)
    # the residual is at most half a pixel diagonal at 1.2 m, 0.5 sqrt(2) 1.2 / 72.5 = 0.0117 m (a little more where the
    # wall recedes), and a weight there is at least 0.5 ((1 - 0.0117 / 0.15) + (1 - 1.2 / 3.9)) = 0.81
    assert float(r["err"]) < 0.075 / 5
    off = T.copy()
    off[2, 3] += 0.3  # the same frames under a transform 0.3 m off along the wall's normal
    r = vr.dense_pair(fa, fb, off.astype(np.float32), np.linalg.inv(off).astype(np.float32), K)
    assert r["reject"]


def test_ref_invalid_pixels_and_depth_range_do_not_count():
    W, H = 20, 13
    f = vr.render_room(vr.pose(), W, H, holes=vr.dense_holes(W, H))
    I = np.eye(4, dtype=np.float32)
    r = vr.dense_pair(f, f, I, I, vr.cache_intrinsics(W, H))
    good = (~np.isneginf(f["campos"][..., 0])) & (f["depth"] >= 0.1) & (f["depth"] <= 4.0)
    assert 0 < good.sum() < W * H and np.any(f["depth"] > 4.0) and np.any(np.isneginf(f["depth"]))
    assert r["sums"][0, 2] == r["sums"][1, 2] == good.sum() and np.all(r["sums"][:, 0] == 0.0)
    assert float(r["corr"]) == np.float32(good.sum()) / np.float32(W * H) and float(r["err"]) == 0.0


# ---- the fixtures of the GPU tests ---------------------------------------------------------------------------------
def test_area_fixture_conditions():
    images, lists = vr.area_fixture()
    keys = np.concatenate([k for k, _ in images])
    assert [len(l) for l in lists][:2] == [5, 25]
    worst, verdicts = 0.0, []
    for l in lists:
        r = vr.surface_area_pair(keys, l, KINV)
        assert not r["border"]
        for a32, a64 in zip(r["area"], r["area64"]):
            if a64 > 0:
                worst = max(worst, abs(float(a32) - a64) / a64)
        verdicts.append(r["reject"])
    print(f"largest relative float32-vs-float64 area difference: {worst:.3e}")
    assert 0 < worst <= vr.AREA_F32_VS_F64
    assert verdicts == [False, False, True, False, True]
    r = vr.surface_area_pair(keys, lists[3], KINV)
    assert r["area"][0] < 0.032 < r["area"][1]  # one side small, the other large
    assert np.all(vr.surface_area_pair(keys, lists[4], KINV)["area"] == 0.0)


def _check_dense(prev, cur, T, K, o, want_reject):
    r = vr.dense_pair(prev, cur, np.asarray(T, np.float32), np.linalg.inv(np.asarray(T, np.float64)).astype(np.float32), K, o)
    assert sum(r["nborder"]) <= 0.01 * 2 * r["npix"], r["nborder"]
    assert r["flips"] == [0, 0]  # float32 and float64 disagree on borderline pixels only
    assert vr.verdict_is_safe(r, o), (r["err"], r["corr"], r["nborder"])
    assert r["reject"] == want_reject, (r["err"], r["corr"])
    return r


@pytest.mark.parametrize("shape", vr.DENSE_SHAPES)
def test_dense_fixture_conditions(shape):
    W, H = shape
    images, frames, K = vr.dense_images(), vr.dense_frames(W, H), vr.cache_intrinsics(W, H)
    R = mr.run(images, 2, 0, [1] * 4, KINV)
    P = vr.dense_poses()
    for prev, want in ((0, False), (1, False), (3, True)):
        f = R["pairs"][prev]["filt"]
        assert f["count"] >= 5 and not f["border"]
        assert np.abs(f["T"] - np.linalg.inv(P[2]) @ P[prev]).max() < 1e-5  # key points agree with the nominal poses
        assert not vr.surface_area_pair(R["keys"], f["idx"], KINV)["reject"]
        _check_dense(frames[prev], frames[2], f["T"], K, vr.dense_opts(W, H), want)
    assert np.any(frames[0]["depth"] > 4.0) and np.any(np.isneginf(frames[0]["depth"]))  # the band and the holes


def test_skip_fixture_conditions():
    images = vr.skip_images()
    W, H = vr.SKIP_SHAPE
    K = vr.cache_intrinsics(W, H)
    R = mr.run(images, vr.SKIP_CUR, 0, [1] * 6, KINV)
    assert mr.borderline_fraction(images, vr.SKIP_CUR, 0, [1] * 6)[0] == 0
    for prev in (0, vr.SKIP_INVALID, vr.SKIP_ZERO, vr.SKIP_LIVE):
        f = R["pairs"][prev]["filt"]
        assert f["count"] >= 5 and not f["border"]
        s = vr.surface_area_pair(R["keys"], f["idx"], KINV)
        assert not s["reject"] and not s["border"]
    assert R["pairs"][vr.SKIP_EMPTY]["filt"]["count"] == 0
    T = R["pairs"][vr.SKIP_LIVE]["filt"]["T"]
    for wrong, want in ((False, False), (True, True)):
        F = vr.skip_frames(wrong)
        _check_dense(F[vr.SKIP_LIVE], F[vr.SKIP_CUR], T, K, vr.SMALL_OPTS, want)


def real_cache_frames():
    o = cache_options(*vr.REAL_IN, max_frames=4)
    return o, [cache_store_frame(o, d, c) for d, c in vr.real_depths()]


def test_real_cache_fixture_conditions():
    o, frames = real_cache_frames()
    assert (o.width, o.height) == (80, 60)
    images = vr.real_images()
    R = mr.run(images, 2, 0, [1] * 3, KINV)
    for prev, want in ((0, False), (1, True)):
        f = R["pairs"][prev]["filt"]
        assert f["count"] >= 5 and not f["border"]
        assert not vr.surface_area_pair(R["keys"], f["idx"], KINV)["reject"]
        _check_dense(frames[prev], frames[2], f["T"], frames[0]["K"], vr.OPTS, want)
