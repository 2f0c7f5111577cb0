"""CPU checks of the sparse matcher (bf_matcher_*): the ABI surface, argument checks that need no device, known
answers of the NumPy restatement (tests/match_ref.py) and the borderline conditions of the GPU tests' fixtures."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
import match_ref as mr
from bundlefusion_amd import abi

BF_ERR_ARG = -2
MATCHER_FUNCTIONS = [
    "bf_matcher_create", "bf_matcher_destroy", "bf_matcher_reset", "bf_matcher_add_image", "bf_matcher_num_images",
    "bf_matcher_num_keys", "bf_matcher_set_valid", "bf_matcher_get_valid", "bf_matcher_match", "bf_matcher_filter",
    "bf_matcher_filter_frames", "bf_matcher_add_to_residuals", "bf_matcher_raw_matches", "bf_matcher_filtered_matches",
    "bf_matcher_transforms", "bf_matcher_debug_dots", "bf_matcher_synchronize", "bf_matcher_timer_start",
    "bf_matcher_timer_stop"]
KINV = mr.intrinsics_inv()


def test_header_declares_and_library_exports_the_matcher():
    declared = set(abi.header_functions())
    L = C.CDLL(abi.LIB_PATH)
    for name in MATCHER_FUNCTIONS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert sorted(n for n in declared if n.startswith("bf_matcher_")) == sorted(MATCHER_FUNCTIONS)


def test_struct_sizes():
    L = bfa.lib()
    assert C.sizeof(abi.BFSiftKeyPoint) == 16 and abi.SIFT_KEYPOINT_DTYPE.itemsize == 16
    for cls in (abi.BFSiftKeyPoint, abi.BFMatcherOptions):
        n = C.c_size_t()
        assert L.bf_abi_struct_size(cls.__name__.encode(), C.byref(n)) == 0
        assert n.value == C.sizeof(cls), cls.__name__
    assert L.bf_abi_version() == 4
    from bundlefusion_amd.match import Matcher, matcher_options
    assert bfa.Matcher is Matcher and bfa.matcher_options is matcher_options


def _create(**fields):
    o = bfa.matcher_options(4, 64, KINV)
    for k, v in fields.items():
        setattr(o, k, v)
    h = C.c_void_p()
    return bfa.lib().bf_matcher_create(C.byref(o), C.byref(h)), bfa.lib().bf_last_error()


def test_bad_arguments_without_device():
    L = bfa.lib()
    h = C.c_void_p()
    assert L.bf_matcher_create(None, C.byref(h)) == BF_ERR_ARG and b"null" in L.bf_last_error()
    o = bfa.matcher_options(4, 64, KINV)
    assert L.bf_matcher_create(C.byref(o), None) == BF_ERR_ARG
    for fields, msg in (({"maxImages": 0}, b"capacity"), ({"maxKeysPerImage": 0}, b"capacity"),
                        ({"maxKeysPerImage": 1025}, b"1024"), ({"matchThresh": float("nan")}, b"non-finite"),
                        ({"ratioMax": float("inf")}, b"non-finite"), ({"maxKabschRes2": -1.0}, b"negative")):
        rc, err = _create(**fields)
        assert rc == BF_ERR_ARG and msg in err, (fields, rc, err)
    o = bfa.matcher_options(4, 64, KINV)
    o.intrinsicsInv[5] = float("nan")
    assert L.bf_matcher_create(C.byref(o), C.byref(h)) == BF_ERR_ARG and b"intrinsicsInv" in L.bf_last_error()
    n = C.c_uint32()
    assert L.bf_matcher_add_image(None, None, None, C.c_uint32(0), C.byref(n)) == BF_ERR_ARG and b"null" in L.bf_last_error()
    assert L.bf_matcher_match(None, C.c_uint32(0), C.c_uint32(0)) == BF_ERR_ARG and b"null" in L.bf_last_error()
    assert L.bf_matcher_filter(None, C.c_uint32(0), C.c_uint32(0)) == BF_ERR_ARG
    assert L.bf_matcher_filter_frames(None, C.c_uint32(0), C.c_uint32(0), C.byref(n)) == BF_ERR_ARG
    assert L.bf_matcher_add_to_residuals(None, C.c_uint32(0), C.c_uint32(0), None, None, C.c_uint32(0), C.byref(n), None) == BF_ERR_ARG
    assert L.bf_matcher_raw_matches(None, C.c_uint32(0), None, None, None) == BF_ERR_ARG
    assert L.bf_matcher_reset(None) == BF_ERR_ARG and L.bf_matcher_synchronize(None) == BF_ERR_ARG
    assert L.bf_matcher_destroy(None) == 0


# ---- known answers of the restatement -----------------------------------------------------------------------
def _grid_keys(n, rng):
    """n points in front of the identity camera whose projections are at least 12 pixels apart."""
    pts, uv = [], []
    while len(pts) < n:
        z = rng.uniform(1.8, 3.4)
        p = np.array([z * rng.uniform(-0.4, 0.4), z * rng.uniform(-0.3, 0.3), z])
        q = np.array([mr.FX * p[0] / z, mr.FY * p[1] / z])
        if all(np.linalg.norm(q - o) >= 12.0 for o in uv):
            pts.append(p)
            uv.append(q)
    return np.array(pts)


def _keys_of(pts, T):
    u, v, z, inside = mr.project(T, pts)
    assert inside.all()
    return np.stack([u, v, np.ones(len(u)), z], 1).astype(np.float32)


def test_ref_same_key_set_permuted():
    rng = np.random.default_rng(0)
    pts = _grid_keys(40, rng)
    keys = _keys_of(pts, np.eye(4))
    _, descs = mr.sift_like(rng, 40)
    for d in descs:  # quantisation leaves |d|^2 a little under 2^18: raise entries until the self dot clamps
        k = 0
        while (d.astype(np.int64) ** 2).sum() < 2 ** 18:
            d[k % 128] = min(int(d[k % 128]) + 1, 255)
            k += 1
    perm = rng.permutation(40)
    images = [(keys, descs), (keys[perm], descs[perm])]
    R = mr.run(images, 1, 0, [1, 1], KINV)
    raw, filt = R["pairs"][0]["raw"], R["pairs"][0]["filt"]
    assert raw["count"] == 40
    assert np.all(perm[raw["idx"][:, 1]] == raw["idx"][:, 0])  # every key matched to itself
    assert np.all(raw["dist"] == 0.0)
    assert filt["count"] > 5 and not filt["border"]
    assert np.abs(filt["T"] - np.eye(4)).max() < 1e-6
    assert R["last"] == 0 and R["valid_cur"]


def test_ref_distance_zero_for_saturated_descriptor():
    d = np.zeros((1, 128), np.uint8)
    d[0, :8] = 255  # dot = 8 * 255^2 > 2^18: clamps
    r = mr.match_pair(d, d)
    assert r["count"] == 1 and r["dist"][0] == 0.0


def test_ref_translation_recovered_and_wrong_matches_removed():
    rng = np.random.default_rng(1)
    pts = _grid_keys(30, rng)
    T1 = np.eye(4)
    T1[0, 3] = 0.05  # camera 1 is 5 cm to the right of camera 0
    k0, k1 = _keys_of(pts, np.eye(4)), _keys_of(pts, T1)
    wrong = [20, 24, 27]
    alt = pts.copy()
    alt[wrong] += [0.3, -0.25, 0.3]
    k1[wrong] = _keys_of(alt[wrong], T1)
    keys = np.concatenate([k0, k1])
    idx = np.stack([np.arange(30), 30 + np.arange(30)], 1)
    out = mr.filter_pair(keys, idx, np.linspace(0.1, 0.3, 30), KINV)
    kept = set(map(tuple, out["idx"]))
    assert out["count"] >= 5 and not out["border"]
    assert not any((w, 30 + w) in kept for w in wrong)
    expect = np.linalg.inv(T1)  # prev -> cur: x_1 = x_0 - 0.05
    assert np.abs(out["T"][:3, 3] - expect[:3, 3]).max() < 1e-5 and mr.rot_diff(out["T"], expect) < 1e-5


def test_ref_collinear_rejected():
    x = np.linspace(-0.8, 0.8, 12)
    pts = np.stack([x, 0.2 * x, 2.5 + 0.1 * x], 1)
    T1 = np.eye(4)
    T1[0, 3] = 0.05
    keys = np.concatenate([_keys_of(pts, np.eye(4)), _keys_of(pts, T1)])
    idx = np.stack([np.arange(12), 12 + np.arange(12)], 1)
    out = mr.filter_pair(keys, idx, np.linspace(0.1, 0.3, 12), KINV)
    assert out["count"] == 0


def test_ref_three_pixels_apart_keeps_the_first():
    rng = np.random.default_rng(2)
    pts = _grid_keys(12, rng)
    k0 = _keys_of(pts, np.eye(4))
    k0[1, :2] = k0[0, :2] + [3.0, 0.0]  # key 1 sits 3 pixels from key 0 in image 0
    k0[1, 3] = k0[0, 3]
    keys = np.concatenate([k0, k0])
    idx = np.stack([np.arange(12), 12 + np.arange(12)], 1)
    out = mr.filter_pair(keys, idx, np.linspace(0.1, 0.3, 12), KINV)
    kept = set(map(tuple, out["idx"]))
    assert (0, 12) in kept and (1, 13) not in kept and out["count"] == 11


def test_ref_best_next_arg_ties_and_zero():
    D = np.array([[5, 9, 9, 1], [0, 0, 0, 0], [7, 3, 2, 7]], np.int64)
    best, nxt, arg = mr.best_next_arg(D)
    assert list(best) == [9, 0, 7] and list(nxt) == [9, 0, 7] and list(arg) == [1, -1, 0]


# ---- the fixtures of the GPU tests ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mr.RAW_SHAPES)
def test_raw_fixtures_have_no_borderline_keys(shape):
    images = mr.raw_fixture(shape)
    b, t = mr.borderline_fraction(images, 1, 0, [1, 1])
    assert t == sum(shape)
    if shape == (1024, 1000):
        assert b <= 0.005 * t, (b, t)
    else:
        assert b == 0
    r = mr.match_pair(images[0][1], images[1][1])
    assert r["count"] >= 1
    if shape == (1024, 1000):
        assert r["count"] > 128  # the cap is exercised


def test_store_and_filter_fixtures_have_no_borderline_items():
    images = mr.store6_fixture()
    valid = [1] * 6
    valid[mr.STORE6_INVALID] = 0
    for cur, start, v in ((5, 0, valid), (2, 3, [1] * 6)):
        assert mr.borderline_fraction(images, cur, start, v)[0] == 0
        R = mr.run(images, cur, start, v, KINV)
        assert not any(p["filt"]["border"] for p in R["pairs"].values())
    images = mr.filter_fixture()
    assert mr.borderline_fraction(images, 5, 0, [1] * 6)[0] == 0
    R = mr.run(images, 5, 0, [1] * 6, KINV)
    assert len(R["pairs"]) == 5 and not any(p["filt"]["border"] for p in R["pairs"].values())
    assert len({p["raw"]["count"] for p in R["pairs"].values()}) >= 4  # differing overlap
    assert all(p["filt"]["count"] >= 5 for p in R["pairs"].values())


def test_e2e_fixture_links_consecutive_frames():
    poses = [bfa.synth_pose(10 * k).astype(np.float64) for k in range(6)]
    images = mr.e2e_fixture(poses)
    for f in range(1, 6):
        assert mr.borderline_fraction(images[:f + 1], f, 0, [1] * (f + 1))[0] == 0
        R = mr.run(images[:f + 1], f, 0, [1] * (f + 1), KINV)
        p = R["pairs"][f - 1]
        assert p["filt"]["count"] >= 5 and not p["filt"]["border"]
        rel = np.linalg.inv(poses[f]) @ poses[f - 1]  # prev -> cur
        assert np.abs(p["filt"]["T"][:3, 3] - rel[:3, 3]).max() < 1e-4 and mr.rot_diff(p["filt"]["T"], rel) < 1e-4
