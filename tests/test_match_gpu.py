"""GPU checks of the sparse matcher (bf_matcher_*) against the NumPy restatement (tests/match_ref.py).

Integer outcomes (dot products, best / second best / argument, the raw list's index pairs, order and count, the
filter's kept set, filterFrames, the EntryJ list) are exact outside the items the restatement marks borderline
(there are none in these fixtures, except possibly <= 0.5 % of the keys at the 1 024-key shape: test_match.py
asserts that on the CPU). Distances are compared with float64 arccos within 4 float32 ulp: ROCm's device-library
documentation installed with the toolchain states no bound for acosf, so the issue's fallback applies.
Transforms use the project's 1 mm / 1e-3 rad.
"""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
import match_ref as mr
from bundlefusion_amd import abi

pytestmark = pytest.mark.gpu

KINV = mr.intrinsics_inv()
NO_FRAME = 0xFFFFFFFF
BF_ERR_ARG, BF_ERR_CAPACITY = -2, -3
ROT_TOL, TRANS_TOL = 1e-3, 1e-3
_worst_ulp = [0.0]


def make_matcher(images, max_images=None, max_keys=None, **kw):
    max_keys = max_keys or max(1, max(len(k) for k, _ in images))
    m = bfa.Matcher(bfa.matcher_options(max_images or len(images), max_keys, KINV, **kw))
    for k, d in images:
        m.add_image(k, d)
    return m


def check_dist(gpu, ref):
    """|acosf - arccos| <= 4 float32 ulp of the value (+ the reference's own rounding)."""
    gpu, ref = np.asarray(gpu, np.float64), np.asarray(ref, np.float64)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    err = np.abs(gpu - ref)
    if len(ref):
        _worst_ulp[0] = max(_worst_ulp[0], float(np.max(err / ulp)))
        print(f"largest acosf difference so far: {_worst_ulp[0]:.3f} float32 ulp")
    assert np.all(err <= 4.0 * ulp + np.spacing(ref)), (err / ulp).max()


def check_raw(m, prev, offs, cur, ref_raw):
    """The raw list of pair (prev, cur) against the restatement's, skipping borderline keys."""
    count, idx, dist = m.raw_matches(prev)
    k = min(ref_raw["count"], mr.MAX_RAW)
    border = ref_raw["border_rows"].any() or ref_raw["border_cols"].any()
    gidx = ref_raw["idx"] + np.array([offs[prev], offs[cur]])
    if not border:
        assert count == ref_raw["count"]
        np.testing.assert_array_equal(idx[:k].astype(np.int64), gidx)
        check_dist(dist[:k], ref_raw["dist"])
    else:  # matches of non-borderline keys appear on both sides, in the same relative order
        assert ref_raw["count"] <= mr.MAX_RAW and count <= mr.MAX_RAW
        br = set(np.flatnonzero(ref_raw["border_rows"]) + offs[prev]), set(np.flatnonzero(ref_raw["border_cols"]) + offs[cur])
        keep = lambda L: [(a, b) for a, b in L if a not in br[0] and b not in br[1]]  # noqa: E731
        assert keep(map(tuple, idx[:count].astype(np.int64))) == keep(map(tuple, gidx))
    np.testing.assert_array_equal(idx[min(count, mr.MAX_RAW):], NO_FRAME)  # padded as the reference pads
    assert np.all(dist[min(count, mr.MAX_RAW):] == 999.0)
    return count, idx, dist


def offsets(images):
    return np.concatenate([[0], np.cumsum([len(k) for k, _ in images])]).astype(np.int64)


# ---- raw matching ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", mr.RAW_SHAPES)
def test_raw_matches_against_restatement(shape):
    images = mr.raw_fixture(shape)
    m = make_matcher(images)
    assert m.num_images() == 2 and m.num_keys(1) == (shape[1], shape[0])
    m.match(1, 0)
    ref = mr.match_pair(images[0][1], images[1][1])
    count, idx, dist = check_raw(m, 0, offsets(images), 1, ref)
    assert count >= 1
    # selected exact dots and the rows' best / second best / argument
    rng = np.random.default_rng(0)
    rows = np.unique(np.concatenate([[0, shape[0] - 1], rng.integers(0, shape[0], 12)]))[:32]
    cols = np.unique(np.concatenate([[0, shape[1] - 1], rng.integers(0, shape[1], 12)]))[:32]
    dots, stats = m.debug_dots(0, 1, rows, cols)
    np.testing.assert_array_equal(dots, ref["D"][np.ix_(rows, cols)])
    rb, rn, ra = ref["rows"]
    np.testing.assert_array_equal(stats, np.stack([rb[rows], rn[rows], ra[rows]], 1))
    m.close()


def test_store_with_empty_and_invalid_images():
    images = mr.store6_fixture()
    offs = offsets(images)
    m = make_matcher(images, max_images=8, max_keys=300)
    assert [m.num_keys(i) for i in range(6)] == [(len(images[i][0]), int(offs[i])) for i in range(6)]
    assert m.get_valid(0) and not m.get_valid(1)
    for i in range(6):
        m.set_valid(i, i != mr.STORE6_INVALID)
    valid = [int(i != mr.STORE6_INVALID) for i in range(6)]
    # curFrame last
    R = mr.run(images, 5, 0, valid, KINV)
    m.match(5, 0)
    for prev in range(5):
        check_raw(m, prev, offs, 5, R["pairs"][prev]["raw"])
    assert m.raw_matches(1)[0] == 0 and m.raw_matches(mr.STORE6_INVALID)[0] == 0
    m.filter(5, 0)
    assert m.filter_frames(5, 0) == R["last"] and m.get_valid(5) == R["valid_cur"]
    # curFrame in the middle, startFrame = cur + 1
    for i in range(6):
        m.set_valid(i, True)
    R = mr.run(images, 2, 3, [1] * 6, KINV)
    m.match(2, 3)
    for prev in (3, 4, 5):
        check_raw(m, prev, offs, 2, R["pairs"][prev]["raw"])
    m.filter(2, 3)
    for prev in (3, 4, 5):
        assert m.filtered_matches(prev)[0] == R["pairs"][prev]["filt"]["count"]
    assert m.filter_frames(2, 3) == R["last"]
    # argument checks that need a handle
    L = bfa.lib()
    assert L.bf_matcher_match(m.h, C.c_uint32(6), C.c_uint32(0)) == BF_ERR_ARG and b"curFrame" in L.bf_last_error()
    assert L.bf_matcher_match(m.h, C.c_uint32(5), C.c_uint32(7)) == BF_ERR_ARG and b"startFrame" in L.bf_last_error()
    d = bfa.DeviceArray((301, 128), np.uint8)
    k = bfa.DeviceArray((301, 4), np.float32)
    assert L.bf_matcher_add_image(m.h, k.ptr, d.ptr, C.c_uint32(301), None) == BF_ERR_ARG
    m.add_image(np.zeros((0, 4), np.float32), np.zeros((0, 128), np.uint8))
    m.add_image(np.zeros((0, 4), np.float32), np.zeros((0, 128), np.uint8))
    assert L.bf_matcher_add_image(m.h, None, None, C.c_uint32(0), None) == BF_ERR_CAPACITY
    m.reset()
    assert m.num_images() == 0
    assert m.add_image(*images[0]) == 0 and m.get_valid(0)
    m.close()


# ---- unsigned range -------------------------------------------------------------------------------------------
def test_unsigned_range_and_clamp():
    rng = np.random.default_rng(4)
    n = 40
    dp = rng.integers(0, 256, (n, 128)).astype(np.uint8)
    dc = rng.integers(0, 256, (37, 128)).astype(np.uint8)
    dp[0] = 255
    dc[0] = 255                      # dot = 128 * 255^2, the largest possible
    dp[1, :] = np.arange(128, 256)   # a 128..255 run
    dc[1, :] = np.arange(255, 127, -1)
    dp[2] = 0
    dc[2] = 0
    dp[3, :64], dp[3, 64:] = 128, 127  # around the signed offset
    dc[3, :64], dc[3, 64:] = 127, 128
    keys = lambda k: np.stack([rng.uniform(0, 639, k), rng.uniform(0, 479, k), np.ones(k), rng.uniform(1, 3, k)], 1).astype(np.float32)  # noqa: E731
    images = [(keys(n), dp), (keys(37), dc)]
    m = make_matcher(images)
    m.match(1, 0)
    ref = mr.match_pair(dp, dc)
    rows, cols = np.arange(32), np.arange(32)
    dots, stats = m.debug_dots(0, 1, rows, cols)
    np.testing.assert_array_equal(dots, ref["D"][:32, :32])
    assert dots[0, 0] == 128 * 255 * 255 and dots[2, 2] == 0
    rb, rn, ra = ref["rows"]
    np.testing.assert_array_equal(stats, np.stack([rb[:32], rn[:32], ra[:32]], 1))
    check_raw(m, 0, offsets(images), 1, ref)
    m.close()
    # a unit-norm-violating descriptor: dot * 2^-18 > 1 clamps to distance 0
    d = np.zeros((2, 128), np.uint8)
    d[0, :8] = 255
    d[1, 64:72] = 200
    images = [(keys(2), d), (keys(2), d[::-1].copy())]
    m = make_matcher(images)
    m.match(1, 0)
    count, idx, dist = m.raw_matches(0)
    assert count == 2 and dist[0] == 0.0 and dist[1] == 0.0
    assert sorted(map(tuple, idx[:2])) == [(0, 3), (1, 2)]
    m.close()


def test_swapping_prev_and_cur_swaps_the_pairs():
    images = mr.raw_fixture((33, 257))
    a = make_matcher(images)
    a.match(1, 0)
    ca, ia, _ = a.raw_matches(0)
    b = make_matcher(images[::-1])
    b.match(1, 0)
    cb, ib, _ = b.raw_matches(0)
    assert ca == cb and ca > 0
    fwd = {(int(p), int(c) - 33) for p, c in ia[:ca]}            # (key of the 33-image, key of the 257-image)
    rev = {(int(c) - 257, int(p)) for p, c in ib[:cb]}
    assert fwd == rev
    # an asymmetric product: rows and columns of selected dots are not interchangeable
    rows, cols = np.arange(5), np.arange(7)
    dots, _ = a.debug_dots(0, 1, rows, cols)
    np.testing.assert_array_equal(dots, mr.dots(images[0][1][:5], images[1][1][:7]))
    a.close()
    b.close()


# ---- cap and determinism --------------------------------------------------------------------------------------
def test_cap_order_and_run_to_run_determinism():
    rng = np.random.default_rng(6)
    _, base = mr.sift_like(rng, 200)
    _, other = mr.sift_like(rng, 60)
    perm = rng.permutation(260)
    dp = np.concatenate([base, other])
    dc = np.concatenate([base, mr.sift_like(rng, 60)[1]])[perm]
    keys = lambda k: np.stack([rng.uniform(0, 639, k), rng.uniform(0, 479, k), np.ones(k), rng.uniform(1, 3, k)], 1).astype(np.float32)  # noqa: E731
    images = [(keys(260), dp), (keys(260), dc)]
    ref = mr.match_pair(dp, dc)
    assert ref["count"] == 200 and not ref["border_rows"].any() and not ref["border_cols"].any()
    m = make_matcher(images)
    m.match(1, 0)
    c1, i1, d1 = check_raw(m, 0, offsets(images), 1, ref)
    assert c1 == 200
    key = [(-int(v), int(b)) for v, (_, b) in zip(ref["dot"], ref["idx"])]
    assert key == sorted(key)  # (dot descending, cur key ascending)
    m.match(1, 0)
    c2, i2, d2 = m.raw_matches(0)
    assert c2 == c1 and i1.tobytes() == i2.tobytes() and d1.tobytes() == d2.tobytes()
    m.close()


# ---- filter ---------------------------------------------------------------------------------------------------
def test_filter_against_restatement():
    images = mr.filter_fixture()
    offs = offsets(images)
    m = make_matcher(images)
    for i in range(6):
        m.set_valid(i, True)
    R = mr.run(images, 5, 0, [1] * 6, KINV)
    m.match(5, 0)
    m.filter(5, 0)
    checked = 0
    for prev in range(5):
        ref = R["pairs"][prev]["filt"]
        if ref["border"]:
            continue
        count, idx, dist = m.filtered_matches(prev)
        assert count == ref["count"]
        assert {tuple(p) for p in idx[:count].astype(np.int64)} == {tuple(p) for p in ref["idx"]}
        np.testing.assert_array_equal(idx[count:], NO_FRAME)
        assert np.all(dist[count:] == 999.0)
        by_pair = {tuple(p): d for p, d in zip(ref["idx"], ref["dist"])}
        check_dist(dist[:count], [by_pair[tuple(p)] for p in idx[:count].astype(np.int64)])
        T, Tinv = m.transforms(prev)
        assert np.linalg.norm(T[:3, 3] - ref["T"][:3, 3]) <= TRANS_TOL and mr.rot_diff(T, ref["T"]) <= ROT_TOL
        assert np.abs(Tinv.astype(np.float64) @ T.astype(np.float64) - np.eye(4)).max() <= 1e-5
        checked += 1
    assert checked >= 5
    assert m.filter_frames(5, 0) == R["last"] == 4 and m.get_valid(5)
    m.close()


def test_filter_rejects_too_few_and_collinear():
    rng = np.random.default_rng(8)
    x = np.linspace(-0.8, 0.8, 12)
    line = np.stack([x, 0.2 * x, 2.5 + 0.1 * x], 1)
    T1 = np.eye(4)
    T1[0, 3] = 0.05
    few = np.stack([rng.uniform(-0.5, 0.5, 4), rng.uniform(-0.4, 0.4, 4), rng.uniform(2, 3, 4)], 1)

    def keys_of(pts, T):
        u, v, z, inside = mr.project(T, pts)
        assert inside.all()
        return np.stack([u, v, np.ones(len(u)), z], 1).astype(np.float32)

    _, d_line = mr.sift_like(rng, 12)
    _, d_few = mr.sift_like(rng, 4)
    images = [(keys_of(line, np.eye(4)), d_line), (keys_of(few, np.eye(4)), d_few),
              (np.concatenate([keys_of(line, T1), keys_of(few, T1)]), np.concatenate([d_line, d_few]))]
    R = mr.run(images, 2, 0, [1, 1, 1], KINV)
    assert R["pairs"][0]["raw"]["count"] == 12 and R["pairs"][1]["raw"]["count"] == 4
    assert R["pairs"][0]["filt"]["count"] == 0 and R["pairs"][1]["filt"]["count"] == 0
    m = make_matcher(images)
    m.set_valid(1, True)
    m.match(2, 0)
    m.filter(2, 0)
    assert m.raw_matches(0)[0] == 12 and m.raw_matches(1)[0] == 4
    assert m.filtered_matches(0)[0] == 0 and m.filtered_matches(1)[0] == 0
    assert m.filter_frames(2, 0) == NO_FRAME and not m.get_valid(2)
    out, total = m.add_to_residuals(2, 0, 16)
    assert len(out) == 0 and total == 0
    m.close()


# ---- filter_frames / add_to_residuals -----------------------------------------------------------------------
def test_add_to_residuals_bit_exact_and_ordered():
    images = mr.filter_fixture()
    m = make_matcher(images)
    for i in range(6):
        m.set_valid(i, True)
    m.match(5, 0)
    m.filter(5, 0)
    filt = [m.filtered_matches(prev) for prev in range(5)]
    expect_idx = np.concatenate([idx[:count] for count, idx, _ in filt]).astype(np.int64)
    expect_prev = np.concatenate([np.full(count, prev) for prev, (count, _, _) in enumerate(filt)])
    total_expect = len(expect_idx)
    out, total, kidx = m.add_to_residuals(5, 0, 200, want_key_indices=True)
    assert total == total_expect == len(out)
    np.testing.assert_array_equal(kidx.astype(np.int64), expect_idx)
    np.testing.assert_array_equal(out["i"], expect_prev)
    assert np.all(out["j"] == 5)
    all_keys = np.concatenate([k for k, _ in images])
    pos = mr.key_points32(all_keys, KINV)
    assert out["pos_i"].tobytes() == pos[expect_idx[:, 0]].tobytes()
    assert out["pos_j"].tobytes() == pos[expect_idx[:, 1]].tobytes()
    cut, total2 = m.add_to_residuals(5, 0, 30)  # cap truncates, the total is still reported
    assert total2 == total_expect and len(cut) == 30 and cut.tobytes() == out[:30].tobytes()
    m.close()


# ---- end to end, pose-free ------------------------------------------------------------------------------------
def test_pose_free_trajectory_through_the_solver():
    from ba_problem import pose_errors
    from bundlefusion_amd.solver import GLOBAL_WEIGHTS_SPARSE_ONLY, SolverBundling
    from oracle_ba import matrix_to_pose
    K = 6
    gt = np.stack([bfa.synth_pose(10 * k) for k in range(K)]).astype(np.float32)
    images = mr.e2e_fixture([g.astype(np.float64) for g in gt])
    m = bfa.Matcher(bfa.matcher_options(K, mr.E2E_KEYS, KINV))
    m.add_image(*images[0])
    poses = [gt[0].astype(np.float64)]  # the gauge: frame 0
    corr = []
    for f in range(1, K):
        m.add_image(*images[f])
        assert m.match_and_filter(f) != NO_FRAME and m.get_valid(f)
        e, total = m.add_to_residuals(f, 0, 25 * K)
        assert total == len(e) > 0
        corr.append(e)
        _, Tinv = m.transforms(f - 1)  # camera f in camera f - 1: the front end's Tinc
        rel = np.linalg.inv(gt[f - 1].astype(np.float64)) @ gt[f].astype(np.float64)
        assert np.linalg.norm(Tinv[:3, 3] - rel[:3, 3]) <= TRANS_TOL and mr.rot_diff(Tinv, rel) <= ROT_TOL
        poses.append(poses[-1] @ Tinv.astype(np.float64))
    m.close()
    corr = np.concatenate(corr)
    rot, trans = np.zeros((K, 3), np.float32), np.zeros((K, 3), np.float32)
    for k in range(K):
        rot[k], trans[k] = matrix_to_pose(poses[k].astype(np.float32))
    S = SolverBundling(K, max(K * 4000, len(corr)))
    d_corr = bfa.DeviceArray.from_host(corr)
    d_valid = bfa.DeviceArray.from_host(np.ones(K, np.int32))
    d_rot, d_trans = bfa.DeviceArray.from_host(rot), bfa.DeviceArray.from_host(trans)
    S.solve(d_corr, len(corr), d_valid, K, 3, 150, GLOBAL_WEIGHTS_SPARSE_ONLY["sparse"], rot=d_rot, trans=d_trans)
    res = S.result()
    assert res["error"] == 0
    er, et = pose_errors(d_rot.download(), d_trans.download(), gt)
    S.close()
    assert er <= ROT_TOL and et <= TRANS_TOL, (er, et)
