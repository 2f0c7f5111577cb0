"""GPU checks of the matcher's surface-area and dense-verify filters against the NumPy restatement
(tests/match_verify_ref.py). The GPU's own filtered lists and bf_matcher_transforms output are fed to the restatement,
so these tests isolate the two new kernels.

Tolerances. Areas: relative 10 x the float32-versus-float64 difference of the restatement on these fixtures
(match_verify_ref.AREA_TOL; test_match_verify.py measures the difference on the CPU). Dense verify: numCorr per
direction equals the restatement's up to its borderline-pixel count; sumResidual and sumWeight within relative 1e-3
(the worst case of a float32 sum of <= 9 600 non-negative terms is (n - 1) 2^-24 = 5.7e-4) plus (borderline count) x
distThresh. Verdicts are equal; test_match_verify.py asserts on the CPU that no fixture verdict is within reach of its
borderline items."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
import match_ref as mr
import match_verify_ref as vr
from bundlefusion_amd.cache import CUDACache, cache_options

pytestmark = pytest.mark.gpu

KINV = mr.intrinsics_inv()
NO_FRAME = 0xFFFFFFFF
BF_ERR_ARG = -2


def make_matcher(images, max_images=None, max_keys=None):
    max_keys = max_keys or max(1, max(len(k) for k, _ in images))
    m = bfa.Matcher(bfa.matcher_options(max_images or len(images), max_keys, KINV))
    for k, d in images:
        m.add_image(k, d)
    return m


def verify_options(o):
    return bfa.match_verify_options(o["area"], o["dist"], o["normal"], o["err"], o["corr"], o["dmin"], o["dmax"])


def all_keys(images):
    return np.concatenate([np.asarray(k, np.float32).reshape(-1, 4) for k, _ in images])


def check_dense_pair(m, prev, frames, cur, K, o):
    """verify_stats of pair prev against the restatement fed with the GPU's transforms; returns the restatement."""
    T, Ti = m.transforms(prev)
    ref = vr.dense_pair(frames[prev], frames[cur], T, Ti, K, o)
    _, sums = m.verify_stats(prev)
    print(f"pair {prev}: gpu {sums.tolist()} ref {ref['sums'].tolist()} borderline {ref['nborder']}")
    for k in range(2):
        nb = ref["nborder"][k]
        assert abs(float(sums[k, 2]) - float(ref["sums"][k, 2])) <= nb, (k, sums, ref["sums"], nb)
        for q in (0, 1):
            tol = 1e-3 * abs(float(ref["sums"][k, q])) + nb * o["dist"]
            assert abs(float(sums[k, q]) - float(ref["sums"][k, q])) <= tol, (k, q, sums, ref["sums"], nb)
    return ref


# ---- surface area ---------------------------------------------------------------------------------------------------
def test_surface_area_against_restatement():
    images, lists = vr.area_fixture()
    keys = all_keys(images)
    m = make_matcher(images)
    for i in range(6):
        m.set_valid(i, True)
    for prev, l in enumerate(lists):
        m.debug_set_filtered(prev, l)
        assert m.filtered_matches(prev)[0] == len(l)
    m.filter_surface_area(5, 0)
    verdicts = []
    for prev, l in enumerate(lists):
        ref = vr.surface_area_pair(keys, l, KINV)
        area, sums = m.verify_stats(prev)
        print(f"pair {prev}: gpu {area.tolist()} ref {ref['area'].tolist()} float64 {ref['area64'].tolist()}")
        assert np.all(np.abs(area.astype(np.float64) - ref["area"]) <= vr.AREA_TOL * np.abs(ref["area"])), (prev, area, ref["area"])
        assert np.all(np.isnan(sums))  # dense verify has not run
        count, idx, _ = m.filtered_matches(prev)
        assert (count == 0) == ref["reject"], prev
        np.testing.assert_array_equal(idx[:len(l)].astype(np.int64), l)  # the list stays
        verdicts.append(count == 0)
    assert verdicts == [False, False, True, False, True]
    assert np.all(np.isnan(m.verify_stats(5)[0]))  # prev == cur
    # a higher threshold through the options rejects the 5-match pair too
    for prev, l in enumerate(lists):
        m.debug_set_filtered(prev, l)
    m.filter_surface_area(5, 0, bfa.match_verify_options(surf_area_pca_thresh=0.12))
    assert [m.filtered_matches(p)[0] == 0 for p in range(5)] == [True, False, True, False, True]
    m.close()


# ---- dense verify -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", vr.DENSE_SHAPES)
def test_dense_verify_against_restatement(shape):
    W, H = shape
    images, frames, K, o = vr.dense_images(), vr.dense_frames(W, H), vr.cache_intrinsics(W, H), vr.dense_opts(W, H)
    m = make_matcher(images)
    for i in range(4):
        m.set_valid(i, True)
    m.match(2, 0)
    m.filter(2, 0)
    before = {p: m.filtered_matches(p) for p in (0, 1, 3)}
    assert all(before[p][0] >= 5 for p in before)
    cache = bfa.CacheFrames.from_host(frames, K)
    m.filter_dense_verify(2, 0, cache, verify_options(o))
    for prev, want in ((0, False), (1, False), (3, True)):
        ref = check_dense_pair(m, prev, frames, 2, K, o)
        assert ref["reject"] == want
        count, idx, dist = m.filtered_matches(prev)
        assert (count == 0) == ref["reject"], (prev, ref["err"], ref["corr"])
        np.testing.assert_array_equal(idx, before[prev][1])
        assert np.all(np.isnan(m.verify_stats(prev)[0]))  # the surface-area stage has not run
    assert np.all(np.isnan(m.verify_stats(2)[1]))
    m.close()


def test_dense_verify_is_deterministic():
    W, H = 80, 60
    images, frames, K = vr.dense_images(), vr.dense_frames(W, H), vr.cache_intrinsics(W, H)
    runs = []
    for _ in range(2):
        m = make_matcher(images)
        for i in range(4):
            m.set_valid(i, True)
        m.match(2, 0)
        m.filter(2, 0)
        m.filter_surface_area(2, 0)
        m.filter_dense_verify(2, 0, bfa.CacheFrames.from_host(frames, K))
        runs.append(np.concatenate([np.concatenate([a, s.ravel()]) for a, s in (m.verify_stats(p) for p in (0, 1, 3))]))
        m.close()
    assert not np.any(np.isnan(runs[0]))
    np.testing.assert_array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))


# ---- skips and indexing -------------------------------------------------------------------------------------------------
def test_skips_and_indexing():
    images = vr.skip_images()
    W, H = vr.SKIP_SHAPE
    K, o = vr.cache_intrinsics(W, H), vr.SMALL_OPTS
    cur, start = vr.SKIP_CUR, vr.SKIP_START
    m = make_matcher(images, max_images=8, max_keys=128)
    for wrong in (False, True):
        frames = vr.skip_frames(wrong)
        cache = bfa.CacheFrames.from_host(frames, K)
        for i in range(6):
            m.set_valid(i, True)
        m.match(cur, 0)
        m.filter(cur, 0)
        m.debug_set_filtered(vr.SKIP_ZERO, np.zeros((0, 2), np.uint32))  # a pair whose count is already 0
        m.set_valid(vr.SKIP_INVALID, False)                              # invalid, with matches left from the filter
        before = {p: (m.filtered_matches(p), m.transforms(p)) for p in range(6) if p != cur}
        assert before[0][0][0] >= 5 and before[vr.SKIP_INVALID][0][0] >= 5 and before[vr.SKIP_LIVE][0][0] >= 5
        assert before[vr.SKIP_EMPTY][0][0] == 0 and before[vr.SKIP_ZERO][0][0] == 0
        m.filter_surface_area(cur, start)
        m.filter_dense_verify(cur, start, cache, verify_options(o))
        for p in (0, vr.SKIP_EMPTY, vr.SKIP_INVALID, vr.SKIP_ZERO, cur):  # before startFrame, and the skipped pairs
            area, sums = m.verify_stats(p)
            assert np.all(np.isnan(area)) and np.all(np.isnan(sums)), p
        for p in (0, vr.SKIP_INVALID):  # untouched: the counts stay
            assert m.filtered_matches(p)[0] == before[p][0][0]
        area, _ = m.verify_stats(vr.SKIP_LIVE)
        sa = vr.surface_area_pair(all_keys(images), before[vr.SKIP_LIVE][0][1][:before[vr.SKIP_LIVE][0][0]], KINV)
        assert not sa["reject"] and np.all(np.abs(area - sa["area"]) <= vr.AREA_TOL * sa["area"])
        ref = check_dense_pair(m, vr.SKIP_LIVE, frames, cur, K, o)
        assert ref["reject"] == wrong
        count, idx, dist = m.filtered_matches(vr.SKIP_LIVE)
        np.testing.assert_array_equal(idx, before[vr.SKIP_LIVE][0][1])  # list and transforms stay either way
        np.testing.assert_array_equal(dist, before[vr.SKIP_LIVE][0][2])
        np.testing.assert_array_equal(m.transforms(vr.SKIP_LIVE)[0], before[vr.SKIP_LIVE][1][0])
        np.testing.assert_array_equal(m.transforms(vr.SKIP_LIVE)[1], before[vr.SKIP_LIVE][1][1])
        res, total = m.add_to_residuals(cur, start, 64)
        # AddCurrToResidualsCU looks at counts only, so the pair invalidated after the filter still contributes
        stale = before[vr.SKIP_INVALID][0][0]
        assert set(res["j"].tolist()) == {cur} and len(res) == total
        if wrong:  # the rejected pair is gone from filterFrames and the EntryJ list
            assert count == 0 and total == stale and set(res["i"].tolist()) == {vr.SKIP_INVALID}
            assert m.filter_frames(cur, start) == NO_FRAME and not m.get_valid(cur)
        else:
            assert count == before[vr.SKIP_LIVE][0][0] and total == stale + count
            assert set(res["i"].tolist()) == {vr.SKIP_INVALID, vr.SKIP_LIVE}
            assert m.filter_frames(cur, start) == vr.SKIP_LIVE and m.get_valid(cur)
    # argument checks that need a handle
    L = bfa.lib()
    u = C.c_uint32
    Kc = cache.intrinsics.ctypes.data_as(C.c_void_p)
    assert L.bf_match_filter_surface_area(m.h, u(6), u(0), None) == BF_ERR_ARG and b"curFrame" in L.bf_last_error()
    assert L.bf_match_filter_dense_verify(m.h, u(6), u(0), cache.table.ptr, u(6), u(W), u(H), Kc, None) == BF_ERR_ARG
    assert b"curFrame" in L.bf_last_error()
    assert L.bf_match_filter_dense_verify(m.h, u(3), u(0), cache.table.ptr, u(5), u(W), u(H), Kc, None) == BF_ERR_ARG
    assert b"nFrames" in L.bf_last_error()
    assert L.bf_match_filter_dense_verify(m.h, u(3), u(0), None, u(6), u(W), u(H), Kc, None) == BF_ERR_ARG
    assert L.bf_match_verify_stats(m.h, u(6), None, None) == BF_ERR_ARG
    m.close()


# ---- the false loop closure, end to end -------------------------------------------------------------------------------------
def test_false_loop_closure_is_rejected_with_frames():
    """Image 3's key points agree with a rigid motion to image 2, its depth was seen from 0.3 m elsewhere: the Kabsch
    filter links the pair, the dense verify does not."""
    W, H = 80, 60
    images, frames, K = vr.dense_images(), vr.dense_frames(W, H), vr.cache_intrinsics(W, H)
    cache = bfa.CacheFrames.from_host(frames, K)
    m = make_matcher(images)

    def prepare():
        for i in range(4):
            m.set_valid(i, i == 3)  # only the false partner is on offer

    prepare()
    assert m.match_and_filter(2, 0) == 3 and m.get_valid(2)
    assert m.add_to_residuals(2, 0, 64)[1] >= 5
    prepare()
    assert m.match_and_filter(2, 0, verify=bfa.match_verify_options()) == 3  # spread-out key points pass surface area
    prepare()
    assert m.match_and_filter(2, 0, cache=cache) == NO_FRAME and not m.get_valid(2)
    assert m.add_to_residuals(2, 0, 64)[1] == 0
    area, sums = m.verify_stats(3)
    assert np.any(area >= 0.032) and not np.any(np.isnan(sums))
    for i in range(4):  # with the honest partners on offer the frame is linked to the highest of them
        m.set_valid(i, True)
    assert m.match_and_filter(2, 0, cache=cache) == 1 and m.get_valid(2)
    assert [m.filtered_matches(p)[0] > 0 for p in (0, 1, 3)] == [True, True, False]
    m.close()


# ---- real cache frames ------------------------------------------------------------------------------------------------------
def test_real_cache_frames():
    opts = cache_options(*vr.REAL_IN, max_frames=4)
    cache = CUDACache(opts)
    keep = []
    for d, c in vr.real_depths():
        dd, cc = bfa.DeviceArray.from_host(d), bfa.DeviceArray.from_host(c)
        keep.append((dd, cc))
        cache.storeFrame(dd, cc, vr.REAL_IN[0], vr.REAL_IN[1])
    frames = [cache.download(i) for i in range(3)]
    table = bfa.CacheFrames.from_cache(cache)
    assert (table.n, table.width, table.height) == (3, 80, 60)
    K = cache.intrinsics()[0]
    images = vr.real_images()
    m = make_matcher(images)
    for i in range(3):
        m.set_valid(i, True)
    m.match(2, 0)
    m.filter(2, 0)
    assert m.filtered_matches(0)[0] >= 5 and m.filtered_matches(1)[0] >= 5
    m.filter_surface_area(2, 0)
    m.filter_dense_verify(2, 0, table)
    for prev, want in ((0, False), (1, True)):
        ref = check_dense_pair(m, prev, frames, 2, K, vr.OPTS)
        assert ref["reject"] == want and (m.filtered_matches(prev)[0] == 0) == want
    assert m.filter_frames(2, 0) == 0
    m.close()
    cache.close()
