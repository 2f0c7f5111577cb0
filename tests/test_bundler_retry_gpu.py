"""GPU checks of the bundler's retry path (bf_retry_*). Fixture (bundler_retry_ref): one scene of 1800 blobs seen in four
stretches of three frames at x = -1.15, 1.15, 0.0, 0.5 m, 320 x 240, submapSize 3, 13 frames. Key frame 1 sees nothing of
key frame 0 and is lost; key frame 2 sees both, so the retry of 1 against 2 revalidates it. Each submap is fused with the
local transforms of the GPU's own sift chain (as bundler_ref.global_reference; no solver is involved).

What the restatement gives for the sequence through all four filters (printed by the fixture): fused keys 52 / 74 / 78 /
78; key frame 1 against 0 raw 1, filtered 0; key frame 2 against 0 filtered 9; the retry of 1 against 2 filtered 24
(surface areas 1.41 / 1.43 m^2 against 0.032, dense error 0.013 against 0.075, correspondence share 0.48 against 0.02);
key frame 3 against (0, 1, 2) filtered (0, 24, 25)."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
import bundler_ref as B
import bundler_retry_ref as RR
import sift_ref as R
from bundlefusion_amd.abi import BUNDLER_GLOBAL, BUNDLER_NO_FRAME
from test_bundler import options

pytestmark = pytest.mark.gpu
NONE = BUNDLER_NO_FRAME
BF_ERR_CAPACITY, BF_ERR_STATE = -3, -4
S = 3
KF = 5  # 13 frames at submapSize 3 need room for five key frames
KINV = R.intrinsics_inv(RR.W, RR.H)


def upload(views):
    return [(bfa.DeviceArray.from_host(np.ascontiguousarray(c)), bfa.DeviceArray.from_host(np.ascontiguousarray(d))) for c, d, *_ in views]


def local_transforms(recs, first, n):
    """frame -> the submap's first frame, float32 in bundler_ref's operation order, from the GPU's sift poses."""
    base = B.rigid_inverse(recs[first]["siftPose"])
    return np.stack([B.mat_mul(base, recs[first + k]["siftPose"]) for k in range(n)]).astype(np.float32)


def feed(b, dev, submap_size, on_keyframe=None, invalid_from=None):
    """Frames through process_frame; every closed submap through fuse_submap (or invalid_submap from key frame
    `invalid_from` on). Per key frame: the record, the retry report, the list, the waits of the fuse."""
    recs, kfs = [], []
    for f, (dc, dd) in enumerate(dev):
        recs.append(b.process_frame(dc, dd))
        if not recs[-1]["submapClosed"]:
            continue
        k = len(kfs)
        if invalid_from is not None and k >= invalid_from:
            b.invalid_submap()
            kfs.append(None)
            continue
        first = f - submap_size
        before = b.stats()["hostWaits"]
        kf = b.fuse_submap(local_transforms(recs, first, submap_size + 1))
        kf["waits"] = b.stats()["hostWaits"] - before
        kf["retry"], kf["list"] = b.last_retry(), b.retry_list()
        kf["frames"] = b.keyframe_frames(k).tolist()
        if on_keyframe:
            on_keyframe(b, k, kf)
        kfs.append(kf)
    return recs, kfs


def key_array(gm):
    return np.concatenate([gm.image_keys(i)[0].view(np.float32).reshape(-1, 4) for i in range(gm.num_images())])


@pytest.fixture(scope="module")
def lost():
    dev = upload(RR.views(S))
    grabbed = {}

    def at_keyframe_2(b, k, kf):
        if k != 2:
            return
        gm = b.matcher(BUNDLER_GLOBAL)
        grabbed["valid"] = [int(gm.get_valid(i)) for i in range(3)]
        grabbed["T"], grabbed["Tinv"] = gm.transforms(2)  # the retry's launch was the last: prev 2 against cur 1
        grabbed["count"] = int(gm.filtered_matches(2)[0])
        grabbed["global"] = b.global_list()
        grabbed["residuals"] = gm.add_to_residuals(1, 2, 1000, want_key_indices=True)

    b = bfa.Bundler(options("medium", S, max_keyframes=KF))
    b.set_retry(True)
    first = feed(b, dev, S, at_keyframe_2)
    g_first, stats = b.global_list(), b.stats()
    gm = b.matcher(BUNDLER_GLOBAL)
    keys = [len(gm.image_keys(i)[0]) for i in range(4)]
    b.reset()
    second = feed(b, dev, S)
    g_second = b.global_list()
    b.close()
    from oracle_lib import cache_store_frame
    v, o = RR.views(S), options("medium", S)
    sc = RR.Scenario(S, True, [cache_store_frame(o.cache, v[S * k][1], v[S * k][0]) for k in range(4)])
    ref, outs = sc.run(max_keyframes=KF)
    for (cur, start), L in sc.log.items():
        for prev, e in L["pairs"].items():
            print(f"restatement: cur {cur} start {start} prev {prev}: raw {e['raw']}, Kabsch {e['kabsch']}, kept {e['count']}")
    return dict(dev=dev, first=first, second=second, g_first=g_first, g_second=g_second, stats=stats, grabbed=grabbed, keys=keys,
                sc=sc, ref=ref, outs=outs)


def test_lost_then_found(lost):
    """Key frame 1 is lost at its own fuse and revalidated by key frame 2's: the records {2, 1} at the list's end, equal to
    bf_matcher_add_to_residuals(1, 2) byte for byte; every integer outcome equals the restatement's; the waits stay in
    budget; the pair transform meets the ground truth within twice the restatement's error; the solver takes the list."""
    recs, kfs = lost["first"]
    ref, outs, gr = lost["ref"], lost["outs"], lost["grabbed"]
    assert [r["submapClosed"] for r in recs] == [0, 0, 0, 1] + [0, 0, 1] * 3 and all(k >= 40 for k in lost["keys"])
    print("fused keys", lost["keys"], "restatement", [len(k) for k, _ in lost["sc"].images], "key frames", [{k: v for k, v in kf.items() if k != "retry"} for kf in kfs])
    k1, k2, k3 = kfs[1:]
    assert k1["globalTrackingLost"] == 1 and k1["valid"] == 0 and k1["list"] == [1] and k1["retry"]["attempted"] == 0
    r = k2["retry"]
    assert k2["valid"] == 1 and r["attempted"] == 1 and r["candidate"] == 1 and r["revalidated"] == 1 and k2["list"] == []
    assert gr["valid"] == [1, 1, 1] and r["lastMatchedGlobal"] == 2 and r["listLength"] == 0 and not r["finished"]
    # every integer outcome against the restatement, key frame by key frame
    for kf, want in zip(kfs, outs):
        for name in ("keyframe", "valid", "lastMatchedGlobal", "residualsAdded", "residualsTotal", "globalTrackingLost"):
            assert kf[name] == want[name], (kf["keyframe"], name)
        assert kf["retry"] == want["retry"], kf["keyframe"]
        assert not kf["capacity"]
    assert [kf["list"] for kf in kfs] == [[], [1], [], []] and list(ref.list) == []
    assert [kf["frames"] for kf in kfs] == ref.frames
    assert r["seeds"] == [(2, 0), (3, 0), (1, 2), (2, 2), (1, 2)]
    # the list: {0, 2} x 9, then the retry's {2, 1} x 24 at its end, then key frame 3's
    g = gr["global"]
    before, added = k2["residualsTotal"], r["residualsAdded"]
    assert added == gr["count"] == 24 and len(g["corr"]) == r["residualsTotal"] == before + added
    tail = g["corr"][before:]
    assert np.all(tail["i"] == 2) and np.all(tail["j"] == 1)
    e, total, kidx = gr["residuals"]
    assert total == added and tail.tobytes() == e.tobytes() and g["key_idx"][before:].tobytes() == kidx.tobytes()
    assert g["prefix"].tolist() == ref.prefix[:3] == [0, 0, before + added]
    gf = lost["g_first"]
    assert gf["prefix"].tolist() == ref.prefix and len(gf["corr"]) == ref.total
    blocks = [(int(p), int(c), n) for p, c, n in ref.records]
    at = 0
    for p, c, n in blocks:  # the blocks in list order, each naming (prev, cur)
        assert np.all(gf["corr"]["i"][at:at + n] == p) and np.all(gf["corr"]["j"][at:at + n] == c), (p, c)
        at += n
    for k, end in enumerate(gf["prefix"]):  # every record below prefix[k] names images <= k only
        assert np.all(np.maximum(gf["corr"]["i"][:end], gf["corr"]["j"][:end]) <= k)
    assert gf["corr"][:before + added].tobytes() == g["corr"].tobytes()
    # waits: <= 3 with an attempt, <= 2 without, none but the fuse's count for the first key frame
    assert [kf["waits"] for kf in kfs] == [1, 2, 3, 2]
    st = lost["stats"]
    assert st["frames"] == 13 and st["keyframes"] == 4 and st["hostWaits"] <= 2 * 13 + 2 * 4 + 1
    # the pair transform (2 -> 1) against the ground truth: key frames 1 and 2 sit at frames 3 and 6
    te, re = RR.pair_error(gr["T"], 2 * S, 1 * S, S)
    rte, rre = RR.pair_error(lost["sc"].log[(1, 2)]["pairs"][2]["T"], 2 * S, 1 * S, S)
    print(f"pair 2 -> 1: translation error {te:.5f} m (restatement {rte:.5f}), rotation error {re:.6f} rad (restatement {rre:.6f})")
    assert te <= 2 * rte and re <= 2 * rre
    # the solver takes records with imgIdx_i > imgIdx_j
    from bundlefusion_amd.solver import GLOBAL_WEIGHTS_SPARSE_ONLY, SolverBundling
    from oracle_ba import matrix_to_pose
    rot, trans = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    base = np.linalg.inv(RR.frame_pose(0, S))
    for k in range(4):
        rot[k], trans[k] = matrix_to_pose((base @ RR.frame_pose(S * k, S)).astype(np.float32))
    sol = SolverBundling(4, 4000)
    corr = bfa.DeviceArray.from_host(gf["corr"].copy())
    sol.solve(corr, len(gf["corr"]), bfa.DeviceArray.from_host(np.ones(4, np.int32)), 4, 3, 150, GLOBAL_WEIGHTS_SPARSE_ONLY["sparse"],
              rot=bfa.DeviceArray.from_host(rot), trans=bfa.DeviceArray.from_host(trans))
    res = sol.result()
    sol.close()
    print("global solve over the list with the retry's records:", res)
    assert res["error"] == 0


def test_retry_off_and_two_runs(lost):
    """Retry off: key frame 1 stays lost, no candidate is tried, every fuse waits as before the feature (the fuse's count,
    then the record); what both runs share is byte-identical. Retry on, twice (the second after reset): bit-identical."""
    dev = lost["dev"]
    b = bfa.Bundler(options("medium", S, max_keyframes=KF))
    recs, kfs = feed(b, dev, S)
    g = b.global_list()
    gm = b.matcher(BUNDLER_GLOBAL)
    valid = [int(gm.get_valid(i)) for i in range(4)]
    with pytest.raises(bfa.BFError) as e:
        b.retry()
    assert e.value.code == BF_ERR_STATE
    with pytest.raises(bfa.BFError) as e:  # a key frame exists
        b.set_retry(True)
    assert e.value.code == BF_ERR_STATE
    b.close()
    ref, outs = lost["sc"].run(retry=False, max_keyframes=KF)
    assert valid == ref.valid == [1, 0, 1, 1] and [kf["globalTrackingLost"] for kf in kfs] == [0, 1, 0, 0]
    for kf, want in zip(kfs, outs):
        for name in ("keyframe", "valid", "lastMatchedGlobal", "residualsAdded", "residualsTotal", "globalTrackingLost"):
            assert kf[name] == want[name], (kf["keyframe"], name)
        assert kf["retry"] == RR.blank(kf["residualsTotal"]) and kf["list"] == []
    assert [kf["waits"] for kf in kfs] == [1, 2, 2, 2]
    assert g["prefix"].tolist() == ref.prefix == [0, 0, 9, 34] and np.all(g["corr"]["i"] < g["corr"]["j"])
    on_recs, on_kfs = lost["first"]
    gon = lost["g_first"]
    for ra, rb in zip(recs, on_recs):  # the local side never sees the setting
        assert {k: np.asarray(v).tobytes() for k, v in ra.items()} == {k: np.asarray(v).tobytes() for k, v in rb.items()}
    assert g["corr"][:9].tobytes() == gon["corr"][:9].tobytes() and g["key_idx"][:9].tobytes() == gon["key_idx"][:9].tobytes()
    assert g["corr"][9:].tobytes() == gon["corr"][57:].tobytes()  # key frame 3 against 2: the same 25 records
    # two runs with retry on
    (ra_, ka), (rb_, kb) = lost["first"], lost["second"]
    for x, y in zip(ra_, rb_):
        assert {k: np.asarray(v).tobytes() for k, v in x.items()} == {k: np.asarray(v).tobytes() for k, v in y.items()}
    assert ka == kb
    for name in ("corr", "key_idx", "prefix"):
        assert lost["g_first"][name].tobytes() == lost["g_second"][name].tobytes(), name


def store(dev, n, **kw):
    """A global store of n key frames at submapSize 1: key frames 0 and 1 fused from frames, the others keyless."""
    b = bfa.Bundler(options("medium", 1, max_keyframes=n + 2, **kw))
    b.set_retry(True)
    feed(b, [dev[f % 3] for f in range(n + 1)], 1, invalid_from=2)
    return b


def forced_case(b, idx, counts, valid, stale=None, expect_capacity=False):
    """Forces the filtered lists and valid flags of the global store, runs the retry closing launch alone for `idx`
    and holds everything it did against bundler_ref."""
    gm = b.matcher(BUNDLER_GLOBAL)
    n = gm.num_images()
    assert len(counts) == len(valid) == n
    rng = np.random.default_rng(7 + idx + n)
    nkeys = len(key_array(gm))
    lists = {p: rng.integers(0, nkeys, size=(counts[p], 2)).astype(np.uint32) for p in range(n)}
    for p in range(n):
        gm.debug_set_filtered(p, lists[p])
        gm.set_valid(p, bool(valid[p]))
    assert not valid[idx]
    g0 = b.global_list()
    K = b.opts.maxKeyframes
    before, cap = len(g0["corr"]), b.opts.maxGlobalCorr or 25 * K * (K - 1) // 2
    waits = b.stats()["hostWaits"]
    r = b.debug_retry_close(idx, allow_capacity=True)
    assert b.stats()["hostWaits"] - waits <= 1
    c = B.close_frame(counts, valid, idx, idx + 1, before, cap)
    g1 = b.global_list()
    assert r["capacity"] == c["overflow"] == expect_capacity
    assert (r["attempted"], r["candidate"], r["residualsTotal"]) == (1, idx, c["total"]) and len(g1["corr"]) == c["total"]
    assert g1["corr"][:before].tobytes() == g0["corr"].tobytes() and g1["prefix"][-1] == c["total"]
    assert np.all(np.diff(g1["prefix"].astype(np.int64)) >= 0)
    assert bool(gm.get_valid(idx)) == c["valid"]
    if not c["valid"]:
        assert r["revalidated"] == NONE and r["residualsAdded"] == 0 and r["seeds"] == [] and r["lastMatchedGlobal"] == NONE
        return r
    assert (r["revalidated"], r["lastMatchedGlobal"], r["residualsAdded"]) == (idx, c["last"], c["added"])
    assert r["seeds"] == [(t, f) for t, f in ((idx, c["last"]), (idx + 1, c["last"]), (idx, c["last"])) if t < K]
    want, want_idx = B.residuals(key_array(gm), lists, counts, idx, idx + 1, KINV)
    assert len(want) == c["added"] and g1["corr"][before:].tobytes() == want.tobytes()
    assert g1["key_idx"][before:].tobytes() == want_idx.tobytes()
    return r


def test_closing_launch_edges(lost):
    dev = lost["dev"]
    b = store(dev, 6)
    with pytest.raises(bfa.BFError) as e:  # the last key frame is no retry frame; a valid image is no candidate
        b.debug_retry_close(5)
    assert e.value.code == BF_ERR_STATE
    with pytest.raises(bfa.BFError) as e:
        b.debug_retry_close(0)
    assert e.value.code == BF_ERR_STATE
    # counts 0 / 25 / 0 / 1 over the later images; the counts below start are 25 on purpose and must not be appended
    r = forced_case(b, 1, [25, 25, 0, 25, 0, 1], [1, 0, 1, 1, 1, 1])
    assert r["residualsAdded"] == 26 and r["lastMatchedGlobal"] == 5
    # a later image that is invalid has a count: it cannot be the last matched frame
    r = forced_case(b, 1, [25, 0, 7, 25, 0, 3], [1, 0, 0, 1, 1, 0])
    assert r["lastMatchedGlobal"] == 3
    r = forced_case(b, 1, [25, 0, 7, 0, 0, 3], [1, 0, 0, 1, 1, 0])  # ... and alone it revalidates nothing
    assert r["revalidated"] == NONE
    # idx + 1 == n - 1: a single later image
    r = forced_case(b, 4, [25, 25, 25, 25, 0, 25], [1, 1, 1, 1, 0, 1])
    assert r["residualsAdded"] == 25 and r["lastMatchedGlobal"] == 5 and r["seeds"] == [(4, 5), (5, 5), (4, 5)]
    b.close()


def test_closing_launch_across_rounds_of_64(lost):
    """66 key frames: start = 2 and n = 66 bound one full round of 64 images; one more key frame puts n in the next round,
    whose bases carry the first round's sum."""
    dev = lost["dev"]
    b = store(dev, 66)
    counts, valid = [0] * 66, [1] + [0] + [1] * 64
    counts[0], counts[2], counts[40], counts[64], counts[65] = 25, 3, 25, 25, 2
    r = forced_case(b, 1, counts, valid)
    assert r["residualsAdded"] == 55 and r["lastMatchedGlobal"] == 65
    b.process_frame(*dev[0])
    b.invalid_submap()
    counts, valid = counts + [4], valid + [1]
    r = forced_case(b, 1, counts, valid)
    assert r["residualsAdded"] == 59 and r["lastMatchedGlobal"] == 66
    valid[66], valid[65] = 0, 0
    r = forced_case(b, 1, counts, valid)  # the last round holds no valid image: the earlier round's survives
    assert r["lastMatchedGlobal"] == 64 and r["residualsAdded"] == 59
    b.close()


def test_closing_launch_capacity(lost):
    """Capacity one below the need: nothing is appended, the count is unchanged, the candidate stays invalid and the
    call returns BF_ERR_CAPACITY; with one more record of room the same lists go through."""
    dev = lost["dev"]
    b = store(dev, 4)
    before = len(b.global_list()["corr"])
    b.close()
    for room, capacity in ((25 + 6 - 1, True), (25 + 6, False)):
        b = store(dev, 4, max_global_corr=before + room)
        assert len(b.global_list()["corr"]) == before
        r = forced_case(b, 1, [25, 0, 25, 6], [1, 0, 1, 1], expect_capacity=capacity)
        assert (r["revalidated"] == NONE) == capacity
        b.close()


def test_sequence_over_mode(lost):
    """Two lost key frames and nothing to match: the calls of bf_retry_attempt in the restatement's order. The newest
    (key frame 2, the last image: matched as a current frame) is tried and goes back to the front; the next call pops it
    again, which is the reference's loop-around stop: finished, and later calls do nothing and wait for nothing."""
    f = R.FIXTURES["medium"]
    other = R.Scene(99, 1800, (2.5, 14.0), 320, extent=2.6)
    dev = lost["dev"][:6] + upload([other.render_color(R.pose(k), f["w"], f["h"], f["dw"], f["dh"]) for k in range(4)])
    b = bfa.Bundler(options("medium", S))
    b.set_retry(True)
    recs, kfs = feed(b, dev, S)
    assert [kf["globalTrackingLost"] for kf in kfs] == [0, 1, 1] and all(kf["numKeys"] >= 40 for kf in kfs)
    assert b.retry_list() == [2, 1]
    ref = RR.Global(4)
    counts = RR.table_counts({})
    for _ in range(3):
        ref.fuse(True, counts)
    assert b.last_retry()["seeds"] == []
    b.apply_seeds(bfa.DeviceArray.from_host(np.zeros((1, 4, 4), np.float32)))  # no seeds: nothing to copy or to refuse
    tried = []
    for call in range(4):
        before = b.stats()["hostWaits"]
        got, want = b.retry(), ref.retry(counts)
        waits = b.stats()["hostWaits"] - before
        assert got == want, call
        assert b.retry_list() == list(ref.list) and waits == (1 if got["attempted"] else 0)
        tried.append(got["candidate"] if got["attempted"] else None)
    assert tried == [2, None, None, None] and got["finished"] == 1 and b.retry_list() == [1]
    assert b.global_list()["prefix"].tolist() == [0, 0, 0]
    b.close()


def test_apply_seeds_copies_in_order(lost):
    """The seeds of key frame 2's fuse on a device array of distinct poses: d_T[to] = d_T[from] in the stated order."""
    b = bfa.Bundler(options("medium", S))
    b.set_retry(True)
    feed(b, lost["dev"][:10], S)
    r = b.last_retry()
    assert r["seeds"] == [(2, 0), (3, 0), (1, 2), (2, 2), (1, 2)]
    T = np.arange(4 * 16, dtype=np.float32).reshape(4, 4, 4)
    d = bfa.DeviceArray.from_host(T.copy())
    b.apply_seeds(d)
    b.synchronize()
    want = T.copy()
    for to, frm in r["seeds"]:
        want[to] = want[frm]
    assert d.download().reshape(4, 4, 4).tobytes() == want.tobytes()
    with pytest.raises(bfa.BFError) as e:  # a seed names pose 3: an array of 3 is refused before any copy
        b.apply_seeds(bfa.DeviceArray.from_host(T[:3].copy()))
    assert e.value.code == -2
    b.close()
