"""GPU checks of the bundler's end of sequence (bf_bundling_end_sequence) on a stand-alone bundler.

Fixture: sift_ref's `medium` scene (320 x 240), views pose(0..8), submapSize 3, at most 4 key frames: the frames
tests/test_recon_bundler_gpu.py uses. 8 frames end in a partial submap of 2 images (overlap frame 6 + frame 7), 9 frames in
one of 3 images, 7 frames on a boundary frame. Closed submaps are fused with the sift-chain local transforms (local_init).
Every bundler runs once (module scope) and the tests read what it left."""
import numpy as np
import pytest

import bundlefusion_amd as bfa
import bundler_ref as B
import fuse_ref as fr
from bundlefusion_amd.abi import BUNDLER_GLOBAL, BUNDLER_LOCAL, BUNDLER_OPT_LOCAL
from test_bundler import options
from test_recon_bundler_gpu import S, local_init, same, upload

pytestmark = pytest.mark.gpu
BF_ERR_STATE = -4


def code_and_text(fn, *a):
    with pytest.raises(bfa.BFError) as e:
        fn(*a)
    return e.value.code, str(e.value)


def store_keys(m):
    """The local store's linear key array and descriptors, as fuse_ref takes them."""
    parts = [m.image_keys(i) for i in range(m.num_images())]
    return (np.concatenate([k.view(np.float32).reshape(-1, 4) for k, _ in parts]), np.concatenate([d for _, d in parts]))


def feed(b, dev, fuse=True):
    """Frames through process_frame; a closed submap is fused with its sift-chain transforms (or left waiting)."""
    recs = []
    for dc, dd in dev:
        recs.append(b.process_frame(dc, dd))
        if recs[-1]["submapClosed"] and fuse:
            sm = b.submap()
            b.fuse_submap(local_init(recs, sm["submap"], sm["valid"]))
    return recs


def run_end(dev, F):
    """F frames, end_sequence, the partial submap read back, then fused; and the same images as a fresh stream."""
    bo = options("medium", S)
    b = bfa.Bundler(bo)
    recs = feed(b, dev[:F])
    waits = b.stats()["hostWaits"]
    end = b.end_sequence()
    waits_after = b.stats()["hostWaits"]
    sub = b.submap()
    keys, descs = store_keys(b.matcher(BUNDLER_LOCAL))  # nothing was swapped: the closed set is still the current one
    T = local_init(recs, 2, sub["valid"])
    kf = b.fuse_submap(T)
    gkeys, gdescs = b.matcher(BUNDLER_GLOBAL).image_keys(2)
    out = dict(b=b, bo=bo, recs=recs, end=end, waits=(waits, waits_after), sub=sub, keys=keys, descs=descs, T=T, kf=kf,
               gkeys=gkeys, gdescs=gdescs, after=b.submap(), glob=b.global_list(), stats=b.stats())
    fresh = bfa.Bundler(bo)
    feed(fresh, dev[6:F])
    out["fresh_end"] = fresh.end_sequence()
    out["fresh"] = fresh.submap()
    fresh.close()
    return out


@pytest.fixture(scope="module")
def dev():
    return upload(B.views("medium", 10))


@pytest.fixture(scope="module")
def ends(dev):
    return {F: run_end(dev, F) for F in (8, 9)}


@pytest.mark.parametrize("F", [8, 9])
def test_partial_close(ends, F):
    run, n = ends[F], F - 6
    assert run["end"] == dict(closed=1, submap=2, numFrames=n, numCorr=len(run["sub"]["corr"]), isValid=1)
    assert run["waits"][0] == run["waits"][1]  # no host wait
    sub, fresh = run["sub"], run["fresh"]
    assert sub["submap"] == 2 and sub["frames"] == n and sub["is_valid"] and not sub["released"]
    assert sub["valid"].tolist() == sub["device_valid"].tolist() == [1] * n
    assert len(sub["corr"]) > 0 and set(sub["corr"]["j"].tolist()) == set(range(1, n)) and np.all(sub["corr"]["i"] < sub["corr"]["j"])
    # the same images in the same local positions of a fresh stream: the lists and flags, not the trajectories
    assert run["fresh_end"] == dict(closed=1, submap=0, numFrames=n, numCorr=len(sub["corr"]), isValid=1)
    assert fresh["frames"] == n and fresh["submap"] == 0
    same(sub["corr"], fresh["corr"], "EntryJ")
    same(sub["key_idx"], fresh["key_idx"], "key indices")
    same(sub["valid"], fresh["valid"], "valid flags")
    same(sub["device_valid"], fresh["device_valid"], "device valid flags")
    # the records of every frame of the set are the list, in frame order
    assert sum(run["recs"][f]["residualsAdded"] for f in range(7, F)) == len(sub["corr"]) == run["recs"][F - 1]["residualsTotal"]


@pytest.mark.parametrize("F", [8, 9])
def test_fuse_of_the_partial_submap(ends, F):
    """bf_bundler_fuse_submap over 2 and 3 images against fuse_ref.fuse on the same inputs, exactly."""
    run, n = ends[F], F - 6
    sub, kf = run["sub"], run["kf"]
    K = np.array(run["bo"].colorIntrinsics[:], np.float32).reshape(4, 4)
    fr.assert_margin(sub["corr"], run["T"])  # no verdict hangs on the last bit of a length
    ref = fr.fuse(run["keys"], run["descs"], sub["corr"], sub["key_idx"], run["T"], K, 1024)
    print(f"{n}-image partial submap: {len(sub['corr'])} EntryJ, {ref['num_tracks']} tracks, {len(ref['keys'])} keys")
    assert kf["keyframe"] == 2 and kf["numTracks"] == ref["num_tracks"] and kf["numKeys"] == len(ref["keys"]) > 0
    bits = lambda k: np.ascontiguousarray(k).view(np.uint32).reshape(-1, 4)
    np.testing.assert_array_equal(bits(run["gkeys"]), bits(ref["keys"]))
    np.testing.assert_array_equal(run["gdescs"], ref["descs"])
    # released as a full one is: the set is reset, the key frame counted, its valid flags kept (min(S, n) of them)
    assert run["after"]["released"] and run["stats"]["keyframes"] == 3 and run["stats"]["frames"] == F
    assert run["b"].matcher(BUNDLER_LOCAL).num_images() == 0 and run["b"].cache(BUNDLER_LOCAL).getNumFrames() == 0
    assert run["b"].keyframe_frames(2).tolist() == [1] * min(S, n)
    assert len(run["glob"]["prefix"]) == 3 and run["glob"]["prefix"][-1] == len(run["glob"]["corr"]) == kf["residualsTotal"]
    assert kf["valid"] and not kf["globalTrackingLost"] and kf["residualsAdded"] > 0  # matched an earlier key frame


def test_nothing_to_close(dev):
    b = bfa.Bundler(options("medium", S))
    recs = feed(b, dev[:6])
    recs.append(b.process_frame(*dev[6]))  # closes submap 1, which now waits
    assert recs[6]["submapClosed"]
    before = b.submap()
    waits = b.stats()["hostWaits"]
    assert b.end_sequence() == dict(closed=0, submap=0, numFrames=0, numCorr=0, isValid=0)
    assert b.stats()["hostWaits"] == waits
    sm = b.submap()
    assert sm["submap"] == 1 and sm["frames"] == S + 1 and not sm["released"]
    same(sm["corr"], before["corr"], "the waiting submap's list")
    kf = b.fuse_submap(local_init(recs, 1, sm["valid"]))  # ... and fuses normally
    assert kf["keyframe"] == 1 and kf["valid"] and kf["numKeys"] > 0 and b.submap()["released"]
    b.reset()
    b.process_frame(*dev[0])
    assert b.end_sequence()["closed"] == 0  # frame 0 alone
    code, text = code_and_text(b.submap)
    assert code == BF_ERR_STATE  # nothing has closed
    b.close()


def test_state(dev):
    b = bfa.Bundler(options("medium", S))
    code, text = code_and_text(b.end_sequence)
    assert code == BF_ERR_STATE and "no frame" in text
    # 8 frames without fusing submap 1: a partial submap would close while the previous one waits
    recs = feed(b, dev[:6])
    recs.append(b.process_frame(*dev[6]))
    recs.append(b.process_frame(*dev[7]))
    code, text = code_and_text(b.end_sequence)
    assert code == BF_ERR_STATE and "waits for fuse_submap / invalid_submap" in text
    sm = b.submap()
    assert sm["submap"] == 1 and not sm["released"]  # nothing changed
    b.fuse_submap(local_init(recs, 1, sm["valid"]))
    end = b.end_sequence()  # the refused call may be repeated
    assert end["closed"] == 1 and end["submap"] == 2 and end["numFrames"] == 2
    # the sequence is over
    code, text = code_and_text(b.process_frame, *dev[8])
    assert code == BF_ERR_STATE and "sequence is over" in text
    assert b.stats()["frames"] == 8
    assert b.end_sequence() == dict(closed=0, submap=0, numFrames=0, numCorr=0, isValid=0)  # a second call does nothing
    sm = b.submap()
    assert sm["submap"] == 2 and sm["frames"] == 2 and not sm["released"]
    b.invalid_submap()  # released as a full one is
    assert b.submap()["released"] and b.stats()["keyframes"] == 3 and len(b.keyframe_frames(2)) == 0
    code, _ = code_and_text(b.process_frame, *dev[8])
    assert code == BF_ERR_STATE
    b.reset()
    assert b.process_frame(*dev[0])["frame"] == 0  # after reset it works
    b.close()
