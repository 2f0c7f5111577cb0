"""GPU checks of key fusing (bf_match_fuse_to_global) against the NumPy float32 restatement (tests/fuse_ref.py).

Everything is compared exactly: the track tables (root, rank, good per key), the number of fused keys, every stored key's
x, y, depth bit for bit, its scale and its descriptor bytes (which name its representative key). No verdict hangs on the
last bit of a sqrtf: tests/test_match_fuse.py asserts that every record of these fixtures is at least 1e-4 away from the
0.03 m threshold, and the end-to-end test's records are noise-free."""
import functools

import numpy as np
import pytest

import bundlefusion_amd as bfa
import fuse_ref as fr
import match_ref as mr

pytestmark = pytest.mark.gpu

NONE = fr.NONE
BF_ERR_ARG, BF_ERR_CAPACITY = -2, -3
ROT_TOL, TRANS_TOL = 1e-3, 1e-3  # the bar of test_match_gpu.py's pose-free test
K = fr.intrinsics()


def local_matcher(fx, max_images=None, max_keys=None, fuse_max_corr=None):
    counts = fx["counts"]
    m = bfa.Matcher(bfa.matcher_options(max_images or len(counts), max_keys or max(counts),
                                        fuse_max_corr=max(len(fx["corr"]), 1) if fuse_max_corr is None else fuse_max_corr))
    for i, n in enumerate(counts):
        at = int(fx["off"][i])
        m.add_image(fx["keys"][at:at + n], fx["descs"][at:at + n])
    return m


def global_matcher(max_images, max_keys):
    return bfa.Matcher(bfa.matcher_options(max_images, max_keys))


def fuse(local, glob, fx, corr=None, key_idx=None):
    corr = fx["corr"] if corr is None else corr
    key_idx = fx["key_idx"] if key_idx is None else key_idx
    return local.fuse_to_global(glob, corr, key_idx, len(corr), fx["T"], K)


@functools.lru_cache(maxsize=None)
def reference(name, limit):
    fx = {"shapes": fr.shapes_fixture, "random": fr.random_fixture, "chain": fr.chain_fixture,
          "depth20": lambda: fr.depth_fixture(20, equal=(3, 11)), "depth8": lambda: fr.depth_fixture(8)}[name]()
    fr.assert_margin(fx["corr"], fx["T"])
    ref = fr.fuse(fx["keys"], fx["descs"], fx["corr"], fx["key_idx"], fx["T"], K, limit)
    return fx, ref


def bits(keys):
    return np.ascontiguousarray(keys).view(np.uint32).reshape(-1, 4)


def check(local, glob, image, result, ref):
    index, num_keys, num_tracks = result
    assert index == image
    root, rank, good = local.fuse_tracks()
    np.testing.assert_array_equal(root, ref["root"])
    np.testing.assert_array_equal(rank, ref["rank"])
    np.testing.assert_array_equal(good, ref["good"])
    assert num_tracks == ref["num_tracks"] and num_keys == len(ref["keys"])
    assert glob.num_keys(image)[0] == num_keys
    keys, descs = glob.image_keys(image)
    np.testing.assert_array_equal(descs, ref["descs"])           # the representative key of every fused key
    np.testing.assert_array_equal(bits(keys), bits(ref["keys"]))  # x, y, scale, depth bit for bit


def test_every_graph_shape_at_once():
    fx, ref = reference("shapes", 16)
    assert ref["num_tracks"] == 9 and len(ref["keys"]) == 9
    local, glob = local_matcher(fx, max_keys=16), global_matcher(2, 16)
    check(local, glob, 0, fuse(local, glob, fx), ref)


def test_random_matchings_exact_and_deterministic():
    fx, ref = reference("random", 64)
    local, glob = local_matcher(fx), global_matcher(2, 64)
    check(local, glob, 0, fuse(local, glob, fx), ref)
    first = [a.copy() for a in local.fuse_tracks()]
    check(local, glob, 1, fuse(local, glob, fx), ref)
    for a, b in zip(first, local.fuse_tracks()):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(glob.image_keys(0), glob.image_keys(1)):
        assert a.tobytes() == b.tobytes()


def test_one_component_through_every_key():
    """2 x 1 024 keys in one chain: the search is 2 048 levels deep, which no fixed-depth stack holds."""
    fx, ref = reference("chain", 1024)
    assert [c[1] for c in ref["tracks"][0]] == [1, 0] + list(range(2, 2048)) and ref["num_tracks"] == 1
    local, glob = local_matcher(fx), global_matcher(1, 1024)
    check(local, glob, 0, fuse(local, glob, fx), ref)
    assert local.fuse_tracks()[1].tolist() == [1, 0] + list(range(2, 2048))


def test_truncation_orders_by_depth_then_track_and_keeps_descriptors_with_their_keys():
    fx, ref = reference("depth20", 8)
    local, glob = local_matcher(fx), global_matcher(2, 8)
    result = fuse(local, glob, fx)
    assert result == (0, 8, 20)
    check(local, glob, 0, result, ref)
    keys, descs = glob.image_keys(0)
    order = sorted(range(20), key=lambda t: (fx["z"][t], t))[:8]
    assert order[7] == 3  # of the two tracks at the cut's depth the earlier one is kept
    np.testing.assert_array_equal(keys["depth"], fx["z"][order])
    np.testing.assert_array_equal(descs, fx["descs"][[20 + t for t in order]])
    # exactly at the limit: nothing is sorted, the image is in track order
    fx8, ref8 = reference("depth8", 8)
    local8 = local_matcher(fx8)
    result = fuse(local8, glob, fx8)
    assert result == (1, 8, 8)
    check(local8, glob, 1, result, ref8)
    np.testing.assert_array_equal(glob.image_keys(1)[0]["depth"], fx8["z"])
    assert np.any(np.diff(fx8["z"]) < 0)


def test_append_behind_the_last_image_full_store_and_empty_submap():
    fx, ref = reference("shapes", 16)
    local, glob = local_matcher(fx, max_keys=16), global_matcher(3, 16)
    n = len(ref["keys"])
    assert fuse(local, glob, fx) == (0, n, n) and glob.num_images() == 1 and glob.num_keys(0) == (n, 0)
    assert glob.get_valid(0)
    empty = fx["corr"][:0], fx["key_idx"][:0]
    assert fuse(local, glob, fx, *empty) == (1, 0, 0) and glob.num_keys(1) == (0, n)  # nCorr = 0: an image without keys
    assert np.all(local.fuse_tracks()[0] == NONE)
    result = fuse(local, glob, fx)
    assert glob.num_images() == 3 and glob.num_keys(2) == (n, n) and not glob.get_valid(2)
    check(local, glob, 2, result, ref)  # behind the first ...
    for a, b in zip(glob.image_keys(0), glob.image_keys(2)):  # ... which it left alone
        assert a.tobytes() == b.tobytes()
    with pytest.raises(bfa.BFError) as e:
        fuse(local, glob, fx)
    assert e.value.code == BF_ERR_CAPACITY and "full" in str(e.value) and glob.num_images() == 3


def test_malformed_record_is_an_error_and_leaves_the_handles_usable():
    """The key index equals the number of keys in use (43) in a store with room for 64, so even a kernel that did
    dereference it would stay inside the store's allocations."""
    fx, ref = reference("shapes", 16)
    local, glob = local_matcher(fx, max_keys=16), global_matcher(2, 16)
    assert sum(fx["counts"]) == 43
    bad = fx["key_idx"].copy()
    bad[7, 1] = 43
    with pytest.raises(bfa.BFError) as e:
        fuse(local, glob, fx, key_idx=bad)
    assert e.value.code == BF_ERR_ARG and glob.num_images() == 0
    bad_img = fx["corr"].copy()
    bad_img["j"][2] = len(fx["counts"])
    with pytest.raises(bfa.BFError) as e:
        fuse(local, glob, fx, corr=bad_img)
    assert e.value.code == BF_ERR_ARG and glob.num_images() == 0
    check(local, glob, 0, fuse(local, glob, fx), ref)


def test_host_rejections():
    fx, _ = reference("shapes", 16)
    plain = local_matcher(fx, max_keys=16, fuse_max_corr=0)  # every matcher from before this entry point
    small = local_matcher(fx, max_keys=16, fuse_max_corr=len(fx["corr"]) - 1)
    glob = global_matcher(2, 16)
    for local, target, word in ((plain, glob, "fuseMaxCorr = 0"), (small, glob, "above fuseMaxCorr"), (small, small, "same matcher")):
        with pytest.raises(bfa.BFError) as e:
            fuse(local, target, fx)
        assert e.value.code == BF_ERR_ARG and word in str(e.value)
    assert glob.num_images() == 0
    with pytest.raises(bfa.BFError) as e:
        small.fuse_tracks()  # no fuse has run on it
    assert e.value.code == -4


def test_two_submaps_fused_and_matched_give_the_key_frames_relative_pose():
    """Pose-free, end to end: 150 landmarks seen noise-free by two submaps of 11 frames; each submap's matches are fused
    with its true transforms, and the global match of the two fused images must give the true relative pose of the two
    key frames."""
    S, F = 2, 11
    rng = np.random.default_rng(4)
    pts = np.stack([rng.uniform(-0.8, 0.8, 150), rng.uniform(-0.6, 0.6, 150), rng.uniform(1.5, 3.5, 150)], 1)
    poses = [mr.pose(k, step=0.01, rot=0.005) for k in range(S * F)]
    images = mr.make_images(13, [150] * (S * F), poses=poses, pts=pts, share=1.0)[0]
    kinv = mr.intrinsics_inv()
    Kc = np.linalg.inv(kinv.astype(np.float64)).astype(np.float32)
    glob = bfa.Matcher(bfa.matcher_options(S, 512, kinv))  # room for every track: a landmark may split into several
    for s in range(S):
        local = bfa.Matcher(bfa.matcher_options(F, 512, kinv, fuse_max_corr=25 * F * (F - 1) // 2))
        corr, key_idx = [], []
        local.add_image(*images[s * F])
        for f in range(1, F):
            local.add_image(*images[s * F + f])
            assert local.match_and_filter(f, 0) != NONE
            e, total, k = local.add_to_residuals(f, 0, 25 * F, want_key_indices=True)
            assert total == len(e) > 0
            corr.append(e)
            key_idx.append(k)
        corr, key_idx = np.concatenate(corr), np.concatenate(key_idx)
        T = np.stack([np.linalg.inv(poses[s * F]) @ poses[s * F + f] for f in range(F)]).astype(np.float32)
        assert np.nanmax(fr.record_errors(corr, T)) < 1e-4  # noise-free: every record is good by a wide margin
        index, num_keys, num_tracks = local.fuse_to_global(glob, corr, key_idx, len(corr), T, Kc)
        assert index == s and num_keys == num_tracks >= 100
        local.close()
    assert glob.match_and_filter(1, 0) == 0 and glob.get_valid(1)
    assert glob.filtered_matches(0)[0] >= 5
    _, Tinv = glob.transforms(0)  # key frame 1 in key frame 0
    rel = np.linalg.inv(poses[0]) @ poses[F]
    assert np.linalg.norm(Tinv[:3, 3] - rel[:3, 3]) <= TRANS_TOL and mr.rot_diff(Tinv, rel) <= ROT_TOL
