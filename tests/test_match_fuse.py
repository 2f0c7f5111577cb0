"""CPU checks of key fusing (bf_match_fuse_to_global): hand-worked cases of the NumPy restatement (tests/fuse_ref.py), the
search the device runs against the literal recursion on random multigraphs, the threshold margin of the GPU tests'
fixtures, and the argument checks that need no device."""
import ctypes as C
import random

import numpy as np

import bundlefusion_amd as bfa
import fuse_ref as fr
from bundlefusion_amd import abi

BF_ERR_ARG = -2
NONE = fr.NONE
I4 = np.eye(4, dtype=np.float32)


def records(edges):
    """edges: (image i, key x, pos_i, image j, key y, pos_j)"""
    corr = np.zeros(len(edges), abi.ENTRYJ_DTYPE)
    key_idx = np.zeros((len(edges), 2), np.uint32)
    for r, (i, x, pi, j, y, pj) in enumerate(edges):
        corr[r]["i"], corr[r]["j"], corr[r]["pos_i"], corr[r]["pos_j"] = i, j, pi, pj
        key_idx[r] = x, y
    return corr, key_idx


def test_header_declares_and_library_exports_the_fuse():
    declared = set(abi.header_functions())
    L = C.CDLL(abi.LIB_PATH)
    for name in ("bf_match_fuse_to_global", "bf_match_fuse_tracks", "bf_match_image_keys"):
        assert name in declared and hasattr(L, name), name
    assert [n for n, _ in abi.BFMatcherOptions._fields_][-2:] == ["fuseMaxCorr", "reserved"]
    assert C.sizeof(abi.BFMatcherOptions) == 96
    assert bfa.matcher_options(2, 8, fuse_max_corr=7).fuseMaxCorr == 7 and bfa.matcher_options(2, 8).fuseMaxCorr == 0


def test_chain_of_three_keys_by_hand():
    """Keys 0 (image 0), 1 (image 1), 2 (image 2), records (0, 1) and (1, 2), identity transforms. The root 0 enters
    through the back edge of its first neighbour: the track is 1, 0, 2, its representative key 1, and the mean is taken
    over the three entries' own positions in track order."""
    keys = np.array([[0, 0, 1.5, 1], [0, 0, 2.5, 1], [0, 0, 3.5, 1]], np.float32)
    descs = np.arange(3 * 128, dtype=np.uint32).reshape(3, 128).astype(np.uint8)
    p0, p1, p1b, p2 = [0.5, 0.25, 2.0], [0.5, 0.25, 2.0], [0.5, 0.25, 2.0], [0.52, 0.25, 2.0]
    corr, key_idx = records([(0, 0, p0, 1, 1, p1), (1, 1, p1b, 2, 2, p2)])
    T = np.stack([I4] * 3)
    K = np.diag([2.0, 4.0, 1.0, 1.0]).astype(np.float32)
    fr.assert_margin(corr, T)
    f = fr.fuse(keys, descs, corr, key_idx, T, K, 8)
    assert [c[1] for c in f["tracks"][0]] == [1, 0, 2] and len(f["tracks"]) == 1
    assert f["root"].tolist() == [0, 0, 0] and f["rank"].tolist() == [1, 0, 2] and f["good"].tolist() == [1, 1, 1]
    s = np.float32(0.5) + np.float32(0.5) + np.float32(0.52)
    mean_x = s / np.float32(3)
    assert f["num_tracks"] == 1 and f["rep"].tolist() == [1]
    np.testing.assert_array_equal(f["keys"][0], np.array([np.float32(2) * mean_x / np.float32(2), 0.5, 2.5, 2.0], np.float32))
    np.testing.assert_array_equal(f["descs"][0], descs[1])


def test_triangle_where_the_discovery_edge_decides():
    """Keys 0, 1, 2; records (0, 1) good, (0, 2) bad, (1, 2) good. The search starts at 1, finds 0 first (record order in
    1's list) and from 0 finds 2 through the BAD record before 1's own good record to 2 is looked at: 2 is out of the
    mean although a good edge reaches it. With the records reordered (1, 2), (0, 1), (0, 2), key 2 is found from 1
    through the good record and key 0 from 2 through the bad one."""
    keys = np.ones((3, 4), np.float32)
    descs = np.zeros((3, 128), np.uint8)
    a, far = [0.0, 0.0, 2.0], [0.0, 0.1, 2.0]
    T = np.stack([I4] * 3)
    e01, e02, e12 = (0, 0, a, 1, 1, a), (0, 0, a, 2, 2, far), (1, 1, a, 2, 2, a)
    corr, key_idx = records([e01, e02, e12])
    fr.assert_margin(corr, T)
    f = fr.fuse(keys, descs, corr, key_idx, T, I4, 8)
    assert [c[1] for c in f["tracks"][0]] == [1, 0, 2]
    assert f["good"].tolist() == [1, 1, 0] and f["rank"].tolist() == [1, 0, 2]
    corr, key_idx = records([e12, e01, e02])
    f = fr.fuse(keys, descs, corr, key_idx, T, I4, 8)
    assert [c[1] for c in f["tracks"][0]] == [1, 2, 0]
    assert f["good"].tolist() == [0, 1, 1] and f["rank"].tolist() == [2, 0, 1]


def test_all_bad_track_yields_nothing_and_truncation_keeps_pairs_together():
    keys = np.ones((2, 4), np.float32)
    corr, key_idx = records([(0, 0, [0, 0, 2.0], 1, 1, [0, 0.2, 2.0])])
    f = fr.fuse(keys, np.zeros((2, 128), np.uint8), corr, key_idx, np.stack([I4] * 2), I4, 8)
    assert f["num_tracks"] == 0 and len(f["keys"]) == 0 and f["root"].tolist() == [0, 0] and f["good"].tolist() == [0, 0]
    fx = fr.depth_fixture(20, equal=(3, 11))
    f = fr.fuse(fx["keys"], fx["descs"], fx["corr"], fx["key_idx"], fx["T"], fr.intrinsics(), 8)
    assert f["num_tracks"] == 20 and len(f["keys"]) == 8
    order = sorted(range(20), key=lambda t: (fx["z"][t], t))[:8]
    assert order[7] == 3 and 11 not in order  # the tie at the cut goes to the earlier track
    assert f["rep"].tolist() == [20 + t for t in order]  # a track's representative is its first entry: the key of image 1
    np.testing.assert_array_equal(f["keys"][:, 3], fx["z"][order])
    np.testing.assert_array_equal(f["descs"], fx["descs"][f["rep"]])


def literal(n, edges):
    adj = [[] for _ in range(n)]
    for r, (x, y) in enumerate(edges):
        adj[x].append((0, y, r))
        adj[y].append((0, x, r))
    return adj


def test_search_from_the_first_neighbour_equals_the_recursion():
    rng = random.Random(1)
    for _ in range(3000):
        n, e = rng.randint(2, 30), rng.randint(0, 40)
        edges = [(rng.randrange(n), rng.randrange(n)) for _ in range(e)]  # parallel records and self records included
        adj = literal(n, edges)
        assert fr.compute_tracks(adj) == fr.search_tracks(adj), (n, edges)


def test_the_recursion_on_a_stack_equals_the_recursion():
    """find_track's explicit stack against the reference's function written as it stands."""
    def find(adj, marker, track, k):
        for c in adj[k]:
            if not marker[c[1]]:
                track.append(c)
                marker[c[1]] = True
                find(adj, marker, track, c[1])
    rng = random.Random(2)
    for _ in range(500):
        n, e = rng.randint(2, 20), rng.randint(0, 30)
        adj = literal(n, [(rng.randrange(n), rng.randrange(n)) for _ in range(e)])
        for k in range(n):
            a, b = [], []
            find(adj, [False] * n, a, k)
            fr.find_track(adj, [False] * n, b, k)
            assert a == b


def test_gpu_fixtures_keep_their_margin_and_their_shapes():
    for fx in (fr.shapes_fixture(), fr.random_fixture(), fr.chain_fixture(64)):
        fr.assert_margin(fx["corr"], fx["T"])
    fx = fr.shapes_fixture()
    f = fr.fuse(fx["keys"], fx["descs"], fx["corr"], fx["key_idx"], fx["T"], fr.intrinsics(), 1024)
    k = lambda img, local: int(fx["off"][img] + local)  # noqa: E731
    assert f["root"][k(0, 3)] == NONE and f["root"][k(1, 3)] == NONE      # the invalidated record joins nothing
    assert f["root"][k(0, 5)] == k(0, 5) and not f["good"][k(1, 5)]        # the all-bad track exists and yields no key
    assert k(1, 5) not in f["rep"].tolist()
    assert not f["good"][k(2, 6)] and not f["good"][k(0, 7)]              # the two cycles
    assert f["root"][k(0, 9)] == k(0, 8)                                   # two keys of image 0 in one component
    assert f["rank"][k(2, 9)] == 0 and f["root"][k(2, 9)] == k(2, 9)       # the record of a key with itself
    deg = np.bincount(fx["key_idx"][fx["corr"]["i"] != NONE].ravel(), minlength=len(fx["keys"]))
    assert deg.max() == 20                                                 # the long list
    fx = fr.chain_fixture(64)
    f = fr.fuse(fx["keys"], fx["descs"], fx["corr"], fx["key_idx"], fx["T"], fr.intrinsics(), 1024)
    assert [c[1] for c in f["tracks"][0]] == [1, 0] + list(range(2, 128)) and len(f["tracks"]) == 1
    fx = fr.random_fixture()
    good = fr.record_errors(fx["corr"], fx["T"]) < fr.MAX_TRACK_CORR_ERROR
    assert 900 <= len(fx["corr"]) <= 1100 and 0.5 < good.mean() < 0.8 and (fx["corr"]["i"] == NONE).sum() > 20


def test_fuse_argument_checks_without_a_device():
    """Null handles and an oversized fuseMaxCorr fail with BF_ERR_ARG before any device work. (A matcher cannot be
    created without a device, so the rejection of a fuse from a matcher with fuse_max_corr = 0, which is a host check
    too, is in test_match_fuse_gpu.py.)"""
    L = bfa.lib()
    assert L.bf_match_fuse_to_global(None, None, None, None, 0, None, None, None, None, None) == BF_ERR_ARG
    assert b"null matcher" in L.bf_last_error()
    assert L.bf_match_fuse_tracks(None, None, None, None) == BF_ERR_ARG
    o = bfa.matcher_options(2, 8, fuse_max_corr=(1 << 28) + 1)
    h = C.c_void_p()
    assert L.bf_matcher_create(C.byref(o), C.byref(h)) == BF_ERR_ARG and b"fuseMaxCorr" in L.bf_last_error()
