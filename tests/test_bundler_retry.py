"""CPU checks of the bundler's retry path: the NumPy restatement (tests/bundler_retry_ref.py) on hand-made count tables
(list order, the attempt rule, the loop-around stop, the seeds, prefix[]) and the argument checks of every new entry,
none of which needs a device."""
import ctypes as C

import numpy as np

import bundlefusion_amd as bfa
import bundler_ref as B
import bundler_retry_ref as RR
from bundlefusion_amd import abi

NONE = RR.NONE
BF_ERR_ARG = -2
RETRY_FUNCTIONS = ["bf_retry_enable", "bf_retry_attempt", "bf_retry_last", "bf_retry_list", "bf_retry_apply_seeds",
                   "bf_retry_keyframe_frames", "bf_retry_debug_close"]


def test_header_declares_and_library_exports_the_retry_entries():
    declared = set(abi.header_functions())
    L = C.CDLL(abi.LIB_PATH)
    for name in RETRY_FUNCTIONS:
        assert name in declared and hasattr(L, name), name
    assert sorted(n for n in declared if n.startswith("bf_retry_")) == sorted(RETRY_FUNCTIONS)
    n = C.c_size_t()
    assert bfa.lib().bf_abi_struct_size(b"BFBundlerRetry", C.byref(n)) == 0 and n.value == C.sizeof(abi.BFBundlerRetry) == 80
    assert bfa.lib().bf_abi_version() == 4
    for m in ("set_retry", "retry", "last_retry", "retry_list", "apply_seeds", "keyframe_frames", "debug_retry_close"):
        assert callable(getattr(bfa.Bundler, m)), m


def test_every_new_entry_rejects_null_arguments_on_the_host():
    """No device is needed: a null handle or pointer is BF_ERR_ARG before any device work."""
    L = bfa.lib()
    r, u, n = abi.BFBundlerRetry(), C.c_uint32(), C.c_uint32()
    words, flags, T = (C.c_uint32 * 4)(), (C.c_int32 * 4)(), (C.c_float * 16)()
    fake = C.c_void_p(8)  # a non-null handle that is never dereferenced: the other pointer is null
    for rc in (L.bf_retry_enable(None, C.c_uint32(1)), L.bf_retry_attempt(None, C.byref(r)), L.bf_retry_attempt(fake, None),
               L.bf_retry_last(None, C.byref(r)), L.bf_retry_last(fake, None),
               L.bf_retry_list(None, words, C.c_uint32(4), C.byref(n)), L.bf_retry_list(fake, words, C.c_uint32(4), None),
               L.bf_retry_list(fake, None, C.c_uint32(4), C.byref(n)),
               L.bf_retry_apply_seeds(None, T, C.c_uint32(1)), L.bf_retry_apply_seeds(fake, None, C.c_uint32(1)),
               L.bf_retry_keyframe_frames(None, u, flags, C.byref(n)), L.bf_retry_keyframe_frames(fake, u, None, C.byref(n)),
               L.bf_retry_keyframe_frames(fake, u, flags, None),
               L.bf_retry_debug_close(None, u, C.byref(r)), L.bf_retry_debug_close(fake, u, None)):
        assert rc == BF_ERR_ARG and b"null" in L.bf_last_error()


def test_close_step_with_start_behind_the_candidate():
    """cur = 1 in the middle, start = 2: counts below start are another launch's and are not read; an invalid later image
    with a count is appended but cannot be the last matched frame."""
    c = B.close_frame([25, 0, 0, 25, 0, 1], [1, 0, 1, 1, 1, 1], 1, 2, 40, 100)
    assert c["valid"] and c["last"] == 5 and c["added"] == 26 and c["total"] == 66 and c["bases"] == {2: 0, 3: 0, 4: 25, 5: 25}
    c = B.close_frame([25, 0, 0, 25, 0, 1], [1, 0, 1, 1, 1, 0], 1, 2, 40, 100)
    assert c["valid"] and c["last"] == 3 and c["added"] == 26
    c = B.close_frame([25, 0, 0, 0, 0, 7], [1, 0, 1, 1, 1, 0], 1, 2, 40, 100)  # only an invalid image has a count
    assert not c["valid"] and c["added"] == 0 and c["total"] == 40
    c = B.close_frame([25, 0, 9], [1, 0, 1], 1, 2, 40, 48)  # a single later image, capacity one below the need
    assert c["overflow"] and not c["valid"] and c["total"] == 40


def test_front_in_front_out_over_a_run_of_three_lost_key_frames():
    """Key frames 1, 2, 3 are lost; 4 sees 0; 3 sees 4, 2 sees 3, 1 sees 2: the newest lost one is tried first and the
    run chains back from its newest end, one revalidation per key frame."""
    counts = RR.table_counts({(0, 4): 20, (3, 4): 11, (2, 3): 12, (1, 2): 13, (0, 5): 9, (0, 6): 9, (0, 7): 9})
    g = RR.Global(16)
    outs = [g.fuse(True, counts) for _ in range(4)]
    assert [o["globalTrackingLost"] for o in outs] == [0, 1, 1, 1] and list(g.list) == [3, 2, 1]
    assert all(o["retry"]["attempted"] == 0 for o in outs)
    o4 = g.fuse(True, counts)
    assert o4["valid"] and o4["lastMatchedGlobal"] == 0 and o4["retry"]["revalidated"] == 3 and list(g.list) == [2, 1]
    assert o4["retry"]["residualsAdded"] == 11 and o4["retry"]["lastMatchedGlobal"] == 4 and g.prefix[4] == 31
    # 4's seeds from key frame 0, then the candidate's: (3, 4), (4, 4) and Bundler.cpp:330's (3, 4)
    assert o4["retry"]["seeds"] == [(4, 0), (5, 0), (3, 4), (4, 4), (3, 4)]
    o5 = g.fuse(True, counts)
    assert o5["retry"]["revalidated"] == 2 and o5["retry"]["lastMatchedGlobal"] == 3 and list(g.list) == [1]
    o6 = g.fuse(True, counts)
    assert o6["retry"]["revalidated"] == 1 and o6["retry"]["lastMatchedGlobal"] == 2 and not g.list
    o7 = g.fuse(True, counts)
    assert o7["retry"] == RR.blank(g.total) | dict(seeds=[(7, 0), (8, 0)]) and g.valid == [1] * 8
    assert g.records == [(0, 4, 20), (4, 3, 11), (0, 5, 9), (3, 2, 12), (0, 6, 9), (2, 1, 13), (0, 7, 9)]
    assert g.prefix == [0, 0, 0, 0, 31, 52, 74, 83] and g.bound_holds()


def test_a_candidate_that_fails_twice_and_a_keyless_key_frame():
    counts = RR.table_counts({(0, 2): 8, (0, 3): 8, (0, 5): 8, (1, 5): 25})
    g = RR.Global(16)
    g.fuse(True, counts)
    assert g.fuse(True, counts)["globalTrackingLost"] and list(g.list) == [1]
    for k in (2, 3):  # 1 fails against 2, then against 2 and 3: back to the front each time
        o = g.fuse(True, counts)
        assert o["valid"] and o["retry"]["attempted"] and o["retry"]["candidate"] == 1 and o["retry"]["revalidated"] == NONE
        assert o["retry"]["seeds"] == [(k, 0), (k + 1, 0)] and list(g.list) == [1] and o["retry"]["listLength"] == 1
    o = g.fuse(False, counts)  # key frame 4 has no keys: lost, but never on the list (Bundler.cpp:115)
    assert o["globalTrackingLost"] and list(g.list) == [1] and not o["retry"]["attempted"]
    g.invalid()                # nor does invalid_submap's image (key frame 5 of the table is key frame 6 here)
    assert list(g.list) == [1] and g.valid[5] == 0
    counts = RR.table_counts({(0, 6): 8, (1, 6): 25})
    o = g.fuse(True, counts)
    assert o["keyframe"] == 6 and o["retry"]["revalidated"] == 1 and o["retry"]["lastMatchedGlobal"] == 6 and not g.list
    assert g.records[-2:] == [(0, 6, 8), (6, 1, 25)] and g.bound_holds()
    off = RR.Global(16, retry=False)
    outs = [off.fuse(True, counts) for _ in range(3)]
    assert [o["globalTrackingLost"] for o in outs] == [0, 1, 1] and not off.list and all(not o["retry"]["seeds"] for o in outs)


def test_the_stop_after_one_loop():
    """Sequence over, nothing matches. A failed candidate goes back to the FRONT, so the next call pops it again: that is
    the loop-around, retrying ends for good, and the popped index is dropped. The older entry is never tried."""
    counts = RR.table_counts({})
    g = RR.Global(16)
    for _ in range(3):
        g.fuse(True, counts)
    assert list(g.list) == [2, 1]
    a = g.retry(counts)  # 2 is the last key frame: matched as a current frame (start 0), pushed back once
    assert a["attempted"] and a["candidate"] == 2 and a["revalidated"] == NONE and not a["finished"] and list(g.list) == [2, 1]
    b = g.retry(counts)
    assert not b["attempted"] and b["finished"] and list(g.list) == [1]
    c = g.retry(counts)
    assert c == RR.blank(0, 1, True) | dict(capacity=False)
    # a candidate that connects once the sequence is over: 1 sees 3, tried after the newer 2 has been revalidated
    counts = RR.table_counts({(0, 3): 5, (1, 3): 6, (2, 3): 7})
    g = RR.Global(16)
    for _ in range(3):
        g.fuse(True, counts)
    o3 = g.fuse(True, counts)
    assert o3["retry"]["revalidated"] == 2 and list(g.list) == [1]
    a = g.retry(counts)
    assert a["revalidated"] == 1 and a["lastMatchedGlobal"] == 3 and a["seeds"] == [(1, 3), (2, 3), (1, 3)] and not g.list
    assert g.prefix == [0, 0, 0, 18] and g.records[-1] == (3, 1, 6) and g.bound_holds()
    assert g.retry(counts) == RR.blank(18) | dict(capacity=False)


def test_seeds_dropped_at_max_keyframes():
    counts = RR.table_counts({(0, 2): 5, (1, 2): 6, (0, 3): 5})
    g = RR.Global(3)
    g.fuse(True, counts)
    g.fuse(True, counts)
    o = g.fuse(True, counts)  # (3, 0) names a pose past the store: dropped; the candidate's (2, 2) stays
    assert o["retry"]["seeds"] == [(2, 0), (1, 2), (2, 2), (1, 2)] and o["retry"]["revalidated"] == 1
    g = RR.Global(16)
    g.fuse(True, counts)
    g.fuse(True, counts)
    assert g.fuse(True, counts)["retry"]["seeds"] == [(2, 0), (3, 0), (1, 2), (2, 2), (1, 2)]
    g = RR.Global(16)  # lastMatched + 1 == cur: no re-initialisation for the current key frame
    assert [g.fuse(True, RR.table_counts({(0, 1): 5}))["retry"]["seeds"] for _ in range(2)] == [[], []]


def test_capacity_leaves_the_candidate_on_the_list():
    counts = RR.table_counts({(0, 2): 5, (1, 2): 6})
    g = RR.Global(16, cap=10)
    g.fuse(True, counts)
    g.fuse(True, counts)
    o = g.fuse(True, counts)
    assert o["valid"] and o["capacity"] and o["retry"]["attempted"] and o["retry"]["revalidated"] == NONE
    assert list(g.list) == [1] and g.total == 5 and g.valid == [1, 0, 1] and g.prefix == [0, 0, 5]
