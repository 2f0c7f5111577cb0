"""CPU checks of the bundler's end of sequence (bf_bundling_end_sequence): the ABI surface, the host rejection that needs no
device, and the restatement of the partial close (tests/bundler_end_ref.py) at every kind of stream end."""
import ctypes as C

import pytest

import bundlefusion_amd as bfa
import bundler_end_ref as E
import bundler_ref as B
from bundlefusion_amd import abi

BF_ERR_ARG = -2


def test_header_declares_and_library_exports_the_end_of_sequence():
    assert "bf_bundling_end_sequence" in abi.header_functions()
    L = C.CDLL(abi.LIB_PATH)
    assert hasattr(L, "bf_bundling_end_sequence")
    n = C.c_size_t()
    assert bfa.lib().bf_abi_struct_size(b"BFBundlerEnd", C.byref(n)) == 0
    assert n.value == C.sizeof(abi.BFBundlerEnd) == 32
    assert bfa.lib().bf_abi_version() == 4
    assert callable(bfa.Bundler.end_sequence)


def test_null_handle_is_rejected_on_the_host():
    L = bfa.lib()
    e = abi.BFBundlerEnd()
    assert L.bf_bundling_end_sequence(None, C.byref(e)) == BF_ERR_ARG and b"null" in L.bf_last_error()


# frames, submapSize -> (frames of the partial submap, its index), None: nothing closes
ENDS = [
    (7, 3, None),                        # ends on boundary frame 6: the set is the overlap frame alone
    (8, 3, ([6, 7], 2)),                 # the smallest that closes
    (9, 3, ([6, 7, 8], 2)),              # one short of full
    (10, 3, None),                       # boundary frame 9
    (1, 10, None),                       # frame 0 alone
    (10, 10, (list(range(10)), 0)),      # submapSize images, no boundary frame yet: submap 0 itself is partial
    (11, 10, None),                      # boundary frame 10
    (12, 10, ([10, 11], 1)),
    (21, 10, None),                      # boundary frame 20
]


@pytest.mark.parametrize("frames,S,want", ENDS)
def test_partial_close_restatement(frames, S, want):
    book = E.run_book(frames, S)
    before = None if book.closed is None else dict(book.closed)
    got = E.close_partial(book)
    if want is None:
        assert got is None and book.closed == before  # a closed submap that still waits stays as it is
        return
    assert got["frames"] == want[0] and got["submap"] == want[1] and got["valid"] == [1] * len(want[0]) and got["is_valid"]
    assert book.closed is got and len(got["frames"]) <= S  # never the S + 1 images of a boundary close
    assert book.images == want[0]  # nothing was copied into another set: the set is as it stood


def test_partial_close_valid_flags():
    """Bundler::isValid looks at the images after the first."""
    got = E.close_partial(E.run_book(8, 3, invalid={7}))
    assert got["frames"] == [6, 7] and got["valid"] == [1, 0] and not got["is_valid"] and got["submap"] == 2
    got = E.close_partial(E.run_book(9, 3, invalid={7}))
    assert got["valid"] == [1, 0, 1] and got["is_valid"]
    got = E.close_partial(E.run_book(9, 3, invalid={7, 8}))
    assert got["valid"] == [1, 0, 0] and not got["is_valid"]
    with pytest.raises(ValueError):
        E.close_partial(B.Book(3))


def test_the_fixture_streams_close_valid_partial_submaps():
    """medium scene, pose(0..8), submapSize 3, in the restatement chain: frames 7 and 8 are valid in their set and every
    pair keeps 25 matches, so the 2-image partial submap has 25 EntryJ and the 3-image one 75."""
    ch = B.chain_reference("medium", 9, 3)
    assert ch["valid"][7] and ch["valid"][8]
    assert ch["counts"][7] == {0: 25} and ch["counts"][8] == {0: 25, 1: 25}
    assert [s["frames"] for s in ch["submaps"]] == [[0, 1, 2, 3], [3, 4, 5, 6]]
