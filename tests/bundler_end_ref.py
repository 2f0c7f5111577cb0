"""NumPy restatement of the bundler's end of sequence (bf_bundling_end_sequence) on top of bundler_ref.Book: processInput's
past-the-end branch (OnlineBundler.cpp:171-174) and prepareLocalSolve(curFrame, true) (:134-165). The current local set
closes where it stands when it holds two or more images and the last frame was no boundary frame; nothing is copied into
the other set. The reference's "only the overlap frame -> invalidate" branch (:138-144) has no counterpart: a set of one
image is frame 0 alone or follows a boundary frame, and :171-173 exclude both."""
import bundler_ref as B


def close_partial(book: B.Book):
    """The closed dict (frames, valid, is_valid, submap) of the trailing partial submap, also left in book.closed; None
    when nothing closes (book.closed then stays what it was). ValueError before the first frame (BF_ERR_STATE)."""
    if book.frame == 0:
        raise ValueError("end of sequence before the first frame")
    last, n = book.frame - 1, len(book.images)
    boundary = last > 0 and last % book.S == 0  # isLastLocalFrame: that frame closed its submap itself
    if n < 2 or boundary:
        return None
    book.closed = dict(frames=list(book.images), valid=list(book.valid), is_valid=any(book.valid[1:]), submap=last // book.S)
    return book.closed


def run_book(frames: int, submap_size: int, invalid=()):
    """A Book fed `frames` frames (those in `invalid` decided invalid), closing at every boundary frame."""
    book = B.Book(submap_size)
    for _ in range(frames):
        f, lf, _, closes = book.add()
        if lf > 0:
            book.decide(f not in invalid)
        if closes:
            book.close()
    return book
