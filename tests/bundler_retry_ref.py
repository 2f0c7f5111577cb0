"""NumPy restatement of the bundler's retry path (csrc/bundler.hip: Bundler::tryRevalidation, Bundler.cpp:306-352; the
retry list, SIFTImageManager.h:263-271; the global-only trajectory re-initialisation, Bundler.cpp:223-237; the
sequence-over attempt, OnlineBundler.cpp:287-296), on top of bundler_ref / match_ref / match_verify_ref / fuse_ref.

`Global` is the global bundler's host bookkeeping alone: which key frame is valid, the list (front in, front out), the
attempt rule, the loop-around stop, the seeds and prefix[]. What a match finds comes from a `counts(cur, start, valid)`
callable: a hand-made table (`table_counts`) or the restated chain over the fixture (`Scenario.counts`). The closing
step is bundler_ref.close_frame, which takes `start`."""
import collections
import functools

import numpy as np

import bundler_ref as B
import match_ref as M
import match_verify_ref as V
import sift_ref as R

NONE = B.NONE
F32, F64 = np.float32, np.float64


def blank(total=0, length=0, finished=False):
    return dict(attempted=0, candidate=NONE, revalidated=NONE, lastMatchedGlobal=NONE, residualsAdded=0, residualsTotal=total,
                listLength=length, finished=int(finished), seeds=[])


class Global:
    """The global store's bookkeeping with retry. records: [(prev, cur, count)] blocks in list order."""

    def __init__(self, max_keyframes, cap=1 << 28, retry=True):
        self.K, self.cap, self.on = max_keyframes, cap, retry
        self.valid, self.has_keys, self.frames = [], [], []
        self.list = collections.deque()
        self.cont = 0  # m_continueRetry: 0 unset, > 0 the first candidate after the sequence ended, -1 done
        self.total, self.prefix, self.records = 0, [], []
        self.last = blank()

    # -- seeds: the reference's d_trajectory copies, (to, from); a `to` past the store is dropped
    def _seed(self, to, frm):
        if to < self.K:
            self.last["seeds"].append((to, frm))

    def _seeds(self, cur, last):
        if last + 1 != cur:
            self._seed(cur, last)
            self._seed(cur + 1, last)

    def _close(self, counts, cur, start):
        c = B.close_frame(counts, self.valid, cur, start, self.total, self.cap)
        self.valid[cur] = int(c["valid"])
        if c["valid"]:
            self.records += [(p, cur, min(int(counts[p]), B.FILT)) for p in range(start, len(counts)) if p != cur and counts[p] > 0]
        self.total = c["total"]
        return c

    def _end(self):
        self.last.update(residualsTotal=self.total, listLength=len(self.list), finished=int(self.cont < 0))
        return dict(self.last, seeds=list(self.last["seeds"]))

    def _revalidate(self, idx, counts):
        n = len(self.valid)
        start = 0 if idx + 1 == n else idx + 1  # the last key frame is a current frame: matched against the earlier ones
        c = self._close(counts(idx, start, list(self.valid)), idx, start)
        self.last.update(attempted=1, candidate=idx)
        if c["valid"]:
            self.last.update(revalidated=idx, lastMatchedGlobal=c["last"], residualsAdded=c["added"])
            self._seeds(idx, c["last"])
            self._seed(idx, c["last"])  # Bundler.cpp:330
        return c

    def _try(self, counts, scan_done):
        """tryRevalidation. Returns the closing step's dict or None when nothing was tried."""
        if self.cont < 0 or not self.list:
            return None
        idx = self.list.popleft()
        if scan_done:
            if self.cont == 0:
                self.cont = idx
            elif self.cont == idx:
                self.cont = -1  # looped around again: idx is dropped, as the reference drops it
                return None
        c = self._revalidate(idx, counts)
        if not c["valid"]:
            self.list.appendleft(idx)
        return c

    def fuse(self, has_keys, counts, frames=()):
        """bf_bundler_fuse_submap's global half. dict(keyframe, valid, lastMatchedGlobal, residualsAdded, residualsTotal,
        globalTrackingLost, capacity, retry)."""
        idx = len(self.valid)
        self.valid.append(1 if idx == 0 else 0)
        self.has_keys.append(bool(has_keys))
        self.frames.append(list(frames))
        self.last = blank()
        out = dict(keyframe=idx, valid=1, lastMatchedGlobal=NONE, residualsAdded=0, residualsTotal=self.total, globalTrackingLost=0,
                   capacity=False)
        if idx > 0:
            c = self._close(counts(idx, 0, list(self.valid)) if has_keys else [0] * (idx + 1), idx, 0)
            out.update(valid=int(c["valid"]), lastMatchedGlobal=c["last"], residualsAdded=c["added"], residualsTotal=c["total"],
                       globalTrackingLost=int(not c["valid"]), capacity=c["overflow"])
            if self.on:
                if c["valid"]:
                    self._seeds(idx, c["last"])
                    r = self._try(counts, False)  # one revalidation per key frame
                    out["capacity"] |= bool(r and r["overflow"])
                elif has_keys:
                    self.list.appendleft(idx)
        self.prefix.append(self.total)
        out["retry"] = self._end()
        return out

    def invalid(self):
        """bf_bundler_invalid_submap: a keyless image; it never enters the list (Bundler.cpp:115)."""
        idx = len(self.valid)
        self.valid.append(1 if idx == 0 else 0)
        self.has_keys.append(False)
        self.frames.append([])
        self.prefix.append(self.total)

    def retry(self, counts):
        """bf_bundler_retry: the sequence-over attempt."""
        assert self.on
        self.last = blank()
        r = self._try(counts, True)
        if self.prefix:
            self.prefix[-1] = self.total
        return dict(self._end(), capacity=bool(r and r["overflow"]))

    def bound_holds(self):
        """Every record below prefix[k] names images <= k only; prefix[] ascends and ends at the list's length."""
        ends = np.cumsum([c for _, _, c in self.records]) if self.records else np.zeros(0, int)
        ok = all(a <= b for a, b in zip(self.prefix, self.prefix[1:])) and (not self.prefix or self.prefix[-1] == self.total)
        for (p, c, _), e in zip(self.records, ends):
            k = next(k for k, v in enumerate(self.prefix) if v >= e)  # the first key frame whose prefix covers the block
            ok = ok and max(p, c) <= k
        return ok


def table_counts(table):
    """counts callable from {(a, b): count}, a < b: what the pair (a, b) keeps, whichever of the two is `cur`. As the
    matcher, an invalid prev gets 0."""
    def counts(cur, start, valid):
        return [0 if p < start or p == cur or not valid[p] else int(table.get((min(p, cur), max(p, cur)), 0)) for p in range(len(valid))]
    return counts


# ---- the fixture: four stretches of one scene, the second out of sight of the first -----------------------------------
W, H = 320, 240
SHIFT = (-1.15, 1.15, 0.0, 0.5)


def scene():
    return R.Scene(18, blobs=1800, sigma_px=(2.5, 14.0), ref_width=320, extent=2.6)


def frame_pose(f: int, S: int) -> np.ndarray:
    """Frame S k + i is pose(i) shifted by SHIFT[k] in x; the last frame (4 S) is pose(S) at SHIFT[3]."""
    k = min(f // S, 3)
    T = R.pose(f - k * S).copy()
    T[0, 3] += SHIFT[k]
    return T


@functools.lru_cache(None)
def views(S: int):
    sc = scene()
    return [sc.render_color(frame_pose(f, S), W, H, W, H) + (frame_pose(f, S),) for f in range(4 * S + 1)]


@functools.lru_cache(None)
def detected(S: int):
    c = R.cfg(W, H, W, H)
    out = []
    for color, depth, _ in views(S):
        d = R.detect(R.intensity(color, W, H), depth, c)
        out.append((d["keys"], d["descs"]))
    return out


def local_chain(images, S):
    """bundler_ref.chain_reference over a given image list: the closed submaps with their entries and the sift poses."""
    kinv = R.intrinsics_inv(W, H)
    book = B.Book(S)
    sift = {0: np.eye(4, dtype=F32)}
    submaps, entries = [], []
    for _ in range(len(images)):
        fr, lf, _, closes = book.add()
        if lf > 0:
            out = M.run([images[i] for i in book.images], lf, 0, book.valid, kinv)
            counts = [out["pairs"][p]["filt"]["count"] if p != lf else 0 for p in range(lf + 1)]
            tinv = [B.rigid_inverse(out["pairs"][p]["filt"]["T"]) if p != lf else None for p in range(lf + 1)]
            c = B.close_frame(counts, book.valid, lf, 0, len(entries), 1 << 28)
            book.decide(c["valid"])
            if c["valid"]:
                entries += out["entries"]
            sift[fr], _ = B.sift_step(sift, fr, lf, counts, tinv, c["valid"])
        if closes:
            book.close()
            submaps.append(dict(book.closed, entries=entries))
            entries = []
    return dict(sift=sift, submaps=submaps)


class Scenario:
    """The fixture through the restatement: local chains, fuse_ref per closed submap (local transforms from the sift
    chain, as bundler_ref.global_reference), then `Global` with the matcher's whole filter chain per attempt."""

    def __init__(self, S=3, verify=True, cache_frames=None):
        import fuse_ref as F
        self.S, self.verify = S, verify
        self.kinv = R.intrinsics_inv(W, H)
        Kc = np.linalg.inv(self.kinv.astype(F64)).astype(F32)
        images = detected(S)
        ch = local_chain(images, S)
        self.chain, self.images = ch, []
        for sm in ch["submaps"]:
            store = [images[i] for i in sm["frames"]]
            keys = np.concatenate([np.asarray(k, F32).reshape(-1, 4) for k, _ in store])
            descs = np.concatenate([d for _, d in store])
            pos = M.key_points32(keys, self.kinv)
            corr = np.array([(p, c, pos[a], pos[b]) for p, c, a, b in sm["entries"]], B._entryj())
            kidx = np.array([(a, b) for _, _, a, b in sm["entries"]], np.uint32).reshape(-1, 2)
            first = B.rigid_inverse(ch["sift"][sm["frames"][0]])
            tr = [B.mat_mul(first, ch["sift"][i]) for i in sm["frames"]]
            out = F.fuse(keys, descs, corr, kidx, tr, Kc, 1024)
            self.images.append((out["keys"], out["descs"]))
        self.cache = cache_frames  # [per key frame: CUDACache.download-like dict], needed when verify
        self.log = {}              # (cur, start) -> dict(raw, kabsch, area, dense, T) per prev

    def counts(self, cur, start, valid):
        n = len(valid)
        run = M.run(self.images[:n], cur, start, valid, self.kinv)
        out, log = [0] * n, {}
        for prev, pr in run["pairs"].items():
            f = pr["filt"]
            e = dict(raw=int(pr["raw"]["count"]) if "count" in pr["raw"] else len(pr["raw"]["idx"]), kabsch=int(f["count"]), T=f["T"],
                     idx=f["idx"], area=None, dense=None)
            c = e["kabsch"]
            if c > 0 and self.verify:
                a = V.surface_area_pair(run["keys"], f["idx"], self.kinv)
                e["area"] = a
                if a["reject"]:
                    c = 0
            if c > 0 and self.verify:
                T = np.asarray(f["T"], F32)
                d = V.dense_pair(self.cache[prev], self.cache[cur], T, B.rigid_inverse(T), self.cache[0]["K"])
                e["dense"] = d
                if d["reject"]:
                    c = 0
            e["count"] = c
            out[prev] = c
            log[prev] = e
        self.log[(cur, start)] = dict(pairs=log, keys=run["keys"])
        return out

    def run(self, retry=True, max_keyframes=4):
        g = Global(max_keyframes, retry=retry)
        outs = []
        for k, sm in enumerate(self.chain["submaps"]):
            outs.append(g.fuse(len(self.images[k][0]) > 0, self.counts, sm["valid"][:min(self.S, len(sm["valid"]))]))
        return g, outs


def pair_error(T_prev_to_cur, prev_frame, cur_frame, S):
    """(translation m, rotation rad) of camera cur in camera prev = inv(T) against the fixture's ground truth."""
    rel = np.linalg.inv(np.asarray(T_prev_to_cur, F64))
    gt = np.linalg.inv(frame_pose(prev_frame, S)) @ frame_pose(cur_frame, S)
    return float(np.linalg.norm(rel[:3, 3] - gt[:3, 3])), M.rot_diff(rel, gt)
