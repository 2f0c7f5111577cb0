"""Python binding of the sparse matcher (bf_matcher_*): the matching side of SIFTImageManager + SiftMatchCU +
Bundler::matchAndFilter, with its Kabsch, surface-area and dense-verify filters. Key points and 128-byte descriptors in,
EntryJ and pair transforms out."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import DeviceArray, check, lib
from .abi import (ENTRYJ_DTYPE, MAX_MATCHES_FILTERED, MAX_MATCHES_RAW, SIFT_KEYPOINT_DTYPE, BFCachedFrame, BFMatcherOptions,
                  BFMatchVerifyOptions)

NO_FRAME = 0xFFFFFFFF


def matcher_options(max_images: int, max_keys_per_image: int = 1024, intrinsics_inv=None, match_thresh=0.7,
                    ratio_max=0.8, min_num_matches=5, max_kabsch_res2=0.0004, fuse_max_corr=0) -> BFMatcherOptions:
    """Defaults are zParametersBundlingDefault.txt's; intrinsics_inv: row-major 4x4 inverse colour intrinsics;
    fuse_max_corr: the most records a fuse_to_global from this matcher takes (0: it cannot be fused from)."""
    o = BFMatcherOptions()
    o.maxImages, o.maxKeysPerImage, o.fuseMaxCorr = max_images, max_keys_per_image, fuse_max_corr
    o.matchThresh, o.ratioMax, o.minNumMatches, o.maxKabschRes2 = match_thresh, ratio_max, min_num_matches, max_kabsch_res2
    k = np.eye(4, dtype=np.float32) if intrinsics_inv is None else np.asarray(intrinsics_inv, np.float32).reshape(4, 4)
    o.intrinsicsInv[:] = k.ravel().tolist()
    return o


def match_verify_options(surf_area_pca_thresh=0.032, proj_corr_dist_thres=0.15, proj_corr_normal_thres=0.97,
                         verify_sift_err_thresh=0.075, verify_sift_corr_thresh=0.02, sensor_depth_min=0.1,
                         sensor_depth_max=4.0) -> BFMatchVerifyOptions:
    """Thresholds of the surface-area and dense-verify filters; the defaults are zParametersBundlingDefault.txt's and
    zParametersDefault.txt's (a field set to 0 takes its default too)."""
    o = BFMatchVerifyOptions()
    o.surfAreaPcaThresh, o.projCorrDistThres, o.projCorrNormalThres = surf_area_pca_thresh, proj_corr_dist_thres, proj_corr_normal_thres
    o.verifySiftErrThresh, o.verifySiftCorrThresh = verify_sift_err_thresh, verify_sift_corr_thresh
    o.sensorDepthMin, o.sensorDepthMax = sensor_depth_min, sensor_depth_max
    return o


class CacheFrames:
    """Device BFCachedFrame[n] table for filter_dense_verify / match_and_filter, with the frame size and the row-major
    4x4 intrinsics of the frames. `table` keeps the device array alive; `keep` whatever owns the frames' memory."""

    def __init__(self, frames, width: int, height: int, intrinsics, keep=None):
        frames = list(frames)
        tab = (BFCachedFrame * max(len(frames), 1))(*frames)
        self.table = DeviceArray.from_host(np.frombuffer(bytes(tab), np.uint8).copy())
        self.n, self.width, self.height = len(frames), int(width), int(height)
        self.intrinsics = np.ascontiguousarray(np.asarray(intrinsics, np.float32).reshape(16))
        self.keep = keep

    @classmethod
    def from_cache(cls, cache, n: int | None = None) -> "CacheFrames":
        """The first n frames (default: all) of a CUDACache; the cache is synchronised, so the frames are complete."""
        n = cache.getNumFrames() if n is None else n
        cache.synchronize()
        return cls([cache.frame(i) for i in range(n)], cache.opts.width, cache.opts.height, cache.intrinsics()[0], keep=cache)

    @classmethod
    def from_host(cls, frames, intrinsics) -> "CacheFrames":
        """frames: dicts of host arrays depth [H, W], campos [H, W, 4], normals [H, W, 4] (float32), uploaded."""
        keep, tab = [], []
        H, W = np.asarray(frames[0]["depth"]).shape
        for f in frames:
            c = BFCachedFrame()
            for name in ("depth", "campos", "normals"):
                d = DeviceArray.from_host(np.ascontiguousarray(f[name], np.float32))
                keep.append(d)
                setattr(c, name, d.ptr.value)
            tab.append(c)
        return cls(tab, W, H, intrinsics, keep=keep)


class Matcher:
    """SIFTImageManager's image store + matchAndFilter over bf_matcher_* (all buffers device-resident)."""

    def __init__(self, opts: BFMatcherOptions):
        self.h = C.c_void_p()
        check(lib().bf_matcher_create(C.byref(opts), C.byref(self.h)))
        self.opts = opts

    def close(self):
        if self.h:
            lib().bf_matcher_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib().bf_matcher_reset(self.h))

    def add_image(self, keys: np.ndarray, descs: np.ndarray) -> int:
        """keys: [n] SIFT_KEYPOINT_DTYPE or [n, 4] float32 (x, y, scale, depth); descs: [n, 128] uint8 (host)."""
        keys = np.ascontiguousarray(keys)
        if keys.dtype != SIFT_KEYPOINT_DTYPE:
            keys = np.ascontiguousarray(keys, np.float32).reshape(-1, 4).view(SIFT_KEYPOINT_DTYPE).reshape(-1)
        descs = np.ascontiguousarray(descs, np.uint8).reshape(-1, 128)
        n = len(keys)
        assert len(descs) == n
        dk = DeviceArray.from_host(keys) if n else None
        dd = DeviceArray.from_host(descs) if n else None
        idx = C.c_uint32()
        check(lib().bf_matcher_add_image(self.h, dk.ptr if n else None, dd.ptr if n else None, C.c_uint32(n), C.byref(idx)))
        self.synchronize()  # the uploads above may be freed once the matcher has copied them
        return idx.value

    def add_image_device(self, keys: DeviceArray, descs: DeviceArray, n: int) -> int:
        idx = C.c_uint32()
        check(lib().bf_matcher_add_image(self.h, keys.ptr, descs.ptr, C.c_uint32(n), C.byref(idx)))
        return idx.value

    def num_images(self) -> int:
        n = C.c_uint32()
        check(lib().bf_matcher_num_images(self.h, C.byref(n)))
        return n.value

    def num_keys(self, image: int):
        """(key count, offset in the linear key array) of an image."""
        n, off = C.c_uint32(), C.c_uint32()
        check(lib().bf_matcher_num_keys(self.h, C.c_uint32(image), C.byref(n), C.byref(off)))
        return n.value, off.value

    def set_valid(self, image: int, valid: bool):
        check(lib().bf_matcher_set_valid(self.h, C.c_uint32(image), int(bool(valid))))

    def get_valid(self, image: int) -> bool:
        v = C.c_int()
        check(lib().bf_matcher_get_valid(self.h, C.c_uint32(image), C.byref(v)))
        return bool(v.value)

    def match(self, cur: int, start: int = 0):
        check(lib().bf_matcher_match(self.h, C.c_uint32(cur), C.c_uint32(start)))

    def filter(self, cur: int, start: int = 0):
        check(lib().bf_matcher_filter(self.h, C.c_uint32(cur), C.c_uint32(start)))

    def filter_frames(self, cur: int, start: int = 0) -> int:
        last = C.c_uint32()
        check(lib().bf_matcher_filter_frames(self.h, C.c_uint32(cur), C.c_uint32(start), C.byref(last)))
        return last.value

    def _verify(self, verify):
        return C.byref(verify) if verify is not None else None

    def filter_surface_area(self, cur: int, start: int = 0, verify: BFMatchVerifyOptions | None = None):
        check(lib().bf_match_filter_surface_area(self.h, C.c_uint32(cur), C.c_uint32(start), self._verify(verify)))

    def filter_dense_verify(self, cur: int, start: int, cache: CacheFrames, verify: BFMatchVerifyOptions | None = None):
        check(lib().bf_match_filter_dense_verify(self.h, C.c_uint32(cur), C.c_uint32(start), cache.table.ptr, C.c_uint32(cache.n),
                                                 C.c_uint32(cache.width), C.c_uint32(cache.height),
                                                 cache.intrinsics.ctypes.data_as(C.c_void_p), self._verify(verify)))

    def verify_stats(self, prev: int):
        """(area [2] = prev's side, cur's side; sums [2, 3] = {sumResidual, sumWeight, numCorr} of prev -> cur and of
        cur -> prev) as the last filter_surface_area / filter_dense_verify left them; NaN where a stage skipped the pair."""
        area, sums = np.empty(2, np.float32), np.empty(6, np.float32)
        check(lib().bf_match_verify_stats(self.h, C.c_uint32(prev), area.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p)))
        return area, sums.reshape(2, 3)

    def debug_set_filtered(self, prev: int, idx):
        """Test hook: replace pair prev's filtered list by idx [n <= 25, 2] (indices into the linear key array)."""
        idx = np.ascontiguousarray(idx, np.uint32).reshape(-1, 2)
        check(lib().bf_match_debug_set_filtered(self.h, C.c_uint32(prev), C.c_uint32(len(idx)), idx.ctypes.data_as(C.c_void_p)))

    def match_and_filter(self, cur: int, start: int | None = None, cache: CacheFrames | None = None,
                         verify: BFMatchVerifyOptions | None = None) -> int:
        """Bundler::matchAndFilter up to filterFrames; returns lastMatchedFrame (NO_FRAME if none). Without `cache` and
        `verify`: match, Kabsch filter, filterFrames. With either, the reference's whole chain in one library call:
        the surface-area filter too, and the dense verify when `cache` is given."""
        if start is None:
            start = 0 if self.num_images() == cur + 1 else cur + 1
        if cache is None and verify is None:
            self.match(cur, start)
            self.filter(cur, start)
            return self.filter_frames(cur, start)
        last = C.c_uint32()
        K = cache.intrinsics.ctypes.data_as(C.c_void_p) if cache is not None else None
        check(lib().bf_match_and_filter(self.h, C.c_uint32(cur), C.c_uint32(start), cache.table.ptr if cache is not None else None,
                                        C.c_uint32(cache.n if cache is not None else 0),
                                        C.c_uint32(cache.width if cache is not None else 0),
                                        C.c_uint32(cache.height if cache is not None else 0), K, self._verify(verify),
                                        C.byref(last)))
        return last.value

    def add_to_residuals(self, cur: int, start: int, cap: int, out: DeviceArray | None = None, want_key_indices=False):
        """(host EntryJ array, total found[, key index pairs [n, 2]])."""
        out = out if out is not None else DeviceArray((max(cap, 1),), ENTRYJ_DTYPE)
        kidx = DeviceArray((max(cap, 1), 2), np.uint32) if want_key_indices else None
        n, total = C.c_uint32(), C.c_uint32()
        check(lib().bf_matcher_add_to_residuals(self.h, C.c_uint32(cur), C.c_uint32(start), out.ptr,
                                                kidx.ptr if kidx is not None else None, C.c_uint32(cap), C.byref(n),
                                                C.byref(total)))
        res = out.download_range(0, 32 * n.value).view(ENTRYJ_DTYPE).copy() if n.value else np.zeros(0, ENTRYJ_DTYPE)
        if want_key_indices:
            k = kidx.download_range(0, 8 * n.value).view(np.uint32).reshape(-1, 2).copy() if n.value else \
                np.zeros((0, 2), np.uint32)
            return res, total.value, k
        return res, total.value

    def fuse_to_global(self, glob: "Matcher", corr, key_idx, n: int, transforms, intrinsics):
        """SIFTImageManager::fuseToGlobal: this (local) store's tracks become the next image of `glob`.
        corr: EntryJ [>= n], key_idx: uint32 [>= n, 2], transforms: float32 [images, 4, 4] (frame -> first frame), each a
        DeviceArray or a host array (uploaded); intrinsics: host row-major 4x4 colour intrinsics.
        Returns (image index in glob, keys stored, fused keys before the cut to maxKeysPerImage)."""
        def dev(a, dtype):
            return a if isinstance(a, DeviceArray) or a is None else DeviceArray.from_host(np.ascontiguousarray(a, dtype))
        n = int(n)
        d_corr = dev(corr if n else None, ENTRYJ_DTYPE)
        d_idx = dev(key_idx if n else None, np.uint32)
        d_T = dev(transforms, np.float32)
        K = np.ascontiguousarray(np.asarray(intrinsics, np.float32).reshape(16))
        idx, keys, tracks = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().bf_match_fuse_to_global(self.h, glob.h, d_corr.ptr if d_corr is not None else None,
                                            d_idx.ptr if d_idx is not None else None, C.c_uint32(n),
                                            d_T.ptr if d_T is not None else None, K.ctypes.data_as(C.c_void_p),
                                            C.byref(idx), C.byref(keys), C.byref(tracks)))
        return idx.value, keys.value, tracks.value

    def fuse_tracks(self):
        """(root, rank, good) per key of this store as the last fuse_to_global from it left them: the lowest key of the
        key's component (NO_FRAME for a key in no track), its position in the track (NO_FRAME), its flag."""
        n = sum(self.num_keys(i)[0] for i in range(self.num_images()))
        root, rank, good = np.full(n, NO_FRAME, np.uint32), np.full(n, NO_FRAME, np.uint32), np.zeros(n, np.uint8)
        check(lib().bf_match_fuse_tracks(self.h, root.ctypes.data_as(C.c_void_p), rank.ctypes.data_as(C.c_void_p),
                                         good.ctypes.data_as(C.c_void_p)))
        return root, rank, good

    def image_keys(self, image: int):
        """(keys [n] SIFT_KEYPOINT_DTYPE, descs [n, 128] uint8) of a stored image, read back to the host."""
        n = self.num_keys(image)[0]
        keys, descs = np.empty(n, SIFT_KEYPOINT_DTYPE), np.empty((n, 128), np.uint8)
        check(lib().bf_match_image_keys(self.h, C.c_uint32(image), keys.ctypes.data_as(C.c_void_p),
                                        descs.ctypes.data_as(C.c_void_p)))
        return keys, descs

    def _matches(self, fn, prev: int, cap: int):
        count = C.c_uint32()
        idx = np.empty((cap, 2), np.uint32)
        dist = np.empty(cap, np.float32)
        check(fn(self.h, C.c_uint32(prev), C.byref(count), idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p)))
        return count.value, idx, dist

    def raw_matches(self, prev: int):
        """(count of mutual matches, idx [128, 2], dist [128]); the first min(count, 128) entries are set."""
        return self._matches(lib().bf_matcher_raw_matches, prev, MAX_MATCHES_RAW)

    def filtered_matches(self, prev: int):
        return self._matches(lib().bf_matcher_filtered_matches, prev, MAX_MATCHES_FILTERED)

    def transforms(self, prev: int):
        """(T prev -> cur, Tinv cur -> prev) as 4x4 float32."""
        T, Ti = np.empty(16, np.float32), np.empty(16, np.float32)
        check(lib().bf_matcher_transforms(self.h, C.c_uint32(prev), T.ctypes.data_as(C.c_void_p), Ti.ctypes.data_as(C.c_void_p)))
        return T.reshape(4, 4), Ti.reshape(4, 4)

    def debug_dots(self, prev: int, cur: int, rows, cols):
        """(dots int32 [len(rows), len(cols)], row stats int32 [len(rows), 3] = best, second best, argument)."""
        rows = np.ascontiguousarray(rows, np.uint32)
        cols = np.ascontiguousarray(cols, np.uint32)
        dots = np.zeros((len(rows), len(cols)), np.int32)
        stats = np.zeros((len(rows), 3), np.int32)
        check(lib().bf_matcher_debug_dots(self.h, C.c_uint32(prev), C.c_uint32(cur), rows.ctypes.data_as(C.c_void_p),
                                          C.c_uint32(len(rows)), cols.ctypes.data_as(C.c_void_p), C.c_uint32(len(cols)),
                                          dots.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p)))
        return dots, stats

    def synchronize(self):
        check(lib().bf_matcher_synchronize(self.h))
