"""Python binding of the bundler (bf_bundler_*): Bundler in its local and global role plus the input half of
OnlineBundler. Frames in; per frame the sift pose and integration transform, per submap and globally the EntryJ lists in
the form bf_solver_solve / bf_recon_set_*_correspondences take."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import DeviceArray, check, lib
from .abi import (BUNDLER_GLOBAL, BUNDLER_LOCAL, BUNDLER_NO_FRAME, BUNDLER_OPT_LOCAL, ENTRYJ_DTYPE, BFBundlerEnd, BFBundlerFrame,
                  BFBundlerKeyframe, BFBundlerOptions, BFBundlerRetry, BFBundlerStats, BFBundlerSubmap, BFCacheOptions, BFMatcherOptions,
                  BFMatchVerifyOptions, BFSiftOptions)
from .cache import CUDACache
from .match import Matcher
from .sift import Sift

__all__ = ["Bundler", "bundler_options", "BUNDLER_LOCAL", "BUNDLER_OPT_LOCAL", "BUNDLER_GLOBAL", "BUNDLER_NO_FRAME"]


def bundler_options(sift: BFSiftOptions, local: BFMatcherOptions, global_: BFMatcherOptions, cache: BFCacheOptions,
                    color_intrinsics, submap_size=10, max_keyframes=1200, verify: BFMatchVerifyOptions | None = None,
                    max_local_corr=0, max_global_corr=0, filter_intensity=False, intensity_sigma_d=2.5) -> BFBundlerOptions:
    """The stages' own option structs (sift_options, matcher_options x 2, cache_options, match_verify_options), copied.
    The fields the bundler decides are set here: both matchers' maxImages, local.fuseMaxCorr, cache.maxFrames.
    color_intrinsics: row-major 4x4 of the SIFT image's camera."""
    o = BFBundlerOptions()
    C.memmove(C.byref(o.sift), C.byref(sift), C.sizeof(BFSiftOptions))
    C.memmove(C.byref(o.local), C.byref(local), C.sizeof(BFMatcherOptions))
    C.memmove(C.byref(o.global_), C.byref(global_), C.sizeof(BFMatcherOptions))
    C.memmove(C.byref(o.cache), C.byref(cache), C.sizeof(BFCacheOptions))
    if verify is not None:
        C.memmove(C.byref(o.verify), C.byref(verify), C.sizeof(BFMatchVerifyOptions))
    o.local.maxImages = o.global_.maxImages = o.local.fuseMaxCorr = o.global_.fuseMaxCorr = o.cache.maxFrames = 0
    o.submapSize, o.maxKeyframes, o.maxLocalCorr, o.maxGlobalCorr = submap_size, max_keyframes, max_local_corr, max_global_corr
    o.colorIntrinsics[:] = np.asarray(color_intrinsics, np.float32).reshape(16).tolist()
    o.filterIntensity, o.intensitySigmaD = int(bool(filter_intensity)), intensity_sigma_d
    return o


def _borrowed(cls, handle: int, **attrs):
    """A stage binding over a handle the bundler owns: close() and the destructor leave it alone."""
    class Borrowed(cls):
        def close(self):
            self.h = C.c_void_p()
    obj = Borrowed.__new__(Borrowed)
    obj.h = C.c_void_p(handle)
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


def _frame_dict(r: BFBundlerFrame) -> dict:
    d = {n: int(getattr(r, n)) for n in ("frame", "localFrame", "submap", "numKeys", "siftFlags", "valid", "lastMatchedLocal",
                                         "residualsAdded", "residualsTotal", "submapClosed")}
    d["siftPose"] = np.array(r.siftPose[:], np.float32).reshape(4, 4)
    d["integrateTransform"] = np.array(r.integrateTransform[:], np.float32).reshape(4, 4)
    return d


def _retry_dict(r: BFBundlerRetry) -> dict:
    d = {n: int(getattr(r, n)) for n in ("attempted", "candidate", "revalidated", "lastMatchedGlobal", "residualsAdded",
                                         "residualsTotal", "listLength", "finished")}
    d["seeds"] = [(int(r.seeds[k][0]), int(r.seeds[k][1])) for k in range(r.numSeeds)]
    return d


class Bundler:
    """OnlineBundler's input half over bf_bundler_* (all buffers device-resident, one stream)."""

    def __init__(self, opts: BFBundlerOptions):
        self.h = C.c_void_p()
        check(lib().bf_bundler_create(C.byref(opts), C.byref(self.h)))
        self.opts = opts

    def close(self):
        if self.h:
            lib().bf_bundler_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        check(lib().bf_bundler_reset(self.h))

    def synchronize(self):
        check(lib().bf_bundler_synchronize(self.h))

    def process_frame(self, color: DeviceArray, depth_filt: DeviceArray, depth_raw: DeviceArray | None = None,
                      allow_capacity=False) -> dict:
        """processInput for the next frame: color [h, w, 4] uint8 RGBX, depths float32 at the detector's depth size
        (depth_raw None: the filtered image twice). Returns BFBundlerFrame as a dict (matrices 4x4 float32).
        allow_capacity: a BF_ERR_CAPACITY frame returns its record with d["capacity"] = True instead of raising."""
        r = BFBundlerFrame()
        raw = depth_filt if depth_raw is None else depth_raw
        rc = lib().bf_bundler_process_frame(self.h, color.ptr, C.c_uint32(color.shape[1]), C.c_uint32(color.shape[0]),
                                            depth_filt.ptr, raw.ptr, C.byref(r))
        if not (allow_capacity and rc == -3):
            check(rc)
        d = _frame_dict(r)
        d["capacity"] = rc == -3
        return d

    def end_sequence(self) -> dict:
        """The end of the input (bf_bundling_end_sequence): a current local set of two or more images closes where it
        stands and submap() / fuse_submap() / invalid_submap() take it as a full one; otherwise nothing closes. Afterwards
        process_frame raises BF_ERR_STATE until reset(). Waits for nothing. dict(closed, submap, numFrames, numCorr,
        isValid), all 0 when nothing closed."""
        e = BFBundlerEnd()
        check(lib().bf_bundling_end_sequence(self.h, C.byref(e)))
        return {n: int(getattr(e, n)) for n in ("closed", "submap", "numFrames", "numCorr", "isValid")}

    def debug_reclose(self) -> dict:
        r = BFBundlerFrame()
        check(lib().bf_bundler_debug_reclose(self.h, C.byref(r)))
        return _frame_dict(r)

    def set_complete_trajectory(self, T, last_valid: int):
        """T: [n, 4, 4] float32 (host array or DeviceArray), the global solve's complete trajectory."""
        d = T if isinstance(T, DeviceArray) else DeviceArray.from_host(np.ascontiguousarray(T, np.float32))
        n = int(np.prod(d.shape)) // 16
        check(lib().bf_bundler_set_complete_trajectory(self.h, d.ptr, C.c_uint32(n), C.c_uint32(last_valid)))
        self.synchronize()  # the upload above may be freed once the bundler has copied it

    def submap_raw(self) -> BFBundlerSubmap:
        s = BFBundlerSubmap()
        check(lib().bf_bundler_submap(self.h, C.byref(s)))
        return s

    def submap(self) -> dict:
        """The last closed submap (a boundary frame's, or the partial one end_sequence closed), read back: corr (EntryJ),
        key_idx [n, 2], valid [frames], is_valid, frames, submap, released, cache_frames (BFCachedFrame list), raw (the BFBundlerSubmap with its device pointers)."""
        s = self.submap_raw()
        self.synchronize()
        n = s.numCorr
        corr, kidx = np.zeros(n, ENTRYJ_DTYPE), np.zeros((n, 2), np.uint32)
        if n:
            check(lib().bf_memcpy_d2h(corr.ctypes.data_as(C.c_void_p), C.c_void_p(s.d_corr), C.c_size_t(32 * n)))
            check(lib().bf_memcpy_d2h(kidx.ctypes.data_as(C.c_void_p), C.c_void_p(s.d_keyIdx), C.c_size_t(8 * n)))
        dvalid = np.zeros(s.numFrames, np.int32)
        check(lib().bf_memcpy_d2h(dvalid.ctypes.data_as(C.c_void_p), C.c_void_p(s.d_validImages), C.c_size_t(4 * s.numFrames)))
        return dict(corr=corr, key_idx=kidx, valid=np.array(s.validImages[:s.numFrames], np.int32), device_valid=dvalid,
                    is_valid=bool(s.isValid), frames=int(s.numFrames), submap=int(s.submap), released=bool(s.released),
                    cache_frames=[s.cacheFrames[i] for i in range(self.opts.submapSize + 1)], raw=s)

    def fuse_submap(self, local_transforms, allow_capacity=False) -> dict:
        """processGlobal, state PROCESS: local_transforms [frames, 4, 4] float32 (host or DeviceArray), frame -> the
        submap's first frame. Returns BFBundlerKeyframe as a dict."""
        d = local_transforms if isinstance(local_transforms, DeviceArray) else \
            DeviceArray.from_host(np.ascontiguousarray(local_transforms, np.float32))
        k = BFBundlerKeyframe()
        rc = lib().bf_bundler_fuse_submap(self.h, d.ptr, C.byref(k))
        if not (allow_capacity and rc == -3):
            check(rc)
        self.synchronize()
        out = {n: int(getattr(k, n)) for n, _ in BFBundlerKeyframe._fields_}
        out["capacity"] = rc == -3
        return out

    def invalid_submap(self):
        check(lib().bf_bundler_invalid_submap(self.h))

    # ---- retry (Bundler::tryRevalidation, the retry list, the trajectory seeds) ----
    def set_retry(self, enable=True):
        """Off after create. Only before the first key frame; reset keeps it."""
        check(lib().bf_retry_enable(self.h, C.c_uint32(int(bool(enable)))))

    def retry(self, allow_capacity=False) -> dict:
        """The sequence-over attempt: one revalidation without a new key frame. BFBundlerRetry as a dict."""
        r = BFBundlerRetry()
        rc = lib().bf_retry_attempt(self.h, C.byref(r))
        if not (allow_capacity and rc == -3):
            check(rc)
        d = _retry_dict(r)
        d["capacity"] = rc == -3
        return d

    def last_retry(self) -> dict:
        """What the last fuse_submap or retry did about the list."""
        r = BFBundlerRetry()
        check(lib().bf_retry_last(self.h, C.byref(r)))
        return _retry_dict(r)

    def retry_list(self) -> list:
        """The key frames waiting for a revalidation, front (the next candidate) first."""
        n = C.c_uint32()
        check(lib().bf_retry_list(self.h, None, C.c_uint32(0), C.byref(n)))
        out = (C.c_uint32 * max(n.value, 1))()
        check(lib().bf_retry_list(self.h, out, C.c_uint32(n.value), C.byref(n)))
        return list(out[:n.value])

    def apply_seeds(self, d_T: DeviceArray):
        """d_T[to] = d_T[from] for the last call's seeds, in order, on the bundler's stream. d_T: [n, 4, 4] float32."""
        check(lib().bf_retry_apply_seeds(self.h, d_T.ptr, C.c_uint32(int(np.prod(d_T.shape)) // 16)))

    def keyframe_frames(self, k: int) -> np.ndarray:
        """The valid flags of the submap frames key frame k stands for (empty for an invalid_submap key frame)."""
        out, n = (C.c_int32 * self.opts.submapSize)(), C.c_uint32()
        check(lib().bf_retry_keyframe_frames(self.h, C.c_uint32(k), out, C.byref(n)))
        return np.array(out[:n.value], np.int32)

    def debug_retry_close(self, idx: int, allow_capacity=False) -> dict:
        r = BFBundlerRetry()
        rc = lib().bf_retry_debug_close(self.h, C.c_uint32(idx), C.byref(r))
        if not (allow_capacity and rc == -3):
            check(rc)
        d = _retry_dict(r)
        d["capacity"] = rc == -3
        return d

    def global_list(self) -> dict:
        """corr (EntryJ, host), key_idx [n, 2], prefix [keyframes] and the device pointer of the list."""
        pc, pk, pp = C.c_void_p(), C.c_void_p(), C.POINTER(C.c_uint32)()
        n, kf = C.c_uint32(), C.c_uint32()
        check(lib().bf_bundler_global(self.h, C.byref(pc), C.byref(pk), C.byref(n), C.byref(pp), C.byref(kf)))
        self.synchronize()
        corr, kidx = np.zeros(n.value, ENTRYJ_DTYPE), np.zeros((n.value, 2), np.uint32)
        if n.value:
            check(lib().bf_memcpy_d2h(corr.ctypes.data_as(C.c_void_p), pc, C.c_size_t(32 * n.value)))
            check(lib().bf_memcpy_d2h(kidx.ctypes.data_as(C.c_void_p), pk, C.c_size_t(8 * n.value)))
        return dict(corr=corr, key_idx=kidx, prefix=np.array(pp[:kf.value], np.uint32), d_corr=pc.value)

    def matcher(self, which: int = BUNDLER_LOCAL) -> Matcher:
        """Borrowed: read-backs only (and debug_set_filtered in tests). Ask again after a frame that closed a submap."""
        h = C.c_void_p()
        check(lib().bf_bundler_matcher(self.h, C.c_uint32(which), C.byref(h)))
        return _borrowed(Matcher, h.value, opts=self.opts.global_ if which == BUNDLER_GLOBAL else self.opts.local)

    def cache(self, which: int = BUNDLER_LOCAL) -> CUDACache:
        h = C.c_void_p()
        check(lib().bf_bundler_cache(self.h, C.c_uint32(which), C.byref(h)))
        return _borrowed(CUDACache, h.value, opts=self.opts.cache)

    def sift(self) -> Sift:
        h = C.c_void_p()
        check(lib().bf_bundler_sift(self.h, C.byref(h)))
        return _borrowed(Sift, h.value, opts=self.opts.sift)

    def intensity(self) -> np.ndarray:
        """The intensity image the last frame's detect read, [height, width] float32 on the host."""
        p = C.c_void_p()
        check(lib().bf_bundler_intensity(self.h, C.byref(p)))
        self.synchronize()
        out = np.empty((self.opts.sift.height, self.opts.sift.width), np.float32)
        check(lib().bf_memcpy_d2h(out.ctypes.data_as(C.c_void_p), p, C.c_size_t(out.nbytes)))
        return out

    def stats(self) -> dict:
        s = BFBundlerStats()
        check(lib().bf_bundler_stats(self.h, C.byref(s)))
        return {n: int(getattr(s, n)) for n, _ in BFBundlerStats._fields_}
