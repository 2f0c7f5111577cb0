"""Python binding of the SIFT detector (bf_sift_*): Bundler::detectFeatures -> SiftGPU::RunSIFT +
GetKeyPointsAndDescriptorsCUDA. Float intensity + depth in, key points and 128-byte descriptors out, device-resident, in
the form Matcher.add_image_device takes."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import DeviceArray, check, lib
from .abi import SIFT_KEYPOINT_DTYPE, SIFT_LEVELS, SIFT_MAX_FILTER, SIFT_TRUNCATED, BFSiftOptions

__all__ = ["Sift", "sift_options", "filter_kernel", "SIFT_TRUNCATED"]


def sift_options(width: int, height: int, depth_width: int | None = None, depth_height: int | None = None, max_keys=1024,
                 feature_count_threshold=150, sensor_depth_min=0.1, sensor_depth_max=4.0, min_key_scale=3.0,
                 dog_threshold=0.0, edge_threshold=0.0) -> BFSiftOptions:
    """Defaults are zParameters*Default.txt's (a field set to 0 takes its default too); the depth image defaults to the
    intensity image's size."""
    o = BFSiftOptions()
    o.width, o.height = width, height
    o.depthWidth = width if depth_width is None else depth_width
    o.depthHeight = height if depth_height is None else depth_height
    o.maxKeys, o.featureCountThreshold = max_keys, feature_count_threshold
    o.sensorDepthMin, o.sensorDepthMax, o.minKeyScale = sensor_depth_min, sensor_depth_max, min_key_scale
    o.dogThreshold, o.edgeThreshold = dog_threshold, edge_threshold
    return o


def filter_kernel(index: int, handle=None) -> np.ndarray:
    """The host-built coefficients of filter table `index` (0 = initial smoothing, 1...5 = level increments). The tables
    do not depend on the options: no detector (and no device) is needed."""
    k = np.zeros(SIFT_MAX_FILTER, np.float32)
    w = C.c_uint32()
    check(lib().bf_sift_filter_kernel(handle, C.c_uint32(index), k.ctypes.data_as(C.c_void_p), C.byref(w)))
    return k[: w.value].copy()


class _View:
    """A device pointer the detector owns, in the shape Matcher.add_image_device reads (.ptr)."""

    def __init__(self, ptr: int):
        self.ptr = C.c_void_p(ptr)


class Sift:
    """SiftGPU as BundleFusion configures it, over bf_sift_* (all buffers device-resident)."""

    def __init__(self, opts: BFSiftOptions):
        self.h = C.c_void_p()
        check(lib().bf_sift_create(C.byref(opts), C.byref(self.h)))
        self.opts = opts

    def close(self):
        if self.h:
            lib().bf_sift_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def intensity(self, color: DeviceArray, out: DeviceArray | None = None):
        """resampleToIntensity of a device RGBX image [h, w, 4] uint8 into `out` or the detector's own buffer."""
        ch, cw = color.shape[0], color.shape[1]
        check(lib().bf_sift_intensity(self.h, color.ptr, C.c_uint32(cw), C.c_uint32(ch), out.ptr if out is not None else None))

    def detect(self, intensity: DeviceArray | None, depth: DeviceArray):
        """Asynchronous; intensity None: the buffer `intensity` filled. Keep the inputs until result() / synchronize()."""
        check(lib().bf_sift_detect(self.h, intensity.ptr if intensity is not None else None, depth.ptr))

    def result_device(self):
        """(keys view, descriptors view, n, flags): device pointers valid until the next detect. Synchronizes."""
        pk, pd = C.c_void_p(), C.c_void_p()
        n, flags = C.c_uint32(), C.c_uint32()
        check(lib().bf_sift_result(self.h, C.byref(pk), C.byref(pd), C.byref(n), C.byref(flags)))
        return _View(pk.value), _View(pd.value), n.value, flags.value

    def result(self):
        """(keys [n] SIFT_KEYPOINT_DTYPE, descriptors [n, 128] uint8, flags) on the host."""
        k, d, n, flags = self.result_device()
        keys = np.zeros(n, SIFT_KEYPOINT_DTYPE)
        descs = np.zeros((n, 128), np.uint8)
        if n:
            check(lib().bf_memcpy_d2h(keys.ctypes.data_as(C.c_void_p), k.ptr, C.c_size_t(16 * n)))
            check(lib().bf_memcpy_d2h(descs.ctypes.data_as(C.c_void_p), d.ptr, C.c_size_t(128 * n)))
        return keys, descs, flags

    def detect_into(self, matcher, intensity: DeviceArray | None, depth: DeviceArray) -> int:
        """detect -> result -> Matcher.add_image_device; returns the image index. The matcher copies on its own stream:
        it is synchronised before returning, so the next detect may overwrite the result."""
        self.detect(intensity, depth)
        k, d, n, _ = self.result_device()
        idx = matcher.add_image_device(k, d, n)
        matcher.synchronize()
        return idx

    def level_counts(self):
        """(raw [12], kept [12]) of the last detect, level index = octave * 3 + level."""
        raw, kept = np.zeros(SIFT_LEVELS, np.uint32), np.zeros(SIFT_LEVELS, np.uint32)
        check(lib().bf_sift_level_counts(self.h, raw.ctypes.data_as(C.c_void_p), kept.ctypes.data_as(C.c_void_p)))
        return raw, kept

    def filter_kernel(self, index: int) -> np.ndarray:
        return filter_kernel(index, self.h)

    def debug_level(self, octave: int, level: int) -> np.ndarray:
        out = np.empty((self.opts.height >> octave, self.opts.width >> octave), np.float32)
        check(lib().bf_sift_debug_level(self.h, C.c_uint32(octave), C.c_uint32(level), out.ctypes.data_as(C.c_void_p)))
        return out

    def debug_raw_keys(self, level_index: int, cap: int = 4096):
        """(colRow int32 [n, 2], packed orientations uint32 [n]) of a level's raw list after cap and LimitFeatureCount(0)."""
        cr = np.zeros((cap, 2), np.int32)
        po = np.zeros(cap, np.uint32)
        n = C.c_uint32()
        check(lib().bf_sift_debug_raw_keys(self.h, C.c_uint32(level_index), cr.ctypes.data_as(C.c_void_p),
                                           po.ctypes.data_as(C.c_void_p), C.c_uint32(cap), C.byref(n)))
        m = min(n.value, cap)
        return cr[:m].copy(), po[:m].copy()

    def synchronize(self):
        check(lib().bf_sift_synchronize(self.h))
