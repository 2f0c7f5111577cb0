"""Standalone timing of the sparse matcher's descriptor matching (bf_matcher_match) and key-point match filter
(bf_matcher_filter) on one GPU: the current image of 1 024 keys against 10 and against 500 earlier images of
1 024 keys (the reference's s_maxNumKeysPerImage and its 500 global key frames), synthetic SIFT-like descriptors
with shared landmarks (tests/match_ref.py's generator). Device-event times, warmed up, median of `reps` calls.
Prints one JSON line: ms per call, the implied int8 multiply-add rate and descriptor bytes per second, and what
they are of the int8 matrix-core rate (2x the ~2.5 PFLOP/s dense BF16 rate = 2.5e15 multiply-adds/s) and of the
HBM bandwidth (6.3 TB/s achievable). Usage: python tools/time_match.py [reps]"""
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bundlefusion_amd as bfa  # noqa: E402
import match_ref as mr  # noqa: E402

KEYS = 1024
PEAK_INT8_MAC = 2.5e15   # multiply-adds per second (MI355X int8 MFMA, dense)
PEAK_HBM = 6.3e12        # bytes per second, achievable


def timed(m, timer, fn, reps):
    L = bfa.lib()
    ms = C.c_float()
    out = []
    for _ in range(reps):
        bfa.check(L.bf_matcher_timer_start(m.h, timer))
        fn()
        bfa.check(L.bf_matcher_timer_stop(m.h, timer, C.byref(ms)))
        out.append(ms.value)
    return float(np.median(out)), float(np.min(out))


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    L = bfa.lib()
    base = mr.make_images(1, [KEYS] * 12)[0]  # 12 distinct images, reused round-robin for the 500
    timer = C.c_void_p()
    bfa.check(L.bf_timer_create(C.byref(timer)))
    result = {"keys_per_image": KEYS, "reps": reps}
    for earlier in (10, 500):
        m = bfa.Matcher(bfa.matcher_options(earlier + 1, KEYS, mr.intrinsics_inv()))
        for i in range(earlier + 1):
            m.add_image(*base[i % len(base)])
            m.set_valid(i, True)
        cur = earlier
        for _ in range(3):  # warm-up
            m.match(cur, 0)
            m.filter(cur, 0)
        m.synchronize()
        match_ms, match_min = timed(m, timer, lambda: m.match(cur, 0), reps)
        filter_ms, _ = timed(m, timer, lambda: m.filter(cur, 0), reps)
        macs = earlier * KEYS * KEYS * 128
        desc_bytes = (earlier + 1) * KEYS * 128  # every descriptor read once from HBM (re-reads hit the caches)
        raw = [m.raw_matches(p)[0] for p in range(min(earlier, 10))]
        result[f"vs_{earlier}"] = {
            "match_ms": round(match_ms, 4), "match_ms_min": round(match_min, 4), "filter_ms": round(filter_ms, 4),
            "int8_mac_per_s": macs / (match_ms * 1e-3), "fraction_of_int8_mfma_rate": macs / (match_ms * 1e-3) / PEAK_INT8_MAC,
            "descriptor_bytes_per_s": desc_bytes / (match_ms * 1e-3),
            "fraction_of_hbm_bandwidth": desc_bytes / (match_ms * 1e-3) / PEAK_HBM,
            "raw_matches_first_pairs": raw}
        m.close()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
