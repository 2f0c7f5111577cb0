"""Standalone timing of the sparse matcher's descriptor matching (bf_matcher_match) and key-point match filter
(bf_matcher_filter) on one GPU: the current image of 1 024 keys against 10 and against 500 earlier images of
1 024 keys (the reference's s_maxNumKeysPerImage and its 500 global key frames), synthetic SIFT-like descriptors
with shared landmarks (tests/match_ref.py's generator). Device-event times, warmed up, median of `reps` calls.
Prints one JSON line: ms per call, the implied int8 multiply-add rate and descriptor bytes per second, and what
they are of the int8 matrix-core rate (2x the ~2.5 PFLOP/s dense BF16 rate = 2.5e15 multiply-adds/s) and of the
HBM bandwidth (6.3 TB/s achievable). Usage: python tools/time_match.py [reps]

With --filters (python tools/time_match.py --filters [reps]) it times the surface-area and dense-verify filters instead:
ms per bf_match_filter_surface_area and bf_match_filter_dense_verify call at 10 and 500 earlier images with 80 x 60
cache frames (analytic renderings, 12 distinct frames reused round-robin like the images), the Kabsch filter re-run
before every timed call so that each call sees the same counts. At 500 a second leg leaves only 10 earlier images
valid, the usual state of a global matcher: the other pairs take the early-out. Reports how many pairs were
non-empty, the bytes the dense verify requests per call (per non-empty pair and direction 36 B x W H streamed plus up
to 36 B x W H gathered) and what that is of the HBM rate, and writes profiles/match_filters_time.json."""
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


def filters_main(reps):
    import match_verify_ref as vr
    L = bfa.lib()
    W, H = 80, 60
    base = mr.make_images(1, [KEYS] * 12)[0]
    frames = [vr.render_room(mr.pose(k), W, H) for k in range(12)]
    timer = C.c_void_p()
    bfa.check(L.bf_timer_create(C.byref(timer)))
    ms = C.c_float()
    result = {"keys_per_image": KEYS, "reps": reps, "cache_frame": [W, H]}
    for earlier, valid in ((10, 10), (500, 500), (500, 10)):
        m = bfa.Matcher(bfa.matcher_options(earlier + 1, KEYS, mr.intrinsics_inv()))
        for i in range(earlier + 1):
            m.add_image(*base[i % len(base)])
        for i in range(earlier + 1):
            m.set_valid(i, i >= earlier - valid)
        cache = bfa.CacheFrames.from_host([frames[i % 12] for i in range(earlier + 1)], vr.cache_intrinsics(W, H))
        cur = earlier
        m.match(cur, 0)
        m.filter(cur, 0)
        nonempty = sum(m.filtered_matches(p)[0] > 0 for p in range(earlier))
        times = {"surface_area": [], "dense_verify": []}
        for r in range(reps + 3):  # 3 warm-up rounds
            for name, fn in (("surface_area", lambda: m.filter_surface_area(cur, 0)),
                             ("dense_verify", lambda: m.filter_dense_verify(cur, 0, cache))):
                m.filter(cur, 0)
                bfa.check(L.bf_matcher_timer_start(m.h, timer))
                fn()
                bfa.check(L.bf_matcher_timer_stop(m.h, timer, C.byref(ms)))
                if r >= 3:
                    times[name].append(ms.value)
        kept = sum(m.filtered_matches(p)[0] > 0 for p in range(earlier))
        dv = float(np.median(times["dense_verify"]))
        requested = nonempty * 2 * 2 * 36 * W * H
        result[f"vs_{earlier}_valid_{valid}"] = {
            "pairs": earlier, "non_empty_pairs": int(nonempty), "kept_after_dense_verify": int(kept),
            "surface_area_ms": round(float(np.median(times["surface_area"])), 4),
            "surface_area_ms_min": round(float(np.min(times["surface_area"])), 4),
            "dense_verify_ms": round(dv, 4), "dense_verify_ms_min": round(float(np.min(times["dense_verify"])), 4),
            "dense_verify_bytes_requested": requested,
            "dense_verify_fraction_of_hbm_bandwidth": requested / (dv * 1e-3) / PEAK_HBM}
        m.close()
    line = json.dumps(result)
    print(line)
    with open(os.path.join(REPO, "profiles", "match_filters_time.json"), "w") as f:
        f.write(line + "\n")


def main():
    if "--filters" in sys.argv:
        rest = [a for a in sys.argv[1:] if a != "--filters"]
        return filters_main(int(rest[0]) if rest else 20)
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
