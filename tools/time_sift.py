"""Standalone timing of the SIFT detector (bf_sift_intensity + bf_sift_detect) on one GPU, at the product shape
640 x 480 and at 320 x 240, on the analytic textured scene of tests/sift_ref.py. Device-event times on the detector's
stream, warmed up, median and minimum of `reps` calls; a detect is queued whole (24 launches, no host round trip), so
the event pair spans exactly the device work. Also the host wall time of detect + result (the call that hands the
count to the host). Prints one JSON line with the key counts and writes profiles/sift_time.json.
Usage: python tools/time_sift.py [reps]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import bundlefusion_amd as bfa  # noqa: E402
import sift_ref as R  # noqa: E402


def timed(s, timer, fn, reps):
    L = bfa.lib()
    ms = C.c_float()
    out = []
    for _ in range(reps):
        bfa.check(L.bf_sift_timer_start(s.h, timer))
        fn()
        bfa.check(L.bf_sift_timer_stop(s.h, timer, C.byref(ms)))
        out.append(ms.value)
    return round(float(np.median(out)), 4), round(float(np.min(out)), 4)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    L = bfa.lib()
    timer = C.c_void_p()
    bfa.check(L.bf_timer_create(C.byref(timer)))
    result = {"reps": reps}
    for name in ("product", "medium"):
        f = R.FIXTURES[name]
        color, depth = R.scene(name).render_color(R.pose(0), f["w"], f["h"], f["dw"], f["dh"])
        s = bfa.Sift(bfa.sift_options(f["w"], f["h"], f["dw"], f["dh"]))
        dc, dd = bfa.DeviceArray.from_host(color), bfa.DeviceArray.from_host(depth)
        for _ in range(3):  # warm-up
            s.intensity(dc)
            s.detect(None, dd)
        s.synchronize()
        intensity_ms, _ = timed(s, timer, lambda: s.intensity(dc), reps)
        detect_ms, detect_min = timed(s, timer, lambda: s.detect(None, dd), reps)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s.detect(None, dd)
            n = s.result_device()[2]
            wall.append((time.perf_counter() - t0) * 1e3)
        raw, kept = s.level_counts()
        result[f"{f['w']}x{f['h']}"] = {
            "intensity_ms": intensity_ms, "detect_ms": detect_ms, "detect_ms_min": detect_min,
            "detect_plus_result_wall_ms": round(float(np.median(wall)), 4), "launches_per_detect": 24,
            "raw_keys": int(raw.sum()), "final_keys": int(n), "raw_per_level": raw.tolist(), "kept_per_level": kept.tolist()}
        s.close()
    line = json.dumps(result)
    print(line)
    with open(os.path.join(REPO, "profiles", "sift_time.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
