"""Standalone timing of key fusing (bf_match_fuse_to_global) on one GPU, at the loop's size - a submap of 11 images x
1 024 keys with 55 pairs x 25 = 1 375 records - and at 11 x 256 keys / 300 records. The records join the same landmark
in two images (25 random landmarks per pair; the small leg takes the first 300 of 6 per pair), a fifth of them with
an error above the 0.03 m threshold and a twentieth invalidated, under transforms near the identity
(tests/fuse_ref.py's generators). The global store is emptied before every call, outside the timed region.

Two figures per leg, warmed up, median and minimum of `reps` calls: device-event time on the local matcher's stream
around the call (the one kernel and the read-back of the counts), and host wall time of the call, which ends in the
stream synchronise and is what the bundling thread waits for. Prints one JSON line and writes
profiles/match_fuse_time.json. Usage: python tools/time_fuse.py [reps]"""
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
import fuse_ref as fr  # noqa: E402

IMAGES = 11


def workload(keys_per_image, per_pair, seed=3):
    """(keys, descs, offsets, corr, key_idx, transforms): key l of every image sees landmark l."""
    rng = np.random.default_rng(seed)
    counts = [keys_per_image] * IMAGES
    keys, descs, off = fr.store(rng, counts)
    E = []
    for i in range(IMAGES):
        for j in range(i + 1, IMAGES):
            for l in rng.permutation(keys_per_image)[:per_pair]:
                E.append((int(off[i] + l), int(off[j] + l), fr.FAR if rng.random() < 0.2 else fr.GOOD))
    T = fr.small_transforms(rng, IMAGES)
    corr, key_idx = fr.records(rng, T, E, off, counts)
    corr["i"][rng.permutation(len(E))[: len(E) // 20]] = fr.NONE
    return keys, descs, off, corr, key_idx, T


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    L = bfa.lib()
    timer = C.c_void_p()
    bfa.check(L.bf_timer_create(C.byref(timer)))
    ms = C.c_float()
    result = {"images": IMAGES, "reps": reps}
    for keys_per_image, records in ((1024, 1375), (256, 300)):
        per_pair = -(-records // 55)
        keys, descs, off, corr, key_idx, T = workload(keys_per_image, per_pair)
        corr, key_idx = corr[:records], key_idx[:records]
        local = bfa.Matcher(bfa.matcher_options(IMAGES, keys_per_image, fuse_max_corr=records))
        for i in range(IMAGES):
            local.add_image(keys[off[i]:off[i] + keys_per_image], descs[off[i]:off[i] + keys_per_image])
        glob = bfa.Matcher(bfa.matcher_options(2, 1024))
        d_corr, d_idx, d_T = bfa.DeviceArray.from_host(corr), bfa.DeviceArray.from_host(key_idx), bfa.DeviceArray.from_host(T)
        K = fr.intrinsics()
        dev, wall, out = [], [], None
        for r in range(reps + 5):  # 5 warm-up calls
            glob.reset()
            glob.synchronize()
            bfa.check(L.bf_matcher_timer_start(local.h, timer))
            t0 = time.perf_counter()
            out = local.fuse_to_global(glob, d_corr, d_idx, records, d_T, K)
            t1 = time.perf_counter()
            bfa.check(L.bf_matcher_timer_stop(local.h, timer, C.byref(ms)))
            if r >= 5:
                dev.append(ms.value)
                wall.append((t1 - t0) * 1e3)
        result[f"keys_{keys_per_image}_records_{records}"] = {
            "keys": IMAGES * keys_per_image, "records": records, "fused_keys": out[1], "tracks": out[2],
            "device_ms": round(float(np.median(dev)), 4), "device_ms_min": round(float(np.min(dev)), 4),
            "host_wall_ms": round(float(np.median(wall)), 4), "host_wall_ms_min": round(float(np.min(wall)), 4)}
        local.close()
        glob.close()
    line = json.dumps(result)
    print(line)
    with open(os.path.join(REPO, "profiles", "match_fuse_time.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
