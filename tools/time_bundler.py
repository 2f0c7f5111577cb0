"""Standalone timing of the bundler's frame (bf_bundler_process_frame) on one GPU, at 640 x 480 (sift_ref's `product`
scene) and at 320 x 240 (`medium`), submapSize 10, views rendered at pose(k). Per frame: device-event time on the
bundler's stream and host wall time; 5 warm-up frames, then median and minimum over the rest (the run crosses one submap
close). In the same run the same frames go through the separate handles by hand (Sift.detect_into + the cache store +
match_and_filter with the dense verify + add_to_residuals + transforms), which is the path before the bundler existed;
its figure is host wall time, since its work spans three streams. A third leg (time_retry) times
bf_bundler_fuse_submap with one retry attempt against the same call with retry off, at both shapes. Prints one JSON line
and writes profiles/bundler_time.json.
Usage: python tools/time_bundler.py [frames]"""
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
from bundlefusion_amd.cache import CUDACache, cache_options  # noqa: E402
from bundlefusion_amd.match import CacheFrames  # noqa: E402

WARMUP, SUBMAP = 5, 10
NONE = 0xFFFFFFFF


def options(name):
    f = R.FIXTURES[name]
    fx, fy, cx, cy = R.camera(f["w"], f["h"])
    kinv = R.intrinsics_inv(f["w"], f["h"])
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return bfa.bundler_options(bfa.sift_options(f["w"], f["h"], f["dw"], f["dh"]), bfa.matcher_options(0, 1024, kinv),
                               bfa.matcher_options(0, 1024, kinv), cache_options(f["dw"], f["dh"], fx, fy, cx, cy, 0), K,
                               submap_size=SUBMAP, max_keyframes=4)


def stats(ms):
    ms = ms[WARMUP:]
    return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4)


def time_bundler(name, dev, timer):
    L = bfa.lib()
    b = bfa.Bundler(options(name))
    dev_ms, wall_ms, keys, added = [], [], [], []
    ms = C.c_float()
    for dc, dd in dev:
        bfa.check(L.bf_bundler_timer_start(b.h, timer))
        t0 = time.perf_counter()
        r = b.process_frame(dc, dd)
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        bfa.check(L.bf_bundler_timer_stop(b.h, timer, C.byref(ms)))
        dev_ms.append(ms.value)
        keys.append(r["numKeys"])
        added.append(r["residualsAdded"])
        if r["submapClosed"]:
            b.invalid_submap()  # takes the closed submap; outside the timed region
    st = b.stats()
    b.close()
    return dict(device_ms=stats(dev_ms)[0], device_ms_min=stats(dev_ms)[1], wall_ms=stats(wall_ms)[0], wall_ms_min=stats(wall_ms)[1],
                host_waits_per_frame=round(st["hostWaits"] / st["frames"], 3), keys=keys, residuals_added=added)


def time_by_hand(name, dev):
    f = R.FIXTURES[name]
    o = options(name)
    sift = bfa.Sift(o.sift)
    mo = bfa.matcher_options(SUBMAP + 1, 1024, R.intrinsics_inv(f["w"], f["h"]))
    co = cache_options(f["dw"], f["dh"], *[o.cache.inputIntrinsics[k] for k in (0, 5, 2, 6)], SUBMAP + 1)
    verify = bfa.match_verify_options()
    out = bfa.DeviceArray((25 * (SUBMAP + 1) * SUBMAP // 2,), bfa.abi.ENTRYJ_DTYPE)

    def fresh():
        m, c = bfa.Matcher(mo), CUDACache(co)
        return m, c, CacheFrames.from_cache(c, SUBMAP + 1)  # the table of all slots, built once per submap
    m, cache, table = fresh()
    wall_ms, added = [], []
    for fr, (dc, dd) in enumerate(dev):
        t0 = time.perf_counter()
        sift.intensity(dc)
        lf = sift.detect_into(m, None, dd)
        cache.storeFrame(dd, dc, f["w"], f["h"])
        n = 0
        if lf > 0:
            last = m.match_and_filter(lf, 0, cache=table, verify=verify)
            if last != NONE:
                n = m.add_to_residuals(lf, 0, 25 * lf, out=out)[1]
                m.transforms(last)
        else:
            cache.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        added.append(n)
        if fr > 0 and fr % SUBMAP == 0:  # the overlap frame into a fresh set; outside the timed region
            keys, descs = m.image_keys(lf)
            m2, cache2, table2 = fresh()
            m2.add_image(keys, descs)
            cache2.copyCacheFrameFrom(cache, lf)
            cache2.synchronize()
            m.close()
            cache.close()
            m, cache, table = m2, cache2, table2
    m.close()
    cache.close()
    sift.close()
    return dict(wall_ms=stats(wall_ms)[0], wall_ms_min=stats(wall_ms)[1], residuals_added=added)


RETRY_SUBMAP, RETRY_KEYFRAMES, RETRY_REPEATS = 2, 8, 4


def retry_frames(name):
    """submapSize 2, 8 key frames: key frame k is anchored at frame 2 k. Frames 2 and 3 come from another scene, so key
    frame 1 matches nothing and waits on the retry list; every later key frame sees key frame 0, is valid, and (retry on)
    tries candidate 1 against the k - 1 later images, in vain: one attempt per fuse from key frame 2 on."""
    f = R.FIXTURES[name]
    sc, other = R.scene(name), R.Scene(f["seed"] + 100, f["blobs"], f["sigma_px"], f["w"])
    dev = []
    for k in range(RETRY_SUBMAP * RETRY_KEYFRAMES + 1):
        color, depth = (other if k in (2, 3) else sc).render_color(R.pose(k), f["w"], f["h"], f["dw"], f["dh"])
        dev.append((bfa.DeviceArray.from_host(color), bfa.DeviceArray.from_host(depth)))
    return dev


def time_retry(name, dev, timer):
    """bf_bundler_fuse_submap with one retry attempt against the same call with retry off: per key frame >= 2 the device
    event time and the host wall time of the call, the median over the repeats after the first (a reset between them)."""
    import bundler_ref as B
    L = bfa.lib()
    S = RETRY_SUBMAP
    o = options(name)
    o.submapSize, o.maxKeyframes = S, RETRY_KEYFRAMES + 1
    out = {}
    for mode in ("off", "on"):
        b = bfa.Bundler(o)
        b.set_retry(mode == "on")
        dev_ms = [[] for _ in range(RETRY_KEYFRAMES)]
        wall_ms = [[] for _ in range(RETRY_KEYFRAMES)]
        waits = [[] for _ in range(RETRY_KEYFRAMES)]
        ms = C.c_float()
        for rep in range(RETRY_REPEATS):
            recs, k, report = [], 0, []
            for fr, (dc, dd) in enumerate(dev):
                recs.append(b.process_frame(dc, dd))
                if not recs[-1]["submapClosed"]:
                    continue
                base = B.rigid_inverse(recs[fr - S]["siftPose"])
                T = bfa.DeviceArray.from_host(np.stack([B.mat_mul(base, recs[fr - S + i]["siftPose"]) for i in range(S + 1)]).astype(np.float32))
                before = b.stats()["hostWaits"]
                bfa.check(L.bf_bundler_timer_start(b.h, timer))
                t0 = time.perf_counter()
                kf = b.fuse_submap(T)
                wall = (time.perf_counter() - t0) * 1e3
                bfa.check(L.bf_bundler_timer_stop(b.h, timer, C.byref(ms)))
                if rep > 0:
                    dev_ms[k].append(ms.value)
                    wall_ms[k].append(wall)
                    waits[k].append(b.stats()["hostWaits"] - before)
                report.append((kf["valid"], b.last_retry()["attempted"], b.last_retry()["revalidated"] != NONE))
                k += 1
            assert [r[0] for r in report] == [1, 0] + [1] * (RETRY_KEYFRAMES - 2), "the sequence did not lose key frame 1 alone"
            assert [r[1] for r in report] == ([0, 0] + [1] * (RETRY_KEYFRAMES - 2) if mode == "on" else [0] * RETRY_KEYFRAMES)
            assert not any(r[2] for r in report), "candidate 1 was revalidated: the two modes no longer do the same own work"
            b.reset()
        b.close()
        out[mode] = dict(device_ms=[round(float(np.median(x)), 4) for x in dev_ms], wall_ms=[round(float(np.median(x)), 4) for x in wall_ms],
                         host_waits=[int(np.max(x)) for x in waits])
    ks = range(2, RETRY_KEYFRAMES)
    out["candidate_pairs"] = [k - 1 for k in ks]  # later images the candidate is matched against at key frame k
    out["added_device_ms"] = [round(out["on"]["device_ms"][k] - out["off"]["device_ms"][k], 4) for k in ks]
    out["added_wall_ms"] = [round(out["on"]["wall_ms"][k] - out["off"]["wall_ms"][k], 4) for k in ks]
    # the attempt's host side (its launches and its one more wait): what the call gains in wall time beyond the device's
    out["added_host_ms"] = [round(w - d, 4) for w, d in zip(out["added_wall_ms"], out["added_device_ms"])]
    return out


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 13
    assert frames > WARMUP + 1
    L = bfa.lib()
    timer = C.c_void_p()
    bfa.check(L.bf_timer_create(C.byref(timer)))
    result = {"frames": frames, "warmup": WARMUP, "submapSize": SUBMAP}
    for name in ("product", "medium"):
        f = R.FIXTURES[name]
        sc = R.scene(name)
        dev = []
        for k in range(frames):
            color, depth = sc.render_color(R.pose(k), f["w"], f["h"], f["dw"], f["dh"])
            dev.append((bfa.DeviceArray.from_host(color), bfa.DeviceArray.from_host(depth)))
        hand = time_by_hand(name, dev)
        bund = time_bundler(name, dev, timer)
        assert hand["residuals_added"] == bund["residuals_added"], "the two paths disagree"
        result[f"{f['w']}x{f['h']}"] = {"bundler": bund, "separate_handles": hand, "fuse_retry": time_retry(name, retry_frames(name), timer)}
    line = json.dumps(result)
    print(line)
    with open(os.path.join(REPO, "profiles", "bundler_time.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
