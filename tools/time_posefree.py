"""Host wall time per bf_recon_process_frame of the pose-free loop (a bundler attached, bf_recon_attach_bundler) on one
GPU, at 640 x 480 (sift_ref's `product` scene) and 320 x 240 (`medium`), submapSize 10, views rendered at pose(k); ordinary
frames and boundary frames (f > 0, f % 10 == 0: the local solve, the fuse, the global solve, all host-ordered) apart.
Beside them, for the same frames: bf_bundler_process_frame alone, and the loop alone without a bundler, which gets what the
attached run produced (the sift chain as its frame-to-frame estimates, each submap's EntryJ list, the global list, cache
frames built by a CUDACache of its own) and so runs the same solves. 5 warm-up frames, then median and minimum. Nothing
overlaps in the synchronous form, so the attached loop is expected at about the sum of the other two.
Prints one JSON line and writes profiles/posefree_time.json.
Usage: python tools/time_posefree.py [frames]"""
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
from bundlefusion_amd.recon import Recon, bundler_cache_intrinsics, recon_options  # noqa: E402

WARMUP, SUBMAP = 5, 10


def bundler_options(name, max_keyframes):
    f = R.FIXTURES[name]
    fx, fy, cx, cy = R.camera(f["w"], f["h"])
    kinv = R.intrinsics_inv(f["w"], f["h"])
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = fx, fy, cx, cy
    return bfa.bundler_options(bfa.sift_options(f["w"], f["h"], f["dw"], f["dh"]), bfa.matcher_options(0, 1024, kinv),
                               bfa.matcher_options(0, 1024, kinv), cache_options(f["dw"], f["dh"], fx, fy, cx, cy, 0), K,
                               submap_size=SUBMAP, max_keyframes=max_keyframes)


def camera(name):
    f = R.FIXTURES[name]
    fx, fy, cx, cy = R.camera(f["w"], f["h"])
    return bfa.depth_camera(f["w"], f["h"], fx=fx, fy=fy, mx=cx, my=cy)


def loop(name, bo, frames):
    params = bfa.hash_params(voxel_size=0.01, num_buckets=1 << 18, num_blocks=1 << 17)
    o = recon_options(frames, submapSize=SUBMAP, cacheWidth=bo.cache.width, cacheHeight=bo.cache.height,
                      cacheIntrinsics=bundler_cache_intrinsics(bo), maxKeyframes=bo.maxKeyframes, asyncBundling=0)
    return Recon(params, camera(name), o)


def split(ms):
    """(ordinary, boundary) median and minimum over the frames after the warm-up."""
    out = {}
    for kind, pick in (("ordinary", lambda f: f % SUBMAP != 0), ("boundary", lambda f: f % SUBMAP == 0)):
        v = [ms[f] for f in range(WARMUP, len(ms)) if pick(f)]
        out[kind] = dict(frames=len(v), wall_ms=round(float(np.median(v)), 4), wall_ms_min=round(float(np.min(v)), 4))
    return out


def time_attached(name, dev, frames, max_keyframes):
    bo = bundler_options(name, max_keyframes)
    b, rc = bfa.Bundler(bo), loop(name, bo, frames)
    rc.attach_bundler(b)
    ms, subs = [], []
    for f, (dc, dd) in enumerate(dev):
        rc.set_frame(f, dd.ptr.value, dc.ptr.value)
        rc.set_frame_bundling(f, dc, dd)
        t0 = time.perf_counter()
        rc.process_frame(f)
        ms.append((time.perf_counter() - t0) * 1e3)
        if f > 0 and f % SUBMAP == 0:
            subs.append(b.submap()["corr"])  # read back outside the timed region, before the next submap closes
    rc.synchronize()
    bst, st = rc.bundling_stats(), rc.stats()
    recs = [rc.bundler_frame(f) for f in range(frames)]
    glob = b.global_list()
    out = split(ms)
    out.update(bundler_ms_per_frame=round(bst["bundlerMs"] / bst["frames"], 4), host_wait_ms_per_frame=round(st["hostWaitMs"] / frames, 4),
               submaps_fused=bst["submapsFused"], frames_not_integrated=bst["framesNotIntegrated"], keyframes_lost=bst["keyframesLost"],
               local_solves=st["localSolves"], global_solves=st["globalSolves"])
    rc.close()
    b.close()
    return out, recs, subs, glob


def time_bundler_alone(name, dev, max_keyframes):
    b = bfa.Bundler(bundler_options(name, max_keyframes))
    ms = []
    for dc, dd in dev:
        t0 = time.perf_counter()
        r = b.process_frame(dc, dd)
        ms.append((time.perf_counter() - t0) * 1e3)
        if r["submapClosed"]:
            b.invalid_submap()  # takes the closed submap; outside the timed region
    b.close()
    return split(ms)


def time_loop_alone(name, dev, frames, max_keyframes, recs, subs, glob):
    f = R.FIXTURES[name]
    bo = bundler_options(name, max_keyframes)
    rc = loop(name, bo, frames)
    fx, fy, cx, cy = R.camera(f["w"], f["h"])
    cache = CUDACache(cache_options(f["dw"], f["dh"], fx, fy, cx, cy, frames, width=bo.cache.width, height=bo.cache.height))
    keep = []
    for k, (dc, dd) in enumerate(dev):
        cache.storeFrame(dd, dc, f["w"], f["h"])
        prev = recs[k - 1]["siftPose"].astype(np.float64) if k else np.eye(4)
        tinc = (np.linalg.inv(prev) @ recs[k]["siftPose"].astype(np.float64)).astype(np.float32)
        rc.set_frame(k, dd.ptr.value, dc.ptr.value, cache.frame(k), tinc)
    cache.synchronize()
    for s, corr in enumerate(subs):
        if len(corr):
            keep.append(bfa.DeviceArray.from_host(corr))
            rc.set_local_correspondences(s, keep[-1].ptr.value, len(corr))
    if len(glob["corr"]):
        keep.append(bfa.DeviceArray.from_host(glob["corr"]))
        rc.set_global_correspondences(keep[-1].ptr.value, len(glob["corr"]), glob["prefix"])
    ms = []
    for k in range(frames):
        t0 = time.perf_counter()
        rc.process_frame(k)
        ms.append((time.perf_counter() - t0) * 1e3)
    rc.synchronize()
    st = rc.stats()
    out = split(ms)
    out.update(local_solves=st["localSolves"], global_solves=st["globalSolves"])
    rc.close()
    cache.close()
    return out


def main():
    frames = int(sys.argv[1]) if len(sys.argv) > 1 else 2 * SUBMAP + 3
    assert frames > SUBMAP + WARMUP
    max_keyframes = (frames - 1) // SUBMAP + 2
    result = {"frames": frames, "warmup": WARMUP, "submapSize": SUBMAP}
    for name in ("product", "medium"):
        f = R.FIXTURES[name]
        sc = R.scene(name)
        dev = []
        for k in range(frames):
            color, depth = sc.render_color(R.pose(k), f["w"], f["h"], f["dw"], f["dh"])
            dev.append((bfa.DeviceArray.from_host(color), bfa.DeviceArray.from_host(depth)))
        attached, recs, subs, glob = time_attached(name, dev, frames, max_keyframes)
        alone = time_bundler_alone(name, dev, max_keyframes)
        plain = time_loop_alone(name, dev, frames, max_keyframes, recs, subs, glob)
        result[f"{f['w']}x{f['h']}"] = {"attached_loop": attached, "bundler_alone": alone, "loop_alone": plain}
    line = json.dumps(result)
    print(line)
    with open(os.path.join(REPO, "profiles", "posefree_time.json"), "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
