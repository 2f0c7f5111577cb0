"""GPU checks of the pose-free loop: a bundler attached to bf_recon_* (bf_recon_attach_bundler), synchronous form.

Fixture: sift_ref's `medium` scene (320 x 240), views pose(0..6), submapSize 3: the frames tests/test_bundler_gpu.py uses, so
two submaps and two key frames, ending on a boundary; a second stream of pose(0..9) gives three key frames and global
solves over two and three. The scene is test_recon_gpu.run_loop's at 1 cm voxels, recordOps = 1. The same images are the
integration images and the bundling images. Every loop runs once (module scope) and the tests read it."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa
import bundler_ref as B
import sift_ref as R
from bundlefusion_amd.recon import FIX_DEINTEGRATE, FIX_INTEGRATE, OP_GC, Recon, bundler_cache_intrinsics, recon_options
from oracle_lib import OracleScene
from test_bundler import options
from tsdf_compare import compare_states

pytestmark = pytest.mark.gpu
BF_ERR_ARG, BF_ERR_STATE = -2, -4
S = 3
I4 = np.eye(4, dtype=np.float32)


def camera():
    f = R.FIXTURES["medium"]
    fx, fy, cx, cy = R.camera(f["w"], f["h"])
    return bfa.depth_camera(f["w"], f["h"], fx=fx, fy=fy, mx=cx, my=cy)


def upload(views):
    return [(bfa.DeviceArray.from_host(np.ascontiguousarray(c)), bfa.DeviceArray.from_host(np.ascontiguousarray(d))) for c, d, *_ in views]


def loop_options(bo, F, **kw):
    return recon_options(F, recordOps=1, submapSize=S, cacheWidth=bo.cache.width, cacheHeight=bo.cache.height,
                         cacheIntrinsics=bundler_cache_intrinsics(bo), maxKeyframes=bo.maxKeyframes, asyncBundling=0, **kw)


def same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def run_posefree(dev, host, drain=30, **kw):
    """The five calls per frame of a pose-free caller; per frame the trajectory row as first integrated and the record,
    per boundary the attached bundler's closed submap (read before the next one closes)."""
    F = len(dev)
    params = bfa.hash_params(voxel_size=0.01, num_buckets=1 << 16, num_blocks=1 << 15)
    bo = options("medium", S)
    b = bfa.Bundler(bo)
    rc = Recon(params, camera(), loop_options(bo, F, **kw))
    rc.attach_bundler(b)
    first, subs = [], []
    for f, (dc, dd) in enumerate(dev):
        rc.set_frame(f, dd.ptr.value, dc.ptr.value)
        rc.set_frame_bundling(f, dc, dd)
        rc.process_frame(f)
        first.append(rc.trajectory(f + 1)[f].copy())
        if f > 0 and f % S == 0:
            subs.append(b.submap())
    rc.finish()
    for _ in range(drain):
        rc.reintegrate()
    rc.synchronize()
    recs = [rc.bundler_frame(f) for f in range(F)]
    nsub = (F - 1) // S
    return dict(rc=rc, b=b, bo=bo, params=params, F=F, dev=dev, host=host, first=first, subs=subs, recs=recs,
                glob=b.global_list(), trace=rc.queue_trace(), ops=rc.op_log(), stats=rc.stats(), bst=rc.bundling_stats(),
                poses=[rc.submap_poses(s, bo.maxKeyframes, S) for s in range(nsub)], traj=rc.trajectory(F),
                opt=rc.optimized_trajectory(), blocks=rc.export_blocks(), bstats=b.stats())


def replay(run):
    """A stand-alone bundler driven by hand from the loop's outputs: the same frames, bf_bundler_fuse_submap with
    bf_recon_submap_poses(s).local, then bf_bundler_set_complete_trajectory with the s-th kind-1 event of the queue trace
    and lastValidCompleteTransform = S * s."""
    b = bfa.Bundler(run["bo"])
    updates = [T for kind, _, T in run["trace"] if kind == 1]
    recs, subs = [], []
    for f, (dc, dd) in enumerate(run["dev"]):
        recs.append(b.process_frame(dc, dd))
        if recs[-1]["submapClosed"]:
            s = len(subs)
            subs.append(b.submap())
            local, _, valid, ok = run["poses"][s]
            assert ok and valid[s]
            b.fuse_submap(local)
            b.set_complete_trajectory(updates[s], S * s)
    out = dict(recs=recs, subs=subs, glob=b.global_list())
    b.close()
    return out


def local_init(recs, s, valid):
    """Tlocal of a submap's frames: inv(sift[first]) * sift[f], rigid inverse and product in double, rounded once; image 0
    the identity, an invalid image -inf."""
    A = recs[s * S]["siftPose"].astype(np.float64)
    inv = np.zeros((4, 4))
    inv[:3, :3] = A[:3, :3].T
    for i in range(3):
        inv[i, 3] = -((A[0, i] * A[0, 3] + A[1, i] * A[1, 3]) + A[2, i] * A[2, 3])
    inv[3, 3] = 1.0
    out = np.full((len(valid), 4, 4), -np.inf, np.float32)
    out[0] = I4
    for k in range(1, len(valid)):
        if valid[k]:
            Bm = recs[s * S + k]["siftPose"].astype(np.float64)
            for r in range(4):
                for c in range(4):
                    acc = 0.0
                    for j in range(4):
                        acc += inv[r, j] * Bm[j, c]
                    out[k, r, c] = np.float32(acc)
    return out


@pytest.fixture(scope="module")
def frames():
    views = B.views("medium", 10)
    other = B.views("medium", 7, 99)
    return dict(host=views, dev=upload(views), other_host=other, other=upload(other))


@pytest.fixture(scope="module")
def seven(frames):
    run = run_posefree(frames["dev"][:7], frames["host"][:7])
    run["again"] = run_posefree(frames["dev"][:7], frames["host"][:7])
    return run


@pytest.fixture(scope="module")
def ten(frames):
    return run_posefree(frames["dev"], frames["host"])


def test_poses_are_the_bundlers(seven, ten):
    for run in (seven, ten):
        added = {f: T for kind, f, T in run["trace"] if kind == 0}
        for f in range(run["F"]):
            r = run["recs"][f]
            assert r["valid"] and r["frame"] == f
            same(run["first"][f], r["integrateTransform"], f"frame {f}: bf_recon_trajectory as first integrated")
            same(added[f], r["integrateTransform"], f"frame {f}: addFrame")
        same(run["first"][0], I4, "frame 0 is the identity")
        first_int = {}
        for kind, f, _, newT in run["ops"]:
            if kind == FIX_INTEGRATE and f not in first_int:
                first_int[f] = newT
        for f in range(run["F"]):
            same(first_int[f].reshape(4, 4), run["recs"][f]["integrateTransform"], f"frame {f}: the scene call")
    # lastValidCompleteTransform is S * s: 0 after submap 0 (case one, the sift chain), 3 after submap 1, so frames 7.. of
    # the longer stream were integrated through the complete trajectory (case three)
    assert all(ten["recs"][f]["integrateTransform"].tobytes() == ten["recs"][f]["siftPose"].tobytes() for f in range(0, 7))
    assert all(ten["recs"][f]["integrateTransform"].tobytes() != ten["recs"][f]["siftPose"].tobytes() for f in range(7, 10))


def test_the_loop_drove_the_bundler_as_a_hand_would(seven, ten):
    for run in (seven, ten):
        nsub = (run["F"] - 1) // S
        assert run["stats"]["removedPairs"] == 0  # else the loop's solves changed the global list in place
        hand = replay(run)
        for f in range(run["F"]):
            for k, v in run["recs"][f].items():
                same(np.asarray(v), np.asarray(hand["recs"][f][k]), f"frame {f} record field {k}")
        assert len(run["subs"]) == len(hand["subs"]) == nsub
        for s in range(nsub):
            a, h = run["subs"][s], hand["subs"][s]
            assert a["submap"] == h["submap"] == s and a["frames"] == h["frames"] == S + 1 and a["is_valid"] and h["is_valid"]
            assert len(a["corr"]) > 0
            same(a["corr"], h["corr"], f"submap {s} EntryJ")
            same(a["key_idx"], h["key_idx"], f"submap {s} key indices")
            same(a["valid"], h["valid"], f"submap {s} valid flags")
            same(a["device_valid"], h["device_valid"], f"submap {s} device valid flags")
        same(run["glob"]["corr"], hand["glob"]["corr"], "global EntryJ")
        same(run["glob"]["key_idx"], hand["glob"]["key_idx"], "global key indices")
        same(run["glob"]["prefix"], hand["glob"]["prefix"], "prefix[]")
        assert len(run["glob"]["prefix"]) == nsub and run["glob"]["prefix"][-1] == len(run["glob"]["corr"]) > 0
        st, bst = run["stats"], run["bst"]
        assert bst["frames"] == run["F"] == run["bstats"]["frames"] and bst["submapsFused"] == nsub == run["bstats"]["keyframes"]
        assert bst["framesNotIntegrated"] == bst["submapsInvalidEarly"] == bst["submapsInvalidVerified"] == 0
        assert bst["keyframesLost"] == bst["keyframesCleared"] == 0 and bst["bundlerMs"] > 0
        assert st["localSolves"] == nsub and st["globalSolves"] == nsub - 1 and st["invalidLocals"] == 0
    assert ten["stats"]["globalSolves"] == 2  # over two and over three key frames


def test_the_solves_are_the_stand_alone_solvers(frames):
    """useLocalDense = 0, disableLocalVerify = 1: each submap's local poses against bf_solver_solve of the replay bundler's
    list with the same initial poses, iteration counts and weights."""
    from bundlefusion_amd.solver import SolverBundling
    run = run_posefree(frames["dev"][:7], frames["host"][:7], drain=0, useLocalDense=0, disableLocalVerify=1)
    hand = replay(run)
    solver = SolverBundling(S + 1, 25 * (S + 1) * S // 2)
    for s in range(2):
        sub = hand["subs"][s]
        init = local_init(hand["recs"], s, sub["valid"])
        d_T = bfa.DeviceArray.from_host(init)
        rot, trans = bfa.DeviceArray.from_host(np.zeros((S + 1, 3), np.float32)), bfa.DeviceArray.from_host(np.zeros((S + 1, 3), np.float32))
        valid = bfa.DeviceArray.from_host(sub["valid"].astype(np.int32))
        corr = bfa.DeviceArray.from_host(sub["corr"])
        solver.matrices_to_poses(d_T, S + 1, rot, trans, valid)
        solver.solve(corr, len(sub["corr"]), valid, S + 1, 2, 100, [1.0, 1.0], rot=rot, trans=trans, find_max_residual=False)
        assert solver.result()["error"] == 0
        solver.poses_to_matrices(rot, trans, S + 1, d_T, valid)
        solver.synchronize()
        local = run["poses"][s][0]
        same(local, d_T.download().reshape(S + 1, 4, 4), f"submap {s} local poses")
        assert local[1:].tobytes() != init[1:].tobytes()  # the solve moved them
    solver.close()
    assert run["stats"]["localVerifications"] == 0 and run["stats"]["localSolves"] == 2
    run["rc"].close()
    run["b"].close()


def test_the_scene_is_the_op_logs(seven):
    ops = seven["ops"]
    kinds = [k for k, *_ in ops]
    assert kinds.count(FIX_INTEGRATE) >= 7 and kinds.count(OP_GC) == 7 + 30
    ora = OracleScene(seven["params"])
    cam = camera()
    for kind, f, oldT, newT in ops:
        color, depth = seven["host"][f][0], seven["host"][f][1]
        if kind == FIX_DEINTEGRATE:
            ora.integrate(oldT.reshape(4, 4), depth, color, cam, deintegrate=True)
        elif kind == FIX_INTEGRATE:
            ora.integrate(newT.reshape(4, 4), depth, color, cam)
        elif kind == OP_GC:
            ora.garbageCollect()
    assert compare_states(seven["params"], seven["rc"], ora) > 100


def test_accuracy_against_the_restatement_chain(seven):
    """Each optimised pose relative to frame 0 against sift_ref.pose; at most twice the accumulated error of the float64-
    checked restatement chain (bundler_ref.chain_reference) at the same frame, the margin the bundler's own tests give a
    float32 pipeline. Measured on the MI355X: see DESIGN §3.7."""
    ref = B.chain_reference("medium", 7, S)
    opt = seven["opt"]
    assert len(opt) == 6  # the frames the complete trajectory covers
    base = np.linalg.inv(opt[0].astype(np.float64))
    worst = []
    for f in range(1, len(opt)):
        te, re = B.pose_error(base @ opt[f].astype(np.float64), 0, f)
        rte, rre = B.pose_error(ref["sift"][f].astype(np.float64), 0, f)
        print(f"frame {f}: translation error {te:.5f} m (restatement chain {rte:.5f}), rotation error {re:.6f} rad "
              f"(restatement chain {rre:.6f})")
        worst.append((f, te, 2 * rte, re, 2 * rre))
    for f, te, tb, re, rb in worst:
        assert te <= tb and re <= rb, (f, te, tb, re, rb)


def edge_frames(frames, kind):
    dev, host = list(frames["dev"][:7]), list(frames["host"][:7])
    if kind == "no_depth":
        bad = np.full(host[2][1].shape, -np.inf, np.float32)
        dev[2] = (dev[2][0], bfa.DeviceArray.from_host(bad))
        host[2] = (host[2][0], bad)
    elif kind == "submap0_other_scene":  # frames 1.. from another scene: nothing in submap 0 matches frame 0
        dev[1:], host[1:] = frames["other"][1:7], frames["other_host"][1:7]
    elif kind == "submap1_other_scene":  # frames 3.. : submap 1 is consistent in itself and matches no earlier key frame
        dev[3:], host[3:] = frames["other"][3:7], frames["other_host"][3:7]
    return dev, host


def test_edge_frame_without_depth(frames):
    run = run_posefree(*edge_frames(frames, "no_depth"))
    r = run["recs"][2]
    assert not r["valid"] and np.all(np.isneginf(r["integrateTransform"]))
    added = {f: T for kind, f, T in run["trace"] if kind == 0}
    assert np.all(np.isneginf(added[2])) and np.all(np.isneginf(run["first"][2]))  # NotIntegrated_NoTransform
    assert all(op[1] != 2 for op in run["ops"] if op[0] != OP_GC)  # never in the op log
    sub = run["subs"][0]
    assert sub["valid"].tolist() == sub["device_valid"].tolist() == [1, 1, 0, 1] and sub["is_valid"]
    local, _, valid, ok = run["poses"][0]
    assert ok and valid[0] and np.all(np.isneginf(local[2])) and np.all(np.isfinite(local[[0, 1, 3]]))
    assert np.all(np.isneginf(run["opt"][2])) and np.all(np.isfinite(run["opt"][[0, 1, 3, 4, 5]]))
    assert np.all(np.isneginf(run["traj"][2])) and np.all(np.isfinite(run["traj"][[0, 1, 3, 4, 5, 6]]))
    bst, st = run["bst"], run["stats"]
    assert bst["frames"] == 7 and bst["framesNotIntegrated"] == 1 and bst["submapsFused"] == 2
    assert bst["submapsInvalidEarly"] == bst["submapsInvalidVerified"] == bst["keyframesLost"] == bst["keyframesCleared"] == 0
    assert st["localSolves"] == 2 and st["globalSolves"] == 1 and st["invalidLocals"] == 0
    run["rc"].close()
    run["b"].close()


def test_edge_first_submap_invalid(frames):
    run = run_posefree(*edge_frames(frames, "submap0_other_scene"))
    assert [r["valid"] for r in run["recs"]] == [1, 0, 0, 0, 1, 1, 1]
    s0, s1 = run["subs"]
    assert not s0["is_valid"] and s0["valid"].tolist() == [1, 0, 0, 0] and len(s0["corr"]) == 0
    assert s1["is_valid"] and s1["valid"].tolist() == [1, 1, 1, 1] and len(s1["corr"]) > 0  # submap 1 still processed
    _, _, valid0, ok0 = run["poses"][0]
    local1, _, valid1, ok1 = run["poses"][1]
    assert not ok0 and not valid0[0]  # no local solve, the key frame invalid
    assert not ok1 and valid1.tolist() == [0, 0] and np.all(np.isfinite(local1))  # solved, then lost at the global match
    assert len(run["glob"]["corr"]) == 0 and run["glob"]["prefix"].tolist() == [0, 0]  # no record of it in the global list
    ops = [(k, f) for k, f, *_ in run["ops"] if k != OP_GC]
    assert (FIX_INTEGRATE, 0) in ops and (FIX_DEINTEGRATE, 0) in ops  # its frames de-integrated by the queue
    assert all(f not in (1, 2, 3) for _, f in ops)
    assert np.all(np.isneginf(run["opt"])) and np.all(np.isneginf(run["traj"][:6]))
    bst, st = run["bst"], run["stats"]
    assert bst["frames"] == 7 and bst["framesNotIntegrated"] == 3 and bst["submapsInvalidEarly"] == 1
    assert bst["submapsFused"] == 1 and bst["keyframesLost"] == 1 and bst["submapsInvalidVerified"] == bst["keyframesCleared"] == 0
    assert st["localSolves"] == 1 and st["globalSolves"] == 0 and st["invalidLocals"] == 2
    assert run["bstats"]["keyframes"] == 2
    run["rc"].close()
    run["b"].close()


def test_edge_second_submap_lost(frames):
    run = run_posefree(*edge_frames(frames, "submap1_other_scene"))
    assert [r["valid"] for r in run["recs"]] == [1, 1, 1, 0, 1, 1, 1]
    s0, s1 = run["subs"]
    assert s0["is_valid"] and s0["valid"].tolist() == [1, 1, 1, 0] and s1["is_valid"] and s1["valid"].tolist() == [1, 1, 1, 1]
    _, _, valid0, ok0 = run["poses"][0]
    _, glob1, valid1, ok1 = run["poses"][1]
    assert ok0 and valid0[0] and not ok1 and valid1.tolist() == [1, 0]  # the fuse reported valid == 0: the gate is 0
    assert len(run["glob"]["corr"]) == 0 and run["glob"]["prefix"].tolist() == [0, 0]
    assert np.all(np.isfinite(run["opt"][:3])) and np.all(np.isneginf(run["opt"][3:]))  # its frames go to -inf
    assert np.all(np.isneginf(run["traj"][3:6]))  # and out of the scene
    bst, st = run["bst"], run["stats"]
    assert bst["frames"] == 7 and bst["framesNotIntegrated"] == 1 and bst["submapsFused"] == 2 and bst["keyframesLost"] == 1
    assert bst["submapsInvalidEarly"] == bst["submapsInvalidVerified"] == bst["keyframesCleared"] == 0
    assert st["localSolves"] == 2 and st["globalSolves"] == 0 and st["invalidLocals"] == 1  # no global solve ran
    run["rc"].close()
    run["b"].close()


def test_two_runs_are_bit_identical(seven):
    a, b = seven, seven["again"]
    same(a["traj"], b["traj"], "trajectory")
    same(a["opt"], b["opt"], "optimised trajectory")
    for f in range(7):
        same(a["first"][f], b["first"][f], f"frame {f}")
    assert len(a["ops"]) == len(b["ops"])
    for x, y in zip(a["ops"], b["ops"]):
        assert x[0] == y[0] and x[1] == y[1]
        same(x[2], y[2])
        same(x[3], y[3])
    for s in range(2):
        same(a["subs"][s]["corr"], b["subs"][s]["corr"], f"submap {s} EntryJ")
        same(a["subs"][s]["key_idx"], b["subs"][s]["key_idx"], f"submap {s} key indices")
        for u, v in zip(a["poses"][s][:3], b["poses"][s][:3]):
            same(u, v, f"submap {s} poses")
    for k in ("corr", "key_idx", "prefix"):
        same(a["glob"][k], b["glob"][k], f"global {k}")
    ba, bb = a["blocks"], b["blocks"]  # the heap slots follow the GC's atomic push order: compare the block set
    key = lambda x: sorted(map(tuple, x[x[:, 3] != 0][:, :3].tolist()))
    assert key(ba) == key(bb) and len(key(ba)) > 100


def small_loop(bo, **kw):
    params = bfa.hash_params(voxel_size=0.02, num_buckets=1 << 10, num_blocks=1 << 10)
    o = loop_options(bo, 8)
    for k, v in kw.items():
        if k == "cacheIntrinsics":
            o.cacheIntrinsics[:] = [float(x) for x in v]
        else:
            setattr(o, k, v)
    return Recon(params, camera(), o)


def code_of(fn, *a):
    with pytest.raises(bfa.BFError) as e:
        fn(*a)
    return e.value.code


def test_attach_rejections(frames):
    bo = options("medium", S)
    b = bfa.Bundler(bo)
    fx, fy, mx, my = bundler_cache_intrinsics(bo)
    for kw in (dict(asyncBundling=1), dict(submapSize=4), dict(maxKeyframes=5), dict(cacheWidth=40), dict(cacheHeight=30),
               dict(cacheIntrinsics=(fx + 1, fy, mx, my)), dict(cacheIntrinsics=(fx, fy, mx, my + 0.5)),
               dict(maxLocalCorr=149), dict(maxGlobalCorr=149)):
        rc = small_loop(bo, **kw)
        assert code_of(rc.attach_bundler, b) == BF_ERR_ARG, kw
        rc.close()
    rc = small_loop(bo)
    rc.set_initial_pose(I4)
    assert code_of(rc.attach_bundler, b) == BF_ERR_STATE
    rc.close()
    b.set_retry(True)
    rc = small_loop(bo)
    assert code_of(rc.attach_bundler, b) == BF_ERR_STATE
    b.set_retry(False)
    # a frame has been processed: by the bundler, or by the loop
    dc, dd = frames["dev"][0]
    b.process_frame(dc, dd)
    assert code_of(rc.attach_bundler, b) == BF_ERR_STATE
    b.reset()
    rc.set_frame(0, dd.ptr.value, dc.ptr.value)
    rc.process_frame(0)
    assert code_of(rc.attach_bundler, b) == BF_ERR_STATE
    rc.close()
    # no bundler attached
    rc = small_loop(bo)
    assert code_of(rc.bundler_frame, 0) == BF_ERR_ARG and code_of(rc.set_frame_bundling, 0, dc, dd) == BF_ERR_STATE
    assert all(v == 0 for v in rc.bundling_stats().values())
    rc.attach_bundler(b)
    assert code_of(rc.attach_bundler, b) == BF_ERR_STATE
    assert code_of(rc.bundler_frame, 0) == BF_ERR_ARG  # not processed yet
    for fn, a in ((rc.end_sequence, ()), (rc.end_solve, ()), (rc.set_comm, (None,)), (rc.attach_cache, (None,)),
                  (rc.attach_preproc, (None,)), (rc.set_initial_pose, (I4,))):
        assert code_of(fn, *a) == BF_ERR_STATE, fn.__name__
    rc.set_frame(0, dd.ptr.value, dc.ptr.value)
    assert code_of(rc.process_frame, 0) == BF_ERR_STATE  # no bundling images for the frame
    rc.close()
    b.close()
