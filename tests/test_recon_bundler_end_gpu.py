"""GPU checks of the pose-free loop's end of sequence: bf_recon_end_sequence / bf_recon_end_solve with a bundler attached.

Fixture: tests/test_recon_bundler_gpu.py's (sift_ref's `medium` scene, 320 x 240, submapSize 3, at most 4 key frames, 1 cm
voxels, recordOps = 1). Streams: `eight` = pose(0..7) ends in a partial submap of 2 images (overlap frame 6 + frame 7), the
smallest that closes; `nine` = pose(0..8) in one of 3 images; `seven` = pose(0..6) ends on a boundary frame, so only the end
solves run. Every loop runs once (module scope) and the tests read it."""
import numpy as np
import pytest

import bundlefusion_amd as bfa
import bundler_ref as B
from bundlefusion_amd.recon import FIX_DEINTEGRATE, FIX_INTEGRATE, Recon
from test_bundler import options
from test_recon_bundler_gpu import BF_ERR_STATE, S, camera, code_of, local_init, loop_options, run_posefree, same, small_loop, upload

pytestmark = pytest.mark.gpu


def run_to_the_end(dev, end_kw, **kw):
    """The pose-free caller's whole call sequence: per frame set_frame, set_frame_bundling, process_frame; then
    end_sequence. Read back as run_posefree does, plus the result of end_sequence, the partial submap (the bundler's last
    closed one) and what a process_frame after the end returned."""
    F = len(dev)
    params = bfa.hash_params(voxel_size=0.01, num_buckets=1 << 16, num_blocks=1 << 15)
    bo = options("medium", S)
    b = bfa.Bundler(bo)
    rc = Recon(params, camera(), loop_options(bo, F + 1, **kw))
    rc.attach_bundler(b)
    first, subs = [], []
    for f, (dc, dd) in enumerate(dev):
        rc.set_frame(f, dd.ptr.value, dc.ptr.value)
        rc.set_frame_bundling(f, dc, dd)
        rc.process_frame(f)
        first.append(rc.trajectory(f + 1)[f].copy())
        if f > 0 and f % S == 0:
            subs.append(b.submap())
    before = rc.optimized_trajectory()
    end = rc.end_sequence(**end_kw)
    partial = (F - 1) % S != 0
    if partial:
        subs.append(b.submap())
    nsub = len(subs)
    run = dict(rc=rc, b=b, bo=bo, params=params, F=F, dev=dev, first=first, subs=subs, end=end, opt_before=before,
               recs=[rc.bundler_frame(f) for f in range(F)], glob=b.global_list(), trace=rc.queue_trace(), ops=rc.op_log(),
               stats=rc.stats(), bst=rc.bundling_stats(), poses=[rc.submap_poses(s, bo.maxKeyframes, S) for s in range(nsub)],
               traj=rc.trajectory(F), opt=rc.optimized_trajectory(), blocks=rc.export_blocks(), bstats=b.stats())
    # one more frame after the end: the bundler's sequence is over
    dc, dd = dev[0]
    rc.set_frame(F, dd.ptr.value, dc.ptr.value)
    rc.set_frame_bundling(F, dc, dd)
    with pytest.raises(bfa.BFError) as e:
        rc.process_frame(F)
    run["after_end"] = (e.value.code, str(e.value))
    return run


def replay_to_the_end(run):
    """A stand-alone bundler driven by hand from the loop's outputs, as test_recon_bundler_gpu.replay, carried on through
    the end: end_sequence, fuse_submap with the partial submap's solved poses, the last update of the trajectory."""
    b = bfa.Bundler(run["bo"])
    updates = [T for kind, _, T in run["trace"] if kind == 1]
    recs, subs = [], []

    def take():
        s = len(subs)
        subs.append(b.submap())
        local, _, valid, ok = run["poses"][s]
        assert ok and valid[s]
        b.fuse_submap(local)
        b.set_complete_trajectory(updates[s], S * s)
    for dc, dd in run["dev"]:
        recs.append(b.process_frame(dc, dd))
        if recs[-1]["submapClosed"]:
            take()
    end = b.end_sequence()
    if end["closed"]:
        take()
    out = dict(recs=recs, subs=subs, end=end, glob=b.global_list(), stats=b.stats())
    b.close()
    return out


def close(run):
    run["rc"].close()
    run["b"].close()


@pytest.fixture(scope="module")
def frames():
    views = B.views("medium", 10)
    return dict(host=views, dev=upload(views))


@pytest.fixture(scope="module")
def eight(frames):
    return run_to_the_end(frames["dev"][:8], dict(num_solve_frames_before_exit=1, dense_at_end=False))


@pytest.fixture(scope="module")
def nine(frames):
    run = run_to_the_end(frames["dev"][:9], dict(num_solve_frames_before_exit=1))
    run["again"] = run_to_the_end(frames["dev"][:9], dict(num_solve_frames_before_exit=1))
    return run


@pytest.fixture(scope="module")
def nine_sparse(frames):
    return run_to_the_end(frames["dev"][:9], dict(num_solve_frames_before_exit=1, dense_at_end=False))


def check_counts(run, F):
    end, st, bst = run["end"], run["stats"], run["bst"]
    assert end["localSolved"] == 1 and end["queueDrained"] == 1 and end["pastEndFrames"] >= 2
    assert st["localSolves"] == 3 and st["invalidLocals"] == 0
    assert run["bstats"]["keyframes"] == 3 and bst["submapsFused"] == 3 and bst["keyframesLost"] == 0
    assert bst["frames"] == F == run["bstats"]["frames"] and bst["bundlerMs"] > 0
    assert bst["framesNotIntegrated"] == bst["submapsInvalidEarly"] == bst["submapsInvalidVerified"] == 0
    assert len(run["opt_before"]) == 6  # the partial submap's frames were not covered before the end
    assert run["opt"].shape == (F, 4, 4) and np.all(np.isfinite(run["opt"]))
    sub = run["subs"][2]
    assert sub["submap"] == 2 and sub["frames"] == F - 6 and sub["is_valid"] and sub["released"]
    local, glob, valid, ok = run["poses"][2]
    assert ok and valid.tolist() == [1, 1, 1] and local.shape == (F - 6, 4, 4) and np.all(np.isfinite(local))
    assert len(run["glob"]["prefix"]) == 3 and run["glob"]["prefix"][-1] == len(run["glob"]["corr"])
    assert run["glob"]["prefix"][2] > run["glob"]["prefix"][1] > 0  # key frame 2 matched an earlier one


def test_eight_ends_in_a_partial_submap_of_two(eight):
    check_counts(eight, 8)
    end, st = eight["end"], eight["stats"]
    assert end["denseSolve"] == 0 and end["last"]["error"] == 0
    # p = 0 the partial submap's global solve over three key frames, p = 1 an end solve
    assert end["globalSolves"] == 2 and st["endSolves"] == 1 and st["globalSolves"] == 2 + 1


def test_nine_ends_in_a_partial_submap_of_three_and_a_dense_solve(nine):
    check_counts(nine, 9)
    end = nine["end"]
    assert end["denseSolve"] == 1 and end["denseSolveMs"] > 0 and end["last"]["error"] == 0 and not end["last"]["skipped"]
    assert end["last"]["numDensePairs"] > 0  # the dense term read the bundler's global cache frames
    assert nine["stats"]["endSolves"] == 1


def test_the_dense_term_reads_the_bundlers_global_cache(frames, nine, nine_sparse):
    """The same stream with and without the dense term at p = 1 is equal up to the partial submap's solves. The fixture
    lies at 1.8 .. 2.35 m, where the reference's depth weight (1 - z / 2)^2.5 is at most 0.004, so at the reference's
    weight 15 the dense solve leaves the sparse solve's poses (printed). That the term is fed from the bundler's global
    cache shows at weight 1000: all three key frame pairs overlap, and the poses of key frames 1 and 2 move."""
    same(nine["poses"][2][0], nine_sparse["poses"][2][0], "the partial submap's local poses")
    same(nine["poses"][2][1], nine_sparse["poses"][2][1], "the key frame poses after the partial submap's global solve")
    assert nine["end"]["last"]["numDensePairs"] == 3
    d = np.abs(nine["opt"].astype(np.float64) - nine_sparse["opt"].astype(np.float64)).max()
    print(f"dense weight 15 against the sparse end solve: largest element difference of the optimised poses {d:.3g}")
    heavy = run_to_the_end(frames["dev"][:9], dict(num_solve_frames_before_exit=1, dense_depth_weight=1000.0))
    end = heavy["end"]
    assert end["denseSolve"] == 1 and end["last"]["numDensePairs"] == 3 and end["last"]["error"] == 0 and end["queueDrained"] == 1
    same(heavy["opt"][:3], nine_sparse["opt"][:3], "submap 0's frames hang on the fixed key frame 0")
    d = np.abs(heavy["opt"][3:].astype(np.float64) - nine_sparse["opt"][3:].astype(np.float64)).max(axis=(1, 2))
    print("dense weight 1000 against the sparse end solve: largest element difference per frame 3..8", [f"{x:.3g}" for x in d])
    assert np.all(np.isfinite(heavy["opt"])) and np.all(d > 1e-5)  # far above float32 rounding of a pose at 2 m
    close(heavy)


def test_seven_ends_on_a_boundary(frames):
    run = run_to_the_end(frames["dev"][:7], dict(num_solve_frames_before_exit=0))
    end, st = run["end"], run["stats"]
    assert end["localSolved"] == 0 and end["globalSolves"] == 1 and end["last"]["error"] == 0
    assert st["endSolves"] == 1 and st["localSolves"] == 2 and run["bstats"]["keyframes"] == 2 and run["bst"]["submapsFused"] == 2
    assert len(run["glob"]["prefix"]) == 2 and len(run["subs"]) == 2
    assert len(run["opt"]) == 6 and np.all(np.isfinite(run["opt"]))
    assert run["after_end"][0] == BF_ERR_STATE and "sequence is over" in run["after_end"][1]
    close(run)


def test_the_loop_drove_the_bundler_as_a_hand_would(frames):
    run = run_to_the_end(frames["dev"][:8], dict(num_solve_frames_before_exit=0))
    assert run["stats"]["removedPairs"] == 0  # else the loop's solves changed the global list in place
    assert run["stats"]["endSolves"] == 0 and run["end"]["localSolved"] == 1
    hand = replay_to_the_end(run)
    assert hand["end"] == dict(closed=1, submap=2, numFrames=2, numCorr=len(hand["subs"][2]["corr"]), isValid=1)
    for f in range(8):
        for k, v in run["recs"][f].items():
            same(np.asarray(v), np.asarray(hand["recs"][f][k]), f"frame {f} record field {k}")
    assert len(run["subs"]) == len(hand["subs"]) == 3
    for s in range(3):
        a, h = run["subs"][s], hand["subs"][s]
        assert a["submap"] == h["submap"] == s and a["frames"] == h["frames"] == (S + 1 if s < 2 else 2)
        assert len(a["corr"]) > 0
        same(a["corr"], h["corr"], f"submap {s} EntryJ")
        same(a["key_idx"], h["key_idx"], f"submap {s} key indices")
        same(a["valid"], h["valid"], f"submap {s} valid flags")
        same(a["device_valid"], h["device_valid"], f"submap {s} device valid flags")
    same(run["glob"]["corr"], hand["glob"]["corr"], "global EntryJ")
    same(run["glob"]["key_idx"], hand["glob"]["key_idx"], "global key indices")
    same(run["glob"]["prefix"], hand["glob"]["prefix"], "prefix[]")
    assert len(run["glob"]["prefix"]) == 3 and run["glob"]["prefix"][-1] == len(run["glob"]["corr"]) > 0
    assert run["bstats"]["keyframes"] == hand["stats"]["keyframes"] == 3
    close(run)


@pytest.mark.parametrize("F", [8, 9])
def test_the_partial_local_solve_is_the_stand_alone_solvers(frames, F):
    """useLocalDense = 0, disableLocalVerify = 1: the partial submap's local poses against bf_solver_solve of the replay
    bundler's list with the same initial poses, iteration counts and weights, at 2 and at 3 images."""
    from bundlefusion_amd.solver import SolverBundling
    n = F - 6
    run = run_to_the_end(frames["dev"][:F], dict(num_solve_frames_before_exit=0, dense_at_end=False), useLocalDense=0,
                         disableLocalVerify=1)
    hand = replay_to_the_end(run)
    sub = hand["subs"][2]
    assert sub["frames"] == n
    solver = SolverBundling(S + 1, 25 * (S + 1) * S // 2)
    init = local_init(hand["recs"], 2, sub["valid"])
    d_T = bfa.DeviceArray.from_host(init)
    rot, trans = bfa.DeviceArray.from_host(np.zeros((n, 3), np.float32)), bfa.DeviceArray.from_host(np.zeros((n, 3), np.float32))
    valid = bfa.DeviceArray.from_host(sub["valid"].astype(np.int32))
    corr = bfa.DeviceArray.from_host(sub["corr"])
    solver.matrices_to_poses(d_T, n, rot, trans, valid)
    solver.solve(corr, len(sub["corr"]), valid, n, 2, 100, [1.0, 1.0], rot=rot, trans=trans, find_max_residual=False)
    assert solver.result()["error"] == 0
    solver.poses_to_matrices(rot, trans, n, d_T, valid)
    solver.synchronize()
    local = run["poses"][2][0]
    same(local, d_T.download().reshape(n, 4, 4), "the partial submap's local poses")
    assert local[1:].tobytes() != init[1:].tobytes()  # the solve moved them
    solver.close()
    assert run["stats"]["localVerifications"] == 0 and run["stats"]["localSolves"] == 3
    close(run)


def test_frames_went_where_the_solves_put_them(eight):
    traj, opt = eight["traj"], eight["opt"]
    assert eight["end"]["queueDrained"] == 1
    for f in (6, 7):
        same(traj[f], opt[f], f"frame {f}: integrated at its optimised pose")
        assert traj[f].tobytes() != eight["first"][f].tobytes(), f"frame {f} is still where it was first integrated"
    ops = [(k, f) for k, f, *_ in eight["ops"]]
    assert (FIX_DEINTEGRATE, 7) in ops and ops.index((FIX_DEINTEGRATE, 7)) > ops.index((FIX_INTEGRATE, 7))
    assert [k for k, f in ops if f == 7 and k in (FIX_DEINTEGRATE, FIX_INTEGRATE)][-1] == FIX_INTEGRATE
    last = [newT for k, f, _, newT in eight["ops"] if k == FIX_INTEGRATE and f == 7][-1]
    same(last.reshape(4, 4), opt[7], "frame 7's last integration is at its optimised pose")
    assert eight["after_end"][0] == BF_ERR_STATE and "sequence is over" in eight["after_end"][1]


def test_two_runs_are_bit_identical(nine):
    a, b = nine, nine["again"]
    same(a["traj"], b["traj"], "trajectory")
    same(a["opt"], b["opt"], "optimised trajectory")
    for f in range(9):
        same(a["first"][f], b["first"][f], f"frame {f}")
    assert len(a["ops"]) == len(b["ops"])
    for x, y in zip(a["ops"], b["ops"]):
        assert x[0] == y[0] and x[1] == y[1]
        same(x[2], y[2])
        same(x[3], y[3])
    for s in range(3):
        same(a["subs"][s]["corr"], b["subs"][s]["corr"], f"submap {s} EntryJ")
        same(a["subs"][s]["key_idx"], b["subs"][s]["key_idx"], f"submap {s} key indices")
        for u, v in zip(a["poses"][s][:3], b["poses"][s][:3]):
            same(u, v, f"submap {s} poses")
    for k in ("corr", "key_idx", "prefix"):
        same(a["glob"][k], b["glob"][k], f"global {k}")
    assert {k: v for k, v in a["end"].items() if k != "denseSolveMs"} == {k: v for k, v in b["end"].items() if k != "denseSolveMs"}
    ba, bb = a["blocks"], b["blocks"]  # the heap slots follow the GC's atomic push order: compare the block set
    key = lambda x: sorted(map(tuple, x[x[:, 3] != 0][:, :3].tolist()))
    assert key(ba) == key(bb) and len(key(ba)) > 100


@pytest.mark.parametrize("dense", [False, True])
def test_accuracy_against_the_restatement_chain(nine, nine_sparse, dense):
    """Each optimised pose relative to frame 0 against sift_ref.pose, frames 6..8 of the partial submap included; at most
    twice the accumulated error of the float64-checked restatement chain (bundler_ref.chain_reference) at the same frame,
    the bar of test_recon_bundler_gpu.test_accuracy_against_the_restatement_chain, without and with the dense end solve.
    Measured on the MI355X: see DESIGN §3.7."""
    run = nine if dense else nine_sparse
    assert run["end"]["denseSolve"] == int(dense)
    ref = B.chain_reference("medium", 9, S)
    opt = run["opt"]
    assert len(opt) == 9
    base = np.linalg.inv(opt[0].astype(np.float64))
    worst = []
    for f in range(1, 9):
        te, re = B.pose_error(base @ opt[f].astype(np.float64), 0, f)
        rte, rre = B.pose_error(ref["sift"][f].astype(np.float64), 0, f)
        print(f"dense {int(dense)} frame {f}: translation error {te:.5f} m (restatement chain {rte:.5f}), rotation error "
              f"{re:.6f} rad (restatement chain {rre:.6f})")
        worst.append((f, te, 2 * rte, re, 2 * rre))
    for f, te, tb, re, rb in worst:
        assert te <= tb and re <= rb, (f, te, tb, re, rb)


def test_state(frames):
    # before the first frame the phase is refused on an attached loop
    bo = options("medium", S)
    b = bfa.Bundler(bo)
    rc = small_loop(bo)
    rc.attach_bundler(b)
    assert code_of(rc.end_sequence) == BF_ERR_STATE and code_of(rc.end_solve) == BF_ERR_STATE
    rc.close()
    b.close()
    # finish() alone leaves the trailing partial submap at its integration poses
    run = run_posefree(frames["dev"][:8], frames["host"][:8], drain=0)
    assert len(run["opt"]) == 6 and run["stats"]["localSolves"] == 2 and run["bstats"]["keyframes"] == 2
    same(run["traj"][7], run["first"][7], "frame 7 after finish()")
    # ... and end_sequence after it still closes and solves it
    end = run["rc"].end_sequence(num_solve_frames_before_exit=0, dense_at_end=False)
    assert end["localSolved"] == 1 and len(run["rc"].optimized_trajectory()) == 8 and run["b"].stats()["keyframes"] == 3
    close(run)
