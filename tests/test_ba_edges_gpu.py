"""The HIP bundle adjuster at its table, row-length and route edges, against the CPU oracle (oracle/ba.cpp).

The inputs come from ba_edge_inputs.py; test_ba_edges.py proves with the oracle alone that each of them reaches
the edge it is named for. Tolerances are the project's own: one GN step with a few PCG iterations tracks the
oracle to 3e-6 rad / m up to 70 images (test_single_gn_step_parity_tight) and to 2e-5 above
(test_many_images_multipass_finisher); longer schedules are held to SURVEY.md's 1e-3 rad / 1 mm. Integer
outcomes (the invalid mask, per-pair counts, iteration counts) are exact, and wherever two routes or two handle
states must compute the same arithmetic the results are compared bit for bit.

Every comparison prints its measured difference before it asserts (pytest -s); profiles/ba_edges_parity.txt
keeps the figures measured on MI355X."""
import ctypes as C
import functools

import numpy as np
import pytest

import ba_edge_inputs as E
import bundlefusion_amd as bfa
from ba_problem import make_problem, pose_diff
from test_ba_gpu import INVALID, MODES, _initial_T, assert_parity, gpu_solve, oracle_solve

pytestmark = pytest.mark.gpu

ASSEMBLED = bfa.abi.NORMAL_EQ_ASSEMBLED
MATRIX_FREE = bfa.abi.NORMAL_EQ_MATRIX_FREE
SURVEY = dict(rot_tol=1e-3, trans_tol=1e-3, energy_rtol=1e-2)


def bar(n_images):
    tol = 3e-6 if n_images <= 70 else 2e-5
    return dict(rot_tol=tol, trans_tol=tol, energy_rtol=1e-4)


def parity(name, g, o, **tol):
    """assert_parity, after printing the measured pose difference; nothing may be non-finite."""
    er, et = pose_diff(g[0], g[1], o[0], o[1])
    print(f"PARITY {name}: rot {er:.2e} rad, trans {et:.2e} m (bar {tol['rot_tol']:.0e}); "
          f"gn {g[3]['gnIterations']}/{o[3]['gnIterations']} pcg {g[3]['pcgIterations']}/{o[3]['pcgIterations']}")
    assert np.isfinite(g[0]).all() and np.isfinite(g[1]).all(), name
    assert np.isfinite(g[3]["maxResidual"]) and np.isfinite(g[3]["energy"]), (name, g[3])
    assert_parity(g[:4], o, **tol)
    assert g[3]["gnIterations"] == o[3]["gnIterations"], (name, g[3], o[3])
    assert g[3]["pcgIterations"] == o[3]["pcgIterations"], (name, g[3], o[3])


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(a[0], b[0], err_msg=what)
    np.testing.assert_array_equal(a[1], b[1], err_msg=what)
    assert a[2].tobytes() == b[2].tobytes(), what
    assert a[3] == b[3], (what, a[3], b[3])


def mode_name(mode):
    return "assembled" if mode == ASSEMBLED else "matrix-free"


def solve_counting_persistent(p, n_nonlin, n_lin, **opts):
    """(gpu_solve's result, k_pcg_persist launches) of an assembled pcgLaunch = 0 solve on a handle of its own, with
    the clock of the persistent launches on: the dispatcher falls back to one launch per iteration quietly, so a
    test that names the persistent route asks here whether it ran."""
    from bundlefusion_amd.solver import SolverBundling
    S = SolverBundling(p["K"], max(p["K"] * 4000, len(p["corr"])), normal_equations=ASSEMBLED, **opts)
    n = C.c_uint64()
    try:
        bfa.check(bfa.lib().bf_solver_pcg_time(S.h, 1, None, None))
        g = gpu_solve(p, n_nonlin, n_lin, [1.0] * n_nonlin, handle=S)
        bfa.check(bfa.lib().bf_solver_pcg_time(S.h, 0, None, C.byref(n)))
    finally:
        S.close()
    return g, int(n.value)


# ---- A. table build -------------------------------------------------------------------------------------------
def table_case(name, prob, mode, corr=None, max_corr=None, schedule=(1, 4)):
    """1 GN x 4 PCG in the given mode: parity with the oracle, the exact invalid mask (assert_parity), and in the
    assembled mode the exact per-pair counts in (a, b) order."""
    corr = prob["corr"] if corr is None else corr
    n_nonlin, n_lin = schedule
    ws = [1.0] * n_nonlin
    g = gpu_solve(prob, n_nonlin, n_lin, ws, corr=corr, mode=mode, max_corr=max_corr, export=mode == ASSEMBLED)
    o = oracle_solve(prob, n_nonlin, n_lin, ws, corr=corr, max_corr=max_corr)
    parity(f"{name} {mode_name(mode)}", g, o, **bar(prob["K"]))
    if mode == ASSEMBLED:
        stats, ab = g[4]
        counts = E.pair_counts(o[2])
        assert [tuple(int(x) for x in p) for p in ab] == list(counts)
        np.testing.assert_array_equal(stats[:, 15], np.array(list(counts.values()), np.float64))
    return g, o


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", E.PREFIX_COUNTS)
def test_table_correspondence_counts(n, mode):
    """Prefixes of one interleaved list on 6 images, at the 64-lane placement step and the 256 tile +-1."""
    p = E.six_problem()
    table_case(f"A prefix {n}", p, mode, corr=p["corr"][:n].copy())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", E.TILE_COUNTS)
@pytest.mark.parametrize("N", E.TILE_N)
def test_table_tile_size(N, n, mode):
    """tile_for: 256 images build with tiles of 256 correspondences, 257 images with tiles of 512."""
    p = E.tile_problem(N)
    table_case(f"A tile N={N} nCorr={n}", p, mode, corr=p["corr"][:n].copy())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(E.PRE_INVALID))
def test_table_pre_invalidated(name, mode):
    """Correspondences that arrive invalid take no slot and no rank, and stay invalid."""
    p = E.six_problem()
    corr = E.invalidated(p["corr"], E.PRE_INVALID[name])
    g, _ = table_case(f"A pre-invalid {name}", p, mode, corr=corr)
    mask = np.zeros(len(corr), bool)
    mask[E.PRE_INVALID[name]] = True
    np.testing.assert_array_equal(g[2]["i"] == INVALID, mask)
    np.testing.assert_array_equal(g[2]["j"] == INVALID, mask)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["exact", "plus1", "cascade", "cascade_shuffled"])
def test_table_cap(name, mode):
    """Rows of exactly cap and cap + 1 entries, and the cascade: a dropped correspondence keeps its rank in its
    other row."""
    p = E.cap_problem(name)
    g, _ = table_case(f"A cap {name}", p, mode, max_corr=E.cap_max_corr(4))
    inv = np.flatnonzero(g[2]["i"] == INVALID)
    if name == "exact":
        assert len(inv) == 0
    elif name == "plus1":
        assert list(inv) == [E.CAP]
    else:
        np.testing.assert_array_equal(g[2]["i"] == INVALID, E.cap_replay(p["corr"], 4, E.CAP))
        if name == "cascade":
            c = p["corr"]
            drops = tuple(int(((g[2]["i"] == INVALID) & (c["i"] == a) & (c["j"] == b)).sum()) for a, b, _ in E.CASCADE)
            assert drops == E.CASCADE_DROPS


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["reverse", "mixed", "interleaved"])
def test_table_orientation_and_order(name, mode):
    """All i > j; both orientations inside one pair; a pair's correspondences scattered among other pairs'."""
    table_case(f"A orientation {name}", E.orientation_problem(name), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", E.ROWLESS)
def test_table_images_without_a_row(name, mode):
    p, none = E.rowless_problem(name)
    g, _ = table_case(f"A rowless {name}", p, mode)
    for v in none:  # delta = 0, and the Lie update round-trips exp / log (test_no_correspondences)
        np.testing.assert_allclose(g[0][v], p["rot"][v], atol=1e-6)
        np.testing.assert_allclose(g[1][v], p["trans"][v], atol=1e-6)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("invalid", [False, True])
def test_invalid_image_is_left_out_of_the_gn_exit(invalid, mode):
    """a.valid is read by k_gn_end's exit test alone: with the one displaced image invalid, the solve stops a
    GN step earlier, as the oracle's does."""
    p = E.invalid_image_problem(False)
    valid = E.invalid_image_problem(invalid)["valid"]
    assert int(valid.sum()) == (7 if invalid else 8) and p["valid"].all()
    n_nonlin, n_lin = E.INVALID_IMAGE["schedule"]
    g = gpu_solve(p, n_nonlin, n_lin, [1.0] * n_nonlin, mode=mode, valid=valid)
    o = oracle_solve(p, n_nonlin, n_lin, [1.0] * n_nonlin, valid=valid)
    assert o[3]["gnIterations"] == (1 if invalid else 2)
    parity(f"A valid[5]={0 if invalid else 1} {mode_name(mode)}", g, o, **SURVEY)


# ---- B. row, run and degree strides ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stride_case(name):
    p = E.rows_problem() if name == "rows" else E.degree_problem()
    return p, oracle_solve(p, 1, 5, [1.0])


def device_transforms(p):
    """The float32 pose matrices the solve builds its world points from (k_transforms and poses_to_matrices share
    one pose_to_matrix)."""
    from bundlefusion_amd.solver import SolverBundling
    n = p["K"]
    S = SolverBundling(n, 4000)
    dT = bfa.DeviceArray.from_host(np.zeros((n, 4, 4), np.float32))
    S.poses_to_matrices(bfa.DeviceArray.from_host(p["rot"]), bfa.DeviceArray.from_host(p["trans"]), n, dT,
                        bfa.DeviceArray.from_host(np.ones(n, np.int32)))
    T = dT.download()
    S.close()
    return T


@pytest.mark.parametrize("name", ["rows", "degrees"])
def test_stride_pair_statistics(name):
    """k_pair_sort / k_pair_fill / k_pair_gather / k_pair_stats on rows of 1..1025 entries, runs of 1..1025 and up
    to 449 partners, both orientations: fp64 sums against the NumPy restatement, counts exact.

    The restatement sums the float32 world points T p, so it is given the device's own float32 T (held to the
    oracle's within 1e-6 here): the device's sinf / cosf differ from the host's in the last place, and over a run
    of 1 025 correspondences those last places add up to 1.6e-6 in a sum that cancels to 0.08, past atol (measured:
    2 of 5 432 and 2 of 59 248 elements at up to 1.4x the bound with the oracle's T, T itself 2e-7 apart; with the
    device's T the statistics are order-only differences in fp64, 3e-9 of the bound, as
    test_pair_statistics_match_numpy says).

    So that the device's pose_to_matrix cannot drift behind the reference it feeds, the oracle's T holds a
    ceiling of its own: the bound twice over (one share for the order of the sums, one for T's last places) on
    every element, and the bound itself on all but 0.1 % of them."""
    from oracle_pairs import pair_stats
    p, _ = stride_case(name)
    g = gpu_solve(p, 1, 5, [1.0], mode=ASSEMBLED, export=True)
    stats, ab = g[4]
    T_dev, T_host = device_transforms(p), _initial_T(p)
    print(f"STATS {name}: device T against the oracle's: max {np.abs(T_dev - T_host).max():.2e}")
    np.testing.assert_allclose(T_dev, T_host, rtol=0, atol=1e-6)
    keys = [tuple(int(x) for x in k) for k in ab]
    excess = {}
    for label, T in (("oracle T", T_host), ("device T", T_dev)):
        ref = pair_stats(E.survivors(g[2]), T)
        assert keys == sorted(ref.keys()) and len(keys) == len(E.pair_counts(p["corr"]))
        R = np.stack([ref[k] for k in keys])
        excess[label] = np.abs(stats - R) / (1e-6 + 2e-6 * np.abs(R))
        print(f"STATS {name} ({label}): max |gpu - ref| / (atol + rtol |ref|) = {excess[label].max():.2e}, "
              f"{int((excess[label] > 1).sum())} of {excess[label].size} above 1")
        np.testing.assert_array_equal(stats[:, 15], R[:, 15])
    assert excess["oracle T"].max() <= 2.0 and (excess["oracle T"] > 1).mean() < 1e-3
    np.testing.assert_allclose(stats, R, rtol=2e-6, atol=1e-6)  # R: the device's T


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["rows", "degrees"])
def test_stride_parity(name, mode):
    p, o = stride_case(name)
    g = gpu_solve(p, 1, 5, [1.0], mode=mode)
    parity(f"B {name} {mode_name(mode)}", g, o, **bar(p["K"]))


@pytest.mark.parametrize("name", ["rows", "degrees"])
def test_stride_persistent_equals_per_iteration(name):
    """k_pcg_persist (partners in registers, as pair refs, and in the tail loop) against k_pcg_pairs (pair_row_ap's
    rounds of 128): the same arithmetic in the same order."""
    p, _ = stride_case(name)
    for sched in ((1, 5), (2, 30)):
        a, launches = solve_counting_persistent(p, *sched)
        b = gpu_solve(p, sched[0], sched[1], [1.0] * sched[0], pcg_launch=1)
        print(f"LAUNCHES B {name} {sched}: {launches} persistent for {a[3]['gnIterations']} GN steps")
        assert launches == a[3]["gnIterations"] == sched[0]  # one persistent launch per GN step
        assert a[3]["error"] == 0 and b[3]["error"] == 0
        same_bits(a, b, f"{name} {sched}")


# ---- C. route boundaries --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def route_case(N, n_nonlin, n_lin):
    p = E.route_problem(N)
    return p, oracle_solve(p, n_nonlin, n_lin, [1.0] * n_nonlin)


@pytest.mark.parametrize("N", E.ROUTE_N)
def test_route_one_step(N):
    """64 | 65: k_pcg_small against the grid routes; 513 | 514: one finisher against four (k_pcg_pairs<2> against
    <8>); 2017 | 2018: the wide persistent launch, its grid exactly the 512 co-resident workgroups of 256 CUs x 2,
    against one launch per iteration; 2049 | 2050: pcg_finisher<8> with its rows in registers against its
    multi-pass form, both under one launch per iteration."""
    p, o = route_case(N, 1, 5)
    g = gpu_solve(p, 1, 5, [1.0], mode=ASSEMBLED)
    assert g[3]["pcgIterations"] == 5
    parity(f"C route N={N} 1x5 assembled", g, o, **bar(N))


@pytest.mark.parametrize("N", E.ROUTE_N)
def test_route_schedule(N):
    """2 x 30 against the oracle, and pcgLaunch 0 against 1 bit for bit from 65 to 2 049 images. The persistent
    route itself ends at WIDE_PERSIST_N = 2 017 (ba_edge_inputs.persist_grid; it assumes MI355X's 256 CUs x 2
    workgroups): up to there the comparison is k_pcg_persist against k_pcg_pairs, and the launch count says that
    k_pcg_persist ran. From 2 018 to 2 049 both settings take one launch per iteration, so there the comparison
    holds only the dispatcher's fall-back, and the count says that too."""
    p, o = route_case(N, 2, 30)
    g, launches = solve_counting_persistent(p, 2, 30)
    print(f"LAUNCHES C route N={N}: {launches} persistent for {g[3]['gnIterations']} GN steps")
    parity(f"C route N={N} 2x30 assembled", g, o, **SURVEY)
    if E.SMALL_N < N <= E.WIDE_PERSIST_N:
        assert launches == g[3]["gnIterations"], "the persistent route ends below ba_edge_inputs.WIDE_PERSIST_N"
    else:
        assert launches == 0, "the persistent route reaches past ba_edge_inputs.WIDE_PERSIST_N"
    if E.SMALL_N < N <= E.FINISHER8_N:
        b = gpu_solve(p, 2, 30, [1.0, 1.0], mode=ASSEMBLED, pcg_launch=1)
        assert b[3]["error"] == 0
        same_bits(g, b, f"N={N}")


@pytest.mark.parametrize("N", [513, 514])
def test_route_matrix_free(N):
    """k_pcg's finisher: 2 rows per thread in registers at 513 images, multi-pass at 514."""
    for n_nonlin, n_lin, tol in ((1, 5, bar(N)), (2, 30, SURVEY)):
        p, o = route_case(N, n_nonlin, n_lin)
        g = gpu_solve(p, n_nonlin, n_lin, [1.0] * n_nonlin, mode=MATRIX_FREE)
        parity(f"C route N={N} {n_nonlin}x{n_lin} matrix-free", g, o, **tol)


@pytest.mark.parametrize("n_lin", [E.NLIN_PERSIST, E.NLIN_PERSIST + 1])
def test_route_nlin_tag_limit(n_lin):
    """A persistent tag is epoch * 256 + iteration + 1: 254 iterations still run in one launch, 255 fall back to
    one launch per iteration. Fixed schedule, so every iteration runs on both. At 255 both settings run the same
    kernels, so there the bit comparison cannot fail: the iteration count and the launch count carry that case."""
    p = E.route_problem(65)
    a, launches = solve_counting_persistent(p, 2, n_lin, early_out=False)
    b = gpu_solve(p, 2, n_lin, [1.0, 1.0], mode=ASSEMBLED, early_out=False, pcg_launch=1)
    print(f"LAUNCHES C n_lin={n_lin}: {launches} persistent")
    assert launches == (2 if n_lin <= E.NLIN_PERSIST else 0)
    assert a[3]["error"] == 0 and b[3]["error"] == 0
    assert a[3]["gnIterations"] == 2 and a[3]["pcgIterations"] == 2 * n_lin
    same_bits(a, b, f"n_lin={n_lin}")


def test_route_dense_above_513_images():
    """The dense term at 514 images: one launch per iteration, k_pcg_pairs<8> with pcg_dense_offdiag."""
    p = E.dense_problem()
    assert p["K"] == E.DENSE_N
    for n_nonlin, n_lin, tol in ((1, 4, bar(E.DENSE_N)), (2, 40, SURVEY)):
        args = (n_nonlin, n_lin, [1.0] * n_nonlin, [1000.0] * n_nonlin, [0.0] * n_nonlin)
        g = gpu_solve(p, *args, use_cache=True, mode=ASSEMBLED)
        o = oracle_solve(p, *args, use_cache=True)
        assert g[3]["numDensePairs"] > 0
        parity(f"C dense N={E.DENSE_N} {n_nonlin}x{n_lin} assembled", g, o, **tol)


# ---- D. handle state ------------------------------------------------------------------------------------------
def test_handle_reused_across_problems():
    """One handle sized for 600 images, as the reconstruction loop keeps one for the whole run: solves of 70, 6,
    520, 70, 70 (tables kept), 6 (dense) and 6 images, each bit-identical to the same solve on a fresh handle of
    exactly its size (same cap: 4000)."""
    from bundlefusion_amd.solver import SolverBundling
    dense = make_problem(K=6, stride=2, max_per_pair=10, outliers=0.0, with_cache=True, drift=(0.2, 0.005))
    sparse = (2, 20, [1.0, 1.0])
    steps = [("70", E.route_problem(70), sparse, {}),
             ("6", E.six_problem(), sparse, {}),
             ("520", E.route_problem(520), sparse, {}),
             ("70 other", E.problem(70, E.band(70, 3, 3), seed=19), sparse, {}),
             ("70 other, tables kept", E.problem(70, E.band(70, 3, 3), seed=19), sparse, dict(rebuild_jt=False)),
             ("6 dense", dense, (2, 40, [1.0, 1.0], [1000.0, 1000.0], [0.0, 0.0]), dict(use_cache=True)),
             ("6", E.six_problem(), sparse, {})]
    max_images = 600
    S = SolverBundling(max_images, max_images * 4000)
    assert S.max_corr // max_images == 4000
    prev = None
    try:
        for name, prob, args, kw in steps:
            got = gpu_solve(prob, *args, handle=S, **kw)
            fresh_kw = {k: v for k, v in kw.items() if k != "rebuild_jt"}
            want = gpu_solve(prob, *args, **fresh_kw)
            assert want[3]["error"] == 0 and want[3]["pcgIterations"] > 0
            same_bits(got, want, f"step {name}")
            if kw.get("rebuild_jt") is False:
                same_bits(got, prev, f"step {name} against the solve before it")
            if kw.get("use_cache"):
                assert got[3]["numDensePairs"] > 0
            prev = got
    finally:
        S.close()


@pytest.mark.parametrize("N", [70, 520])
def test_handle_larger_than_the_problem(N):
    """max_images = 2 N against max_images = N: the strides by maxN (vector fields, Ap granules, pose backup,
    per-image pair lists) are not the strides by N."""
    p = E.route_problem(N)
    a = gpu_solve(p, 2, 20, [1.0, 1.0], max_images=2 * N)
    b = gpu_solve(p, 2, 20, [1.0, 1.0])
    assert a[3]["error"] == 0 and a[3]["pcgIterations"] > 0
    same_bits(a, b, f"N={N}")
