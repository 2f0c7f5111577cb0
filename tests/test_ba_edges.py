"""The inputs of test_ba_edges_gpu.py (ba_edge_inputs.py) reach the edges they are named for: checked here with
the CPU oracle (oracle/ba.cpp) and NumPy alone (but for the dense case's cache frames, which come from the
synthetic room).

A parity test proves nothing about a branch its input never takes: a graph whose longest row has 40 entries
cannot tell a broken chunk boundary from a working one, and a list with every row under the cap cannot tell
`>= cap` from `> cap`. Every assertion below is a condition on an input, not a tolerance on a kernel; a change
to the generator that empties one of the GPU tests fails here first. Every oracle result must be finite: a
case whose oracle result is not would be no valid input."""
import functools

import numpy as np
import pytest

import ba_edge_inputs as E
from oracle_ba import dense_system, max_corr_per_image, solve


def oracle(prob, n_nonlin=1, n_lin=4, max_corr=None, corr=None, valid=None, early_out=True):
    K = prob["K"]
    corr = prob["corr"] if corr is None else corr
    max_corr = max_corr or max(K * 4000, len(corr))
    return solve(corr, prob["valid"] if valid is None else valid, prob["rot"], prob["trans"], n_nonlin, n_lin,
                 [1.0] * n_nonlin, max_corr_per_img=max_corr_per_image(K, max_corr), early_out=early_out)


def finite(o):
    rot, trans, _, res = o
    return bool(np.isfinite(rot).all() and np.isfinite(trans).all() and np.isfinite(res["maxResidual"]) and
                np.isfinite(res["finalEnergy"]))


def test_generator_is_seeded_and_exact():
    """Same arrays on every call; the correspondences of a pair agree under the ground-truth poses to the noise."""
    a, b = E.route_problem(65), E.route_problem(65)
    assert a["corr"].tobytes() == b["corr"].tobytes() and a["rot"].tobytes() == b["rot"].tobytes()
    assert (a["rot"][0] == a["gt_rot"][0]).all() and (a["trans"][0] == a["gt_trans"][0]).all()
    assert np.abs(a["rot"][1:] - a["gt_rot"][1:]).max() > 1e-3
    T = E.pose_matrices(a["gt_rot"], a["gt_trans"])
    c = a["corr"]
    Pi = np.einsum("nij,nj->ni", T[c["i"], :3, :3], c["pos_i"]) + T[c["i"], :3, 3]
    Pj = np.einsum("nij,nj->ni", T[c["j"], :3, :3], c["pos_j"]) + T[c["j"], :3, 3]
    d = np.abs(Pi - Pj)
    assert 1e-4 < d.mean() < 3e-3 and d.max() < 0.01
    # the float64 exponential is the oracle's poseToMatrix
    from oracle_ba import pose_to_matrix
    for k in (0, 1, 64):
        np.testing.assert_allclose(T[k], pose_to_matrix(a["gt_rot"][k], a["gt_trans"][k]), atol=2e-6)


def test_prefix_counts_sit_on_the_step_and_tile():
    p = E.six_problem()
    assert len(p["corr"]) == 513 == E.PREFIX_COUNTS[-1]
    for n in (E.WAVE, E.TILE, 2 * E.TILE):
        assert {n - 1, n + 1} <= set(E.PREFIX_COUNTS)
    assert {E.WAVE, E.TILE, 1} <= set(E.PREFIX_COUNTS)
    # interleaved: the first 9 correspondences are 9 distinct pairs, so a 64-wide step holds many rows
    head = p["corr"][:9]
    assert len({(int(e["i"]), int(e["j"])) for e in head}) == 9
    for n in E.PREFIX_COUNTS:
        assert finite(oracle(p, corr=p["corr"][:n])), n


@pytest.mark.parametrize("N", E.TILE_N)
def test_tile_cases_change_the_tile_count(N):
    p = E.tile_problem(N)
    tile = E.TILE * (-(-N // E.TILE_IMAGES) if N > E.TILE_IMAGES else 1)
    assert tile == (256 if N == 256 else 512)
    assert len(p["corr"]) >= max(E.TILE_COUNTS)
    tiles = [-(-n // tile) for n in E.TILE_COUNTS]
    assert tiles == ([2, 2, 3] if N == 256 else [1, 1, 2])
    for n in E.TILE_COUNTS:
        assert (E.row_lengths(p["corr"][:n], N) > 0).all()  # every image keeps a row
        assert finite(oracle(p, corr=p["corr"][:n])), n


@pytest.mark.parametrize("name", list(E.PRE_INVALID))
def test_pre_invalidated_entries(name):
    p = E.six_problem()
    idx = E.PRE_INVALID[name]
    corr = E.invalidated(p["corr"], idx)
    o = oracle(p, corr=corr)
    assert finite(o)
    mask = np.zeros(len(corr), bool)
    mask[idx] = True
    np.testing.assert_array_equal(o[2]["i"] == E.INVALID, mask)  # nothing else goes, nothing comes back
    if name == "one_step":
        assert idx[0] % E.WAVE == 0 and len(idx) == E.WAVE
    if name == "one_tile":
        assert idx[0] % E.TILE == 0 and len(idx) == E.TILE
    if name == "last":
        assert idx[-1] == len(corr) - 1


def test_row_of_exactly_cap_and_cap_plus_one():
    mc = E.cap_max_corr(4)
    assert max_corr_per_image(4, mc) == E.CAP
    p = E.cap_problem("exact")
    assert E.row_lengths(p["corr"], 4).max() == E.CAP
    o = oracle(p, max_corr=mc)
    assert finite(o) and not (o[2]["i"] == E.INVALID).any()
    p = E.cap_problem("plus1")
    assert E.row_lengths(p["corr"], 4).max() == E.CAP + 1
    o = oracle(p, max_corr=mc)
    inv = np.flatnonzero(o[2]["i"] == E.INVALID)
    assert finite(o) and list(inv) == [E.CAP]  # the highest-index entry of row 1: (0,1) x 500 then (1,2) x 501
    assert (p["corr"]["i"][E.CAP], p["corr"]["j"][E.CAP]) == (1, 2)


@pytest.mark.parametrize("name", ["cascade", "cascade_shuffled"])
def test_cap_cascade_counts_dropped_entries_in_their_other_row(name):
    """Row 2 drops 100 of (2, 3) although only 900 of its entries survive: the 200 dropped (1, 2) entries keep
    their ranks in row 2."""
    p = E.cap_problem(name)
    mc = E.cap_max_corr(4)
    o = oracle(p, max_corr=mc)
    assert finite(o)
    inv = o[2]["i"] == E.INVALID
    np.testing.assert_array_equal(inv, E.cap_replay(p["corr"], 4, E.CAP))
    drops = [int(inv[(p["corr"]["i"] == a) & (p["corr"]["j"] == b)].sum()) for a, b, _ in E.CASCADE]
    if name == "cascade":
        assert tuple(drops) == E.CASCADE_DROPS
    else:
        assert sum(drops) > 0 and tuple(drops) != E.CASCADE_DROPS  # the order decides which go
    rows = E.row_lengths(o[2], 4)
    assert (rows < E.CAP).sum() >= 3 and rows[2] < E.CAP  # a dropped correspondence with both rows under the cap
    assert inv[(p["corr"]["i"] == 2) & (p["corr"]["j"] == 3)].any()


@pytest.mark.parametrize("name", ["reverse", "mixed", "interleaved"])
def test_orientation_and_order_cases(name):
    p = E.orientation_problem(name)
    c = p["corr"]
    if name == "reverse":
        assert (c["i"] > c["j"]).all()
    elif name == "mixed":
        for a, b in E.pair_counts(c):
            fwd = ((c["i"] == a) & (c["j"] == b)).sum()
            bwd = ((c["i"] == b) & (c["j"] == a)).sum()
            assert fwd > 5 and bwd > 5, (a, b)
    else:
        key = c["i"].astype(np.int64) * 8 + c["j"]
        assert (key[1:] != key[:-1]).all()  # no two neighbours of one pair
    assert E.pair_counts(c) == E.pair_counts(E.six_pairs_contiguous()["corr"])
    assert finite(oracle(p))


@pytest.mark.parametrize("name", E.ROWLESS)
def test_rowless_images(name):
    p, none = E.rowless_problem(name)
    rows = E.row_lengths(p["corr"], p["K"])
    assert [int(v) for v in np.flatnonzero(rows == 0)] == none
    if name == "two_components":
        assert all((a < 3) == (b < 3) for a, b in E.pair_counts(p["corr"]))
    if name == "single":
        assert len(p["corr"]) == 1
    o = oracle(p)
    assert finite(o)
    for v in none:  # an image without a row does not move (exp / log round trip)
        np.testing.assert_allclose(o[0][v], p["rot"][v], atol=1e-6)
        np.testing.assert_allclose(o[1][v], p["trans"][v], atol=1e-6)


def test_invalid_image_changes_the_gn_exit():
    c = E.INVALID_IMAGE
    n_nonlin, n_lin = c["schedule"]
    a = oracle(E.invalid_image_problem(False), n_nonlin, n_lin)
    b = oracle(E.invalid_image_problem(True), n_nonlin, n_lin)
    assert finite(a) and finite(b)
    assert (a[3]["gnIterations"], b[3]["gnIterations"]) == (2, 1)


@functools.lru_cache(maxsize=None)
def rows_case():
    p = E.rows_problem()
    return p, oracle(p, 1, 5)


@functools.lru_cache(maxsize=None)
def degree_case():
    p = E.degree_problem()
    return p, oracle(p, 1, 5)


def test_row_and_run_lengths():
    p, o = rows_case()
    assert p["K"] == E.ROWS_N > E.SMALL_N
    assert finite(o) and not (o[2]["i"] == E.INVALID).any()
    rows = set(int(x) for x in E.row_lengths(p["corr"], p["K"]))
    assert set(E.ROW_LENGTHS) <= rows, sorted(rows)
    for n in (E.CH, 2 * E.CH):
        assert {n - 1 if n == E.CH else n, n, n + 1} <= set(E.ROW_LENGTHS)
    runs = set(E.pair_counts(p["corr"]).values())
    assert set(E.RUN_LENGTHS) <= runs, sorted(runs)
    for n in (E.WAVE, 2 * E.WAVE):
        assert {n, n + 1} <= set(E.RUN_LENGTHS)
    # both orientations inside the runs
    assert (p["corr"]["i"] > p["corr"]["j"]).sum() > 1000 and (p["corr"]["i"] < p["corr"]["j"]).sum() > 1000


def test_row_degrees():
    p, o = degree_case()
    assert E.SMALL_N < p["K"] == E.DEGREE_N <= E.ONE_FINISHER_N
    assert finite(o) and not (o[2]["i"] == E.INVALID).any()
    deg = E.row_degrees(p["corr"], p["K"])
    assert set(E.DEGREES) <= set(int(d) for d in deg[1:]), sorted(set(deg))  # row 0 (fixed) is not computed
    for n in (E.ROW_PAIR_ROUND, E.PP_REGS, E.PP_REFS):
        assert {n, n + 1} <= set(E.DEGREES)
    assert E.row_lengths(p["corr"], p["K"]).max() < 4000


@pytest.mark.parametrize("N", E.ROUTE_N)
def test_route_problems(N):
    p = E.route_problem(N)
    assert len(p["corr"]) == (3 * N - 6) * 3
    for n in (E.SMALL_N, E.ONE_FINISHER_N, E.WIDE_PERSIST_N, E.FINISHER8_N):
        assert {n, n + 1} <= set(E.ROUTE_N)
    # the last image count whose wide persistent grid is co-resident on 256 CUs x 2 workgroups: exactly full
    assert E.WIDE_PERSIST_N == 2017 and E.persist_grid(2017) == E.PERSIST_CAPACITY == 512 < E.persist_grid(2018)
    assert E.persist_grid(E.FINISHER8_N) == 520
    o = oracle(p, 1, 5)
    assert finite(o) and o[3]["pcgIterations"] == 5
    assert (E.row_lengths(p["corr"], N) > 0).all()


def test_oracle_order_measure_at_2050():
    """The oracle against itself with its correspondence list reversed (a summation-order change only; no cap
    applies): the float32 noise floor of the N = 2 050 band, far under the 2e-5 bar of the GPU test."""
    from ba_problem import pose_diff
    p = E.route_problem(2050)
    a = oracle(p, 1, 5)
    b = oracle(p, 1, 5, corr=p["corr"][::-1].copy())
    er, et = pose_diff(a[0], a[1], b[0], b[1])
    print(f"oracle order measure N=2050: rot {er:.2e} trans {et:.2e}")
    assert er < 5e-6 and et < 5e-6


def test_handle_state_problems_differ():
    a, b = E.route_problem(70), E.problem(70, E.band(70, 3, 3), seed=19)
    assert len(a["corr"]) == len(b["corr"]) and a["corr"].tobytes() != b["corr"].tobytes()
    assert finite(oracle(b, 1, 5))


def test_dense_case_above_513_images_overlaps():
    """The smallest cache size of DENSE_SIZES at which BuildDenseSystem's overlap search finds a pair."""
    found = None
    for size in E.DENSE_SIZES:
        prob = E.dense_problem(size)
        assert prob["K"] == E.DENSE_N == E.ONE_FINISHER_N + 1
        n = dense_system(prob["valid"], prob["rot"], prob["trans"], prob["cache"], prob["intrinsics"])[3]
        print(f"dense {size}: {n} overlapping pairs")
        if n > 0:
            found = size
            break
    assert found == E.DENSE_SIZE, found
