"""The inputs of test_image_edges_gpu.py (image_edge_inputs.py) meet the conditions that make those
comparisons worth running: checked here with the CPU oracle (oracle/frames.cpp) alone.

A bit-exact GPU comparison proves little on an input that never leaves one side of a branch: a frame that is
valid everywhere cannot tell a skipped bounds test from a kept one, and a pair list whose pairs are all full
cannot tell a wrong scan from a right one. Every assertion below is a condition on an input, not a tolerance on
a kernel."""
import functools

import numpy as np
import pytest

from bundlefusion_amd import io as bio
from bundlefusion_amd.cache import cache_options
from bundlefusion_amd.corr import corr_options
from image_edge_inputs import (CACHE_SHAPES, CACHE_TAIL, CORR_H, CORR_OPTION_SETS, CORR_W, CORR_WINDOWS, FX,
                               OFF_GRID_SIZES, boundary_sizes, corr_intrinsics, corr_problem, depth_metres,
                               flat_frame, interior_tiles, pose_inverse, sensor_frame)
from oracle_lib import cache_store_frame, corr_from_depth as or_corr, preprocess


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- generators ----------------------------------------------------------------------------------------
def test_generators_are_deterministic_and_shaped():
    d, c = sensor_frame(67, 19, 3)
    d2, c2 = sensor_frame(67, 19, 3)
    assert d.dtype == np.uint16 and d.shape == (19, 67) and c.dtype == np.uint8 and c.shape == (19, 67, 4)
    assert np.array_equal(d, d2) and np.array_equal(c, c2)
    assert not np.array_equal(d, sensor_frame(67, 19, 4)[0])
    assert np.all(d[19 // 3:19 // 3 + 4, 67 // 2:67 // 2 + 5] == 0)           # the hole
    fd, fc = flat_frame(33, 9)
    assert np.all(fd == 2000) and np.all(fc == fc[0, 0])
    m = depth_metres(d)
    assert np.all(np.isneginf(m[d == 0])) and np.all(m[d > 0] == d[d > 0].astype(np.float32) / np.float32(1000))


@pytest.mark.parametrize("R", range(1, 8))   # R = 0 has no halo: every whole tile is interior
def test_boundary_sizes_have_one_interior_tile_or_none(R):
    a, b, c = boundary_sizes(R)
    assert [interior_tiles(*s, R) for s in (a, b, c)] == [1, 0, 0]
    # and it is the smallest: nothing with fewer columns or rows has one
    assert interior_tiles(a[0] - 1, 4 * a[1], R) == 0 and interior_tiles(4 * a[0], a[1] - 1, R) == 0


# ---- preprocessing -------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(67, 19), (66, 18), (68, 20), (33, 9), (31, 7), (100, 37)])
def test_sensor_frame_exercises_both_sides(W, H):
    u16, col = sensor_frame(W, H)
    raw = depth_metres(u16)
    assert 0.8 < (u16 > 0).mean() < 0.99
    er, _ = preprocess(bio.preprocess_options(structure=3, depth_filter=False), u16, col, (W, H))
    assert 0.6 < np.isfinite(er).mean() < 0.95               # erosion removes some pixels and keeps most
    assert (bits(er) != bits(raw)).mean() > 0.05
    fl, _ = preprocess(bio.preprocess_options(erode=False), u16, col, (W, H))
    assert (bits(fl) != bits(raw)).mean() > 0.8              # the bilateral filter moves nearly every valid pixel
    assert np.array_equal(np.isfinite(fl), np.isfinite(raw))


@pytest.mark.parametrize("R", range(1, 8))
def test_boundary_frames_exercise_every_radius(R):
    """At every radius and boundary size: erosion both removes and keeps pixels, and the filter's range test
    (default sigmaR) both takes and refuses taps, i.e. its output differs from the one with sigmaR = 100."""
    for W, H in boundary_sizes(R):
        u16, col = sensor_frame(W, H, R)
        raw = depth_metres(u16)
        er, _ = preprocess(bio.preprocess_options(structure=R, depth_filter=False), u16, col, (W, H))
        gone = np.isfinite(raw) & ~np.isfinite(er)
        assert gone.mean() > 0.02 and np.isfinite(er).mean() > 0.3, (R, W, H)
        near = preprocess(bio.preprocess_options(erode=False, sigma_d=R / 2), u16, col, (W, H))[0]
        wide = preprocess(bio.preprocess_options(erode=False, sigma_d=R / 2, sigma_r=100.0), u16, col, (W, H))[0]
        assert (bits(near) != bits(raw)).mean() > 0.5 and (bits(near) != bits(wide)).mean() > 0.05, (R, W, H)


@pytest.mark.parametrize("R", range(8))
def test_flat_frame_shows_a_tap_from_outside(R):
    """The reference skips out-of-image taps, so on the flat frame erosion counts nothing at the border and
    the filter averages equal depths: the outputs are the input. A tap read from the staged 0.0f outside the
    image would be counted by the erosion and, with sigmaR = 100, weighted by the filter."""
    for W, H in boundary_sizes(R) + (OFF_GRID_SIZES if R in (3, 7) else []):
        u16, col = flat_frame(W, H)
        for frac in (0.3, 0.004):    # 0.004 < 1 / 15^2: one counted tap would erode the pixel
            er, _ = preprocess(bio.preprocess_options(structure=R, depth_filter=False, erode_fraction=frac), u16, col,
                               (W, H))
            assert np.array_equal(bits(er), bits(depth_metres(u16))), (R, W, H, frac)
        if R == 0:
            continue
        fl, _ = preprocess(bio.preprocess_options(erode=False, sigma_d=R / 2, sigma_r=100.0), u16, col, (W, H))
        assert np.all(np.abs(fl - 2.0) < 1e-5), (R, W, H)
        # what one stray 0.0f tap at the largest distance would do: far more than that bound
        w_far = np.exp(-2 * R * R / (2 * (R / 2) ** 2))
        w_all = sum(np.exp(-(a * a + b * b) / (2 * (R / 2) ** 2)) for a in range(-R, R + 1) for b in range(-R, R + 1))
        assert 2.0 * w_far / w_all > 1e-5


def test_resample_maps_stay_inside():
    """Down- and upsampling of the resampling cases sample every output pixel (no pixel is left unwritten,
    which the zero-filled oracle output and an uninitialised device buffer would not agree on)."""
    for W, H in ((67, 19), (100, 37)):
        for ow, oh, iw, ih in ((W // 2 + 1, H // 2 + 1, W, H), (W + 9, H + 5, W, H), (W + 9, H + 5, W + 11, H + 6),
                               (W // 2 + 1, H // 2 + 1, W + 11, H + 6), (640, 480, 1296, 968), (320, 240, 1296, 968),
                               (320, 240, 640, 480), (34, 10, 67, 19)):
            xi = (np.arange(ow, dtype=np.float32) * (np.float32(iw - 1) / np.float32(ow - 1)) + np.float32(0.5)).astype(np.uint32)
            yi = (np.arange(oh, dtype=np.float32) * (np.float32(ih - 1) / np.float32(oh - 1)) + np.float32(0.5)).astype(np.uint32)
            assert xi.max() == iw - 1 and yi.max() == ih - 1 and xi.min() == 0 and yi.min() == 0


# ---- cache ---------------------------------------------------------------------------------------------
def cache_case(inp, out, col, seed=0, max_frames=1, **kw):
    (iW, iH), (W, H), (cW, cH) = inp, out, col
    f = FX * iW / 640
    o = cache_options(iW, iH, f, f, (iW - 1) / 2, (iH - 1) / 2, max_frames, width=W, height=H, **kw)
    d = depth_metres(sensor_frame(iW, iH, seed)[0])
    c = sensor_frame(cW, cH, seed + 100)[1]
    return o, d, c


@pytest.mark.parametrize("shape", [CACHE_TAIL] + CACHE_SHAPES[:2])
def test_cache_inputs_have_valid_and_invalid_normals_and_derivatives(shape):
    o, d, c = cache_case(*shape)
    r = cache_store_frame(o, d, c)
    W, H = shape[1]
    inner = (slice(1, H - 1), slice(1, W - 1))
    assert 0.6 < np.isfinite(r["depth"]).mean() < 1.0
    assert 0.3 < np.isfinite(r["normals"][..., 0]).mean() < 0.9
    nrm = np.isfinite(r["normals"][..., 0])
    assert np.all(r["normalsU8"][~nrm] == 0) and np.all(r["normalsU8"][nrm][:, :3].max(axis=1) > 0)
    # derivatives: -inf on the border ring, finite inside (the intensity is valid everywhere)
    dv = np.isfinite(r["intensityDeriv"][..., 0])
    assert dv[inner].all() and dv.sum() == (W - 2) * (H - 2)
    assert np.ptp(r["intensity"]) > 0.01


def test_cache_tail_shape_is_off_every_grid():
    (iW, iH), (W, H), (cW, cH) = CACHE_TAIL
    assert (W * H) % 64 == 17 and W % 8 and H % 8 and (cW, cH) != (iW, iH) and (cW, cH) != (W, H)


def test_cache_radii_change_the_outputs():
    """Each filter radius of the nine-store sweep gives different depth / intensity bits from its neighbour's,
    so a store that picked the wrong instantiation cannot pass."""
    sig = [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5]
    outs = []
    for s in sig:
        o, d, c = cache_case(*CACHE_TAIL, color_sigma=s, depth_sigma_d=s)
        outs.append(cache_store_frame(o, d, c))
    for a, b in zip(outs, outs[1:]):
        assert not np.array_equal(bits(a["depth"]), bits(b["depth"]))
        assert not np.array_equal(bits(a["intensity"]), bits(b["intensity"]))


# ---- EntryJ producer -----------------------------------------------------------------------------------
def corr_opts(stride, max_pp, min_pp):
    return corr_options(CORR_W, CORR_H, *corr_intrinsics(), stride=stride, max_per_pair=max_pp, min_per_pair=min_pp)


@functools.lru_cache(maxsize=None)
def oracle_counts(n, cur, start, stride, max_pp, min_pp):
    images, sel, T, Tinv = corr_problem(n)
    e, total = or_corr([images[s] for s in sel], T, Tinv, cur, start, corr_opts(stride, max_pp, min_pp), 1 << 17)
    assert total == len(e)
    return np.bincount(e["i"], minlength=cur)[start:cur], total


@pytest.mark.parametrize("stride,max_pp,min_pp", CORR_OPTION_SETS)
@pytest.mark.parametrize("cur,start", [(1099, 0), (1099, 1034), (70, 3)])
def test_corr_problem_mixes_pair_classes(cur, start, stride, max_pp, min_pp):
    cnt, total = oracle_counts(1100, cur, start, stride, max_pp, min_pp)
    pairs = cur - start
    empty, capped = (cnt == 0).sum(), (cnt == max_pp).sum()
    between = pairs - empty - capped
    assert empty >= 0.1 * pairs and capped >= 0.1 * pairs
    if max_pp > 1:
        assert between >= 0.1 * pairs
    else:
        assert between == 0
    assert total == cnt.sum() and np.all(cnt <= max_pp)
    if min_pp > 1:   # the drop runs: pairs with 1 .. minPerPair - 1 raw matches exist and contribute nothing
        raw, _ = oracle_counts(1100, cur, start, stride, max_pp, 1)
        dropped = (raw > 0) & (raw < min_pp)
        assert dropped.sum() >= 1 and np.all(cnt[dropped] == 0) and np.array_equal(cnt[~dropped], raw[~dropped])


def test_corr_grids_cover_the_round_cases():
    n = [(CORR_W // s) * (CORR_H // s) for s, _, _ in CORR_OPTION_SETS]
    assert n == [54, 234, 140, 408]              # < 256 three times; 408 = 256 + 152: a partial second round
    assert CORR_W % 5 and CORR_W % 8 == 0 and CORR_H % 8   # widths that are and are not multiples of the stride
    assert [c - s for c, s in CORR_WINDOWS] == [1099, 65, 67, 64, 65, 1025, 1024, 1, 0]
    # both rounds run: the pairs in between scan all 408 candidates
    cnt, _ = oracle_counts(1100, 1099, 0, 3, 64, 1)
    assert ((cnt > 0) & (cnt < 64)).sum() > 100


def test_corr_degenerate_poses_on_the_oracle():
    images, sel, T, Tinv = corr_problem(70)
    depths = [images[s] for s in sel]
    o = corr_opts(8, 25, 1)
    base, _ = or_corr(depths, T, Tinv, 69, 0, o, 1 << 14)
    # an invalid pose (-inf everywhere): no match with that frame as i, the other pairs unchanged
    bad = next(k for k in range(10, 69) if (base["i"] == k).sum() > 0)
    Tb = T.copy()
    Tb[bad] = -np.inf
    e, total = or_corr(depths, Tb, pose_inverse(Tb), 69, 0, o, 1 << 14)
    assert total == len(base) - (base["i"] == bad).sum() and e.tobytes() == base[base["i"] != bad].tobytes()
    # ... and none at all when it is cur
    Tc = T.copy()
    Tc[69] = -np.inf
    assert or_corr(depths, Tc, pose_inverse(Tc), 69, 0, o, 1 << 14)[1] == 0
    # cur almost on the wall: pj.z ~ 1e-6, the projection is far outside the image, nothing matches with cur = 69;
    # pushed 40 m sideways as well, the projected pixel is beyond +-2^31 and the conversion saturates
    for dx in (0.0, 40.0, -40.0):
        Tz = T.copy()
        Tz[69, 2, 3] = np.float32(2.0 - 1e-6)
        Tz[69, 0, 3] += np.float32(dx)
        Tzi = pose_inverse(Tz)
        f = corr_intrinsics()[0]
        pz = np.float32(2.0) + Tzi[69, 2, 3]
        assert 0 < pz < 2e-6
        if dx:
            assert (abs(dx) - 3.0) * f / pz > 2.0 ** 31   # |pj.x| >= |dx| - 3 m
        assert or_corr(depths, Tz, Tzi, 69, 0, o, 1 << 14)[1] == 0
        assert or_corr(depths, Tz, Tzi, 68, 0, o, 1 << 14)[1] > 0   # the other windows still match
