"""CPU checks of the SIFT detector (bf_sift_*): the ABI additions, the argument checks, the host-built filter tables
against the restatement, known answers of the restatement itself (tests/sift_ref.py), and the conditions the GPU
fixtures rely on. No GPU calls."""
import ctypes as C
import math

import numpy as np
import pytest

import bundlefusion_amd as bfa
from bundlefusion_amd import abi
from bundlefusion_amd import sift as bsift

import sift_ref as R

SIFT_NAMES = {"bf_sift_create", "bf_sift_destroy", "bf_sift_intensity", "bf_sift_detect", "bf_sift_result",
              "bf_sift_level_counts", "bf_sift_filter_kernel", "bf_sift_debug_level", "bf_sift_debug_raw_keys",
              "bf_sift_synchronize", "bf_sift_timer_start", "bf_sift_timer_stop"}


def test_abi_additions():
    names = {n for n in abi.header_functions() if n.startswith("bf_sift_")}
    assert names == SIFT_NAMES
    L = C.CDLL(abi.LIB_PATH)
    assert all(hasattr(L, n) for n in SIFT_NAMES)
    n = C.c_size_t()
    assert bfa.lib().bf_abi_struct_size(b"BFSiftOptions", C.byref(n)) == 0
    assert n.value == C.sizeof(abi.BFSiftOptions) == 48
    text = open(abi.HEADER_PATH.replace("bf.h", "types.h")).read()
    assert "typedef struct BFSiftOptions" in text and "#define BF_SIFT_TRUNCATED 1u" in text
    assert bfa.lib().bf_abi_version() == 4
    assert bfa.Sift is bsift.Sift and bfa.sift_options is bsift.sift_options


def _create(o):
    h = C.c_void_p()
    rc = bfa.lib().bf_sift_create(C.byref(o) if o is not None else None, C.byref(h))
    return rc, bfa.lib().bf_last_error()


@pytest.mark.parametrize("field,value,msg", [
    ("width", 31, b"32...4096"), ("height", 24, b"32...4096"), ("width", 4097, b"32...4096"),
    ("depthWidth", 0, b"depth size"), ("depthHeight", 5000, b"depth size"), ("maxKeys", 1025, b"maxKeys"),
    ("dogThreshold", -1.0, b"threshold"), ("edgeThreshold", float("nan"), b"threshold"),
    ("minKeyScale", float("inf"), b"threshold"), ("sensorDepthMax", -0.5, b"threshold"),
    ("sensorDepthMin", 5.0, b"sensorDepthMin"),
])
def test_argument_checks_without_device(field, value, msg):
    o = bsift.sift_options(160, 120)
    setattr(o, field, value)
    rc, err = _create(o)
    assert rc == -2 and msg in err, (rc, err)


def test_null_arguments_without_device():
    rc, err = _create(None)
    assert rc == -2 and b"null" in err
    L = bfa.lib()
    o = bsift.sift_options(160, 120)
    assert L.bf_sift_create(C.byref(o), None) == -2
    for call in (lambda: L.bf_sift_detect(None, None, None), lambda: L.bf_sift_result(None, None, None, None, None),
                 lambda: L.bf_sift_intensity(None, None, 2, 2, None), lambda: L.bf_sift_level_counts(None, None, None),
                 lambda: L.bf_sift_debug_level(None, 0, 0, None), lambda: L.bf_sift_synchronize(None),
                 lambda: L.bf_sift_debug_raw_keys(None, 0, None, None, 0, None)):
        assert call() == -2 and b"null" in L.bf_last_error()
    assert L.bf_sift_destroy(None) == 0
    k = np.zeros(33, np.float32)
    assert L.bf_sift_filter_kernel(None, 6, k.ctypes.data_as(C.c_void_p), None) == -2


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_filter_tables_match_the_restatement():
    """Widths 13, 11, 13, 17, 21, 25. Coefficients within 4 ulp: the library and the restatement both take exp in
    double and round to float, but through different C library entry points whose double results may differ by 1 ulp
    (double); after the rounding to float that is at most 1 float ulp in a few taps, which moves the float sum of <= 25
    taps and its reciprocal by at most 2 ulp, and the product of the two by at most 1 + 2 + rounding = 4 ulp."""
    t = R.tables()
    assert t["widths"] == [13, 11, 13, 17, 21, 25]
    worst = 0
    for i in range(6):
        k = bsift.filter_kernel(i)
        assert len(k) == t["widths"][i]
        assert np.all(k > 0) and abs(float(k.sum(dtype=np.float64)) - 1.0) < 1e-6
        assert np.array_equal(k, k[::-1])
        worst = max(worst, int(_ulps(k, t["k"][i]).max()))
    print("filter tables: worst difference", worst, "ulp")
    assert worst <= 4
    assert abs(float(t["sigmas"][0]) - math.sqrt(1.6 ** 2 - 0.5 ** 2)) < 1e-6
    assert np.allclose(t["level_sigma"], [1.6 * 2 ** (1 / 3), 1.6 * 2 ** (2 / 3), 3.2], rtol=1e-6)


# ---- known answers of the restatement ------------------------------------------------------------------------------
def _flat_depth(w, h, z=2.0):
    return np.full((h, w), z, np.float32)


@pytest.mark.parametrize("sigma_b,level,col,row", [(4.0, 2, 80, 60), (8.0, 5, 40, 30)])
def test_isolated_blob_gives_one_key_at_its_centre(sigma_b, level, col, row):
    """A DoG level answers like the scale-normalised Laplacian at about the geometric mean of its two Gaussian sigmas
    (2.26, 2.85, 3.59 in octave 0, twice that in octave 1, in octave-0 pixels), and a Gaussian blob's Laplacian peaks
    over scale at its own sigma: sigma 4 belongs to level 2, sigma 8 to level 5 (octave 1, at half the coordinates)."""
    d = R.detect(R.blob_image(160, 120, 80, 60, sigma_b), _flat_depth(160, 120), R.cfg(160, 120), descriptors=False)
    found = [(L, r.tolist()) for L, r in enumerate(d["raw"]) if len(r)]
    assert found == [(level, [[col, row]])]
    assert len(d["keys"]) >= 1
    x, y, scale, depth = d["keys"][0]
    o = level // 3
    assert (x, y) == ((1 << o) * col + 0.5, (1 << o) * row + 0.5) and depth == 2.0
    assert scale == np.float32(1 << o) * R.tables()["level_sigma"][level % 3]


def _asym_image(n):
    img = np.full((n, n), 0.3, np.float32)
    for cx, cy, s, a in ((40.0, 50.0, 4.0, 0.5), (47.0, 50.0, 4.0, -0.2), (85.0, 40.0, 8.0, 0.4), (92.0, 48.0, 6.0, -0.2),
                         (60.0, 90.0, 5.0, 0.45), (66.0, 85.0, 4.0, -0.25)):
        img += R.blob_image(n, n, cx, cy, s, a) - np.float32(0.25)
    return img


def test_rotated_image_gives_rotated_keys():
    """np.rot90(img): old (col, row) -> new (col, row) = (row, n - 1 - col); a gradient (dx, dy) becomes (dy, -dx), so
    every orientation drops by a quarter turn. n = 129 keeps the octaves' every-second-pixel grids on the same pixels
    after the turn: in octave o, (col, row) -> (row, (128 >> o) - col). The separable filter adds its taps in another
    order after the turn, so levels agree to rounding, not bit for bit: the key sets must be equal and the
    orientations within 2e-3 rad."""
    n = 129
    img = _asym_image(n)
    a = R.detect(img, _flat_depth(n, n), R.cfg(n, n), descriptors=False)
    b = R.detect(np.ascontiguousarray(np.rot90(img)), _flat_depth(n, n), R.cfg(n, n), descriptors=False)
    assert sum(a["raw_counts"]) >= 4
    for L in range(R.LEVELS):
        ka = {(int(r), ((n - 1) >> (L // 3)) - int(c)) for c, r in a["raw"][L]}  # rotated: (new col, new row)
        kb = {(int(c), int(r)) for c, r in b["raw"][L]}
        assert ka == kb, L
    assert len(a["entries"]) == len(b["entries"]) >= 3
    fa = {(L, int(a["lists"][L][i][1]), ((n - 1) >> (L // 3)) - int(a["lists"][L][i][0]), k): float(o)
          for L, i, k, o in a["entries"]}
    fb = {(L, int(b["lists"][L][i][0]), int(b["lists"][L][i][1]), k): float(o) for L, i, k, o in b["entries"]}
    assert fa.keys() == fb.keys()
    for key, oa in fa.items():
        diff = (fb[key] - (oa - math.pi / 2) + math.pi) % (2 * math.pi) - math.pi
        assert abs(diff) < 2e-3, (key, oa, fb[key])


def test_invalid_depth_removes_the_key():
    img, depth, c = R.fixture("small")
    d = R.fixture_detect("small", "f64", False)
    L = max(range(R.LEVELS), key=lambda l: len(d["raw"][l]))
    col, row = d["raw"][L][0]
    dx, dy = R.depth_pixel(c, L // 3, col, row)
    for bad in (-np.inf, 0.05, 4.5):
        dep = depth.copy()
        dep[dy, dx] = bad
        r2 = R.raw_keys_level(d["g"][L // 3][L % 3:L % 3 + 4], L // 3, dep, c)
        gone = {tuple(k) for k in d["raw"][L].tolist()} - {tuple(k) for k in r2.tolist()}
        assert (int(col), int(row)) in gone
        assert all(tuple(R.depth_pixel(c, L // 3, cc, rr)) == (dx, dy) for cc, rr in gone)
    none = R.raw_keys(d["g"], np.full_like(depth, -np.inf), c)
    assert sum(len(r) for r in none) == 0


def test_cap_and_limit_rules():
    assert R.fmax(640, 480) == 1536 and R.fmax(320, 240) == 384 and R.fmax(80, 60) == 32 and R.fmax(4096, 4096) == 4096
    assert R.fmaxs(R.cfg(160, 120)) == [96] * 3 + [32] * 9
    # per-level cap, then LimitFeatureCount(0): finest levels are emptied while the rest still exceeds 150
    assert R.cap_and_limit([100, 40, 40] + [40, 10, 10] + [5] * 6, [96] * 3 + [32] * 9, 150) == \
        [0, 40, 40, 32, 10, 10, 5, 5, 5, 5, 5, 5]  # 258 - 96 = 162 > 150, 162 - 40 = 122: stop
    assert R.limit([50, 50, 50, 50, 0, 0, 0, 0, 0, 0, 0, 10], 150) == [0, 50, 50, 50, 0, 0, 0, 0, 0, 0, 0, 10]
    assert R.limit([10] * 12, 150) == [10] * 12
    assert R.limit([0, 0, 200, 1] + [0] * 8, 150) == [0, 0, 200, 1] + [0] * 8  # 201 - 200 = 1: level 2 stays
    # the guard: a threshold nothing can meet empties every level and stops at the last
    assert R.limit([5] * 12, -1) == [0] * 12
    # hard cap: coarsest levels whole, the crossing level its first keys
    assert R.hard_cap([0, 0, 30, 20, 10, 10, 5, 0, 0, 0, 0, 1], 64) == ([0, 0, 18, 20, 10, 10, 5, 0, 0, 0, 0, 1], True)
    assert R.hard_cap([0, 0, 30, 20, 10], 64) == ([0, 0, 30, 20, 10], False)
    assert R.hard_cap([100, 100], 64) == ([0, 64], True)


# ---- the conditions the GPU fixtures rely on ------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PARITY)
def test_fixture_conditions(name):
    d = R.fixture_detect(name)
    n = len(d["entries"])
    print(name, "raw", d["raw_counts"], "kept", d["kept"], "final", n, "borderline keys", int(d["key_border"].sum()),
          "borderline bytes", int(d["byte_border"].sum()), "reaches 256:", d["reach256"])
    assert n >= 40
    assert d["key_border"].mean() <= 0.05
    assert d["byte_border"].mean() <= 0.02
    assert np.all(d["keys"][:, 3] >= 0.1) and np.all(d["keys"][:, 3] <= 4.0)
    assert not d["reach256"]  # no fixture reaches the byte wrap


def test_cap_fixtures_exceed_their_caps():
    _, _, c = R.fixture("dense")
    d = R.fixture_detect("dense")
    over = [L for L in range(3, 6) if d["raw_counts"][L] > R.fmaxs(c)[L]]
    assert over and all(len(d["lists"][L]) == 32 for L in over)  # an octave-1 level beyond its cap of 32
    d = R.fixture_detect("medium")
    raw, lst = d["raw_counts"], [len(x) for x in d["lists"]]
    assert sum(raw) > 150 and lst[0] == 0 and raw[0] > 0  # the soft limit empties levels
    assert sum(lst) - lst[[i for i, v in enumerate(lst) if v][0]] <= 150
    h = R.fixture_detect("hardcap")
    assert h["truncated"] and len(h["entries"]) == 64 and len(d["entries"]) > 64
    assert h["kept"][-1] == d["kept"][-1] and sum(h["kept"]) == 64
    _, _, c = R.fixture("product")
    p = R.fixture_detect("product", "f64", False)
    assert sum(p["raw_counts"]) > 500 and sum(1 for a, b in zip(p["raw_counts"], [len(x) for x in p["lists"]]) if a and not b) >= 3


def test_small_fixture_shapes():
    """Octave 3 of 160 x 120 is 20 x 15: narrower than the 25-tap filter; 172 x 130 is odd at every octave."""
    g = R.fixture_detect("small", "f64", False)["g"]
    assert g[3][5].shape == (15, 20) and R.tables()["widths"][5] == 25
    g = R.fixture_detect("odd", "f64", False)["g"]
    assert [g[o][0].shape for o in range(4)] == [(130, 172), (65, 86), (32, 43), (16, 21)]


# ---- end to end on the CPU ----------------------------------------------------------------------------------------------
def test_restatement_chain_keeps_the_matches():
    """Three 320 x 240 views through the restatement and match_ref.run: every consecutive pair keeps at least
    minNumMatches filtered matches; the pose error against the truth is what the GPU test's bar is twice of."""
    e = R.e2e_reference()
    for prev in (0, 1):
        print("pair", prev, "filtered", e["counts"][prev], "translation error %.4f m" % e["t_err"][prev],
              "rotation error %.5f rad" % e["r_err"][prev])
        assert e["counts"][prev] >= 5
        assert e["t_err"][prev] < 0.05 and e["r_err"][prev] < 0.03
