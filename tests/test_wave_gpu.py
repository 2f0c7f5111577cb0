"""csrc/wave.h's workgroup scan and ballot compaction, run directly (bf_debug_wg_scan) at every workgroup size the
kernels use and at input lengths around the wave, the workgroup and the second round: the kernels that share the
helpers reach them only at their own sizes. uint32 sums wrap, so every output word and the total are compared
exactly with NumPy's uint32 cumsum shifted by one."""
import ctypes as C

import numpy as np
import pytest

import bundlefusion_amd as bfa

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


def lengths(wg):
    return [0, 1, 63, 64, 65, wg - 1, wg, wg + 1, 2 * wg + 3]


def exclusive(v):
    """(exclusive uint32 prefix sums, total) of v, wrapping."""
    incl = np.cumsum(v, dtype=np.uint32)
    return np.concatenate([np.zeros(1, np.uint32), incl[:-1]])[: v.size], np.uint32(incl[-1] if v.size else 0)


@pytest.mark.parametrize("wg", [256, 512, 1024])
def test_wg_scan_and_compact(wg):
    L = bfa.lib()
    rng = np.random.default_rng(wg)
    nmax = 2 * wg + 3
    wide = rng.integers(0, 1 << 32, nmax, dtype=np.uint64).astype(np.uint32)  # full range: the sums wrap
    bits = rng.integers(0, 2, nmax, dtype=np.uint64).astype(np.uint32)
    assert int(wide[:wg].astype(np.uint64).sum()) >= 1 << 32
    d_out = bfa.DeviceArray(nmax, np.uint32)
    d_total = bfa.DeviceArray(1, np.uint32)
    blank = np.full(nmax, SENTINEL, np.uint32)
    for name, host, flags, counted in (("wide", wide, 0, wide), ("0/1", bits, 0, bits), ("0/1 flags", bits, 1, bits),
                                       ("wide flags", wide, 1, (wide != 0).astype(np.uint32))):
        d_in = bfa.DeviceArray.from_host(host)
        for n in lengths(wg):
            d_out.upload(blank)
            d_total.upload(np.full(1, SENTINEL, np.uint32))
            bfa.check(L.bf_debug_wg_scan(d_in.ptr, C.c_uint32(n), C.c_uint32(wg), C.c_int(flags), d_out.ptr, d_total.ptr))
            want, total = exclusive(counted[:n])
            got = d_out.download()
            what = f"{name}, wg {wg}, n {n}"
            assert np.array_equal(got[:n], want), what
            assert np.all(got[n:] == SENTINEL), what  # nothing written past the input
            assert d_total.download()[0] == total, what
