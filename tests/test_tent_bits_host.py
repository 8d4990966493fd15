"""CPU: the tent filter made straight from the generator's bits (pt_core.h tent_e_from_bits, tent_e: 52 bits under exponent 0x400,
e = v - 3, x = 1 - |e|, copysign(sqrt(x) - 1, e)) against the form from the uniform itself, tent_t<false>(unit_from_bits(z)), through
the host self-test apt_selftest_tent_bits_host: the square-root arguments equal bit for bit, the results equal except the sign of the
zero at r == 1 exactly (mantissa 2^51)."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()                   # a no-op when the in-tree library is current
    import ascendpathtracing_amd as pkg
    return pkg


def _selftest(apt, z):
    L = apt._lib.lib()
    z = np.ascontiguousarray(z, dtype=np.uint64)
    res = np.zeros(2, dtype=np.uint64)
    rc = L.apt_selftest_tent_bits_host(z.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(z.size), res.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, L.apt_last_error()
    return int(res[0]), int(res[1])


def _outputs(mantissas, low_bits):
    """64-bit generator outputs whose 52 high bits are the mantissas; the 12 low bits (dropped by both forms) from low_bits."""
    m = np.asarray(mantissas, dtype=np.uint64)
    return (m << np.uint64(12)) | (np.asarray(low_bits, dtype=np.uint64) & np.uint64(0xFFF))


def edge_mantissas():
    top = 1 << 52
    m = set()
    for c in (0, 1 << 50, 1 << 51, 3 << 50, top - 1):                   # r = 0, 0.5, 1, 1.5, 2 - 2^-51: within +-2
        m.update(c + d for d in range(-2, 3))
    for k in range(53):                                                  # every power of two and its complement to 2^52: within +-1
        for c in (1 << k, top - (1 << k)):
            m.update(c + d for d in range(-1, 2))
    return np.array(sorted(v for v in m if 0 <= v < top), dtype=np.uint64)


def test_ten_million_seeded_outputs(apt):
    rng = np.random.default_rng(20250)
    z = rng.integers(0, 1 << 64, size=10_000_000, dtype=np.uint64)
    assert _selftest(apt, z) == (0, 0)


def test_edge_mantissas(apt):
    m = edge_mantissas()
    assert m.size > 300 and (1 << 51) in m.tolist() and 0 in m.tolist() and (1 << 52) - 1 in m.tolist()
    for low in (0, 0xFFF, 0x5A5):
        assert _selftest(apt, _outputs(m, np.full(m.size, low))) == (0, 0), low


def test_the_only_zero_results_are_mantissa_two_to_the_51(apt):
    """What the self-test forgives is a zero against a zero, and a zero result needs sqrt(x) == 1, x == 1, r == 1.  In numpy, on the
    edge mantissas: the form from the uniform gives a zero at mantissa 2^51 and nowhere else."""
    m = edge_mantissas()
    u = ((m | np.uint64(0x3FF << 52)).view(np.float64)) - 1.0
    r = 2 * u
    x = np.where(r < 1, r, 2 - r)
    t = np.sqrt(x) - 1
    res = np.where(r < 1, t, -t)
    assert (m[res == 0] == np.uint64(1 << 51)).all() and (res == 0).sum() == 1
    # and the bits form, restated: v in [2, 4), e = v - 3, x = 1 - |e|
    e = ((m | np.uint64(0x400 << 52)).view(np.float64)) - 3.0
    assert np.array_equal((1.0 - np.abs(e)).view(np.uint64), x.view(np.uint64))
    assert np.array_equal(e < 0, r < 1)


def test_the_entry_checks_its_arguments(apt):
    L = apt._lib.lib()
    res = np.zeros(2, dtype=np.uint64)
    z = np.zeros(4, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.apt_selftest_tent_bits_host(None, ctypes.c_uint64(4), p(res)) == 1
    assert L.apt_selftest_tent_bits_host(p(z), ctypes.c_uint64(4), None) == 1
    assert L.apt_selftest_tent_bits_host(p(z), ctypes.c_uint64(0), p(res)) == 0 and not res.any()
