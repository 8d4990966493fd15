"""apt_selftest_div3_seeded: the divide of the two-path bounce (pt_core.h div3_seeded_packed2 -- the reciprocal refined from the square
root's v_rsq_f32 seed by two Newton steps, ONE residual round per quotient, and a flag, e1 == 2^-24, for the divisors with an all-ones
mantissa whose reciprocal did not converge) against the device's `/`, bit for bit.

  (a) the operand sets of apt_selftest_div3's generator (all three ways of forming the divisor, special mantissas, exponent edges,
      signed zeros), the same 2^32 sets tests/test_gpu_parity.py runs the old forms on
  (b) every float bit pattern as len2, d = sqrtf(len2), the instruction's own seed: finds the reciprocal's exception set
  (c) EVERY divisor with an all-ones mantissa that the validity chain accepts, d = 2^k (2 - 2^-23) for k = -29 .. 28 (d <= 2^29, and a
      numerator |n| >= 2^-29 at or below the divisor's exponent exists), against all 2^23 numerator mantissas at up to three exponents
      (the divisor's, one and twelve below, as far as they stay >= 2^-29), from the v_rsq_f32 seed of every len2 next to d * d whose
      sqrtf() is d and from three synthetic seeds RN(1/d) - 1, + 0, + 1 ulp.  It is the one family (b) shows flagged; (b) must show no
      other divisor whose refined reciprocal is not RN(1/d), so the "or whose r2 differed" half of the issue's set is empty.

Acceptance: a set is accepted when div3_operands_ok() holds -- the predicate the OLD packed form is tested under, so the new form's
operand range is the old one's, set for set -- and the flag is not raised.  apt_selftest_div3 reports ONE accepted count for its two
forms (the scalar form's own, wider, flags and the packed form's predicate); the new entry recounts both on the same sets, the sum must
equal the old entry's figure (that ties the new kernel's sets and predicate to the old kernel's), and since the new kernel accepts
exactly the sets in that range whose flag is down, what the new form rejects is what the old packed form rejects plus the flagged
sets -- every one of which must have an all-ones divisor (flagged_other == 0).  Those two assertions carry the reject-share check; the
literal comparison of shares with apt_selftest_div3's single figure would compare one form with the sum of two."""
import struct

import pytest


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()                   # a no-op when the in-tree library is current
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, render
    _lib.require_gpu()
    pkg.render = render
    return pkg


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@pytest.mark.gpu
def test_generator_sets_and_reject_share(apt):
    n = 1 << 32
    new = apt.render.selftest_div3_seeded(part=0, first=0, count=n)
    old_bad, _, old_accepted = apt.render.selftest_div3(first=0, count=n)
    print("seeded, generator sets:", new, "old entry accepted:", old_accepted)
    assert new["bad"] == 0, new
    assert new["accepted"] > 0
    assert new["flagged_other"] == 0, new
    assert old_bad == 0
    # the same sets, the same predicate: the old entry's accepted count is the two forms' together
    assert new["in_range"] + new["shared_ok"] == old_accepted, (new, old_accepted)
    # the generator gives an all-ones divisor to half of a quarter of the third of its sets that take the divisor independently (1/24),
    # and to a square root now and then
    assert new["flagged"] <= n // 24 + n // 1000, new
    assert new["recip_off"] == 0, new


@pytest.mark.gpu
def test_every_len2_with_the_real_seed(apt):
    r = apt.render.selftest_div3_seeded(part=1, first=0, count=1 << 32)
    print("seeded, every len2:", r)
    assert r["bad"] == 0, r
    # len2 in [2^-58, 2^58] up to the seed's last ulp, 116 binades of 2^23 patterns: the triple at the divisor's own exponent is in
    # range on all of them, the three triples up to 13 binades below it on the 90 binades from 2^-32 up at least
    assert r["accepted"] > (116 + 3 * 90 - 6) * (1 << 23), r
    assert r["flagged_other"] == 0, r
    assert r["flagged"] <= 4 * 4 * 120, r       # at most the len2 values whose square root has an all-ones mantissa (<= 4 per binade of d), x 4 triples
    assert r["recip_off"] == 0, r               # no divisor outside the flagged family has a refined reciprocal that is not RN(1/d)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(-29, 29))
def test_all_ones_divisors_against_every_numerator(apt, k):
    """d = 2^k (2 - 2^-23).  rsq(len2) >= 2^-29 needs d <= 2^29: k <= 28.  The numerator classes sit 0, 1 and 12 binades below the
    divisor's and must reach 2^-29: class 0 from k = -29, class 1 from -28, class 2 from -17 on."""
    d = (2.0 - 2.0 ** -23) * 2.0 ** k
    classes = 1 + (k >= -28) + (k >= -17)
    r = apt.render.selftest_div3_seeded(part=2, first=_bits(d), count=3 << 23)
    print("seeded, all-ones divisor 2^%d:" % k, r)
    assert r["bad"] == 0, r
    assert r["flagged_other"] == 0 and r["recip_off"] == 0, r
    # per numerator the three synthetic seeds are in range, and so is every len2 of the divisor (at least one exists); of the
    # synthetic ones RN(1/d) itself converges, so it is accepted for every numerator of a class in range
    assert r["in_range"] >= 4 * classes << 23, r
    assert r["accepted"] >= classes << 23, r
    assert r["in_range"] % (classes << 23) == 0 and r["accepted"] + r["flagged"] == r["in_range"], r


@pytest.mark.gpu
@pytest.mark.parametrize("mantissa", (0x7ffffe, 0x000000, 0x000001, 0x3504f3))
def test_neighbouring_divisors_against_every_numerator(apt, mantissa):
    """The neighbours of the all-ones family, a power of two, and RN(sqrt(2)): never flagged, every seed accepted (the three
    synthetic ones and the seed of at least one len2 whose square root is the divisor)."""
    r = apt.render.selftest_div3_seeded(part=2, first=(127 << 23) | mantissa, count=3 << 23)
    print("seeded, divisor mantissa %06x:" % mantissa, r)
    assert r["bad"] == 0 and r["flagged"] == 0 and r["recip_off"] == 0, r
    assert r["accepted"] >= 4 * (3 << 23), r    # the three synthetic seeds and at least one len2 of the divisor


def test_entry_rejects_bad_arguments():
    """(No GPU: argument checks come before any launch.)"""
    import ctypes
    import __graft_entry__ as g
    g.build()
    from ascendpathtracing_amd import _lib
    L = _lib.lib()
    res = (ctypes.c_uint64 * 8)()
    assert L.apt_selftest_div3_seeded(None, 0, ctypes.c_uint64(0), ctypes.c_uint64(1), None) == 1
    assert L.apt_selftest_div3_seeded(None, 3, ctypes.c_uint64(0), ctypes.c_uint64(1), res) == 1
    assert L.apt_selftest_div3_seeded(None, 1, ctypes.c_uint64(1), ctypes.c_uint64(1 << 32), res) == 1
    assert L.apt_selftest_div3_seeded(None, 2, ctypes.c_uint64(1 << 32), ctypes.c_uint64(1), res) == 1
    assert L.apt_selftest_div3_seeded(None, 2, ctypes.c_uint64(0x3f800000), ctypes.c_uint64((3 << 23) + 1), res) == 1
    assert L.apt_selftest_div3_seeded(None, 0, ctypes.c_uint64(0), ctypes.c_uint64(0), res) == 0
