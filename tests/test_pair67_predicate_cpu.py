"""The per-sphere predicate of pair (6,7)'s skip (pt_trace.h sphere_reachable_mask: a lane is outside the mask when med3(disc, b, -c)
>= -2^-60 fails) may only hold where the oracle's root selection on disc = b*b - c returns the miss value, for every eps >= 0: the
kernel then leaves the sphere's root stage out.  More than 10^7 float32 triples (b, c, eps):

  random      b and c with random signs and exponents over the whole float32 range, and of the scenes' magnitudes
  structured  c around 0 and denormal, b around the guard 2^-60 and around +-2^+-63 (b*b at the ends of the normal range), disc on both
              sides of 0 (c within a few ulps of b*b), infinities and NaNs; all crossed with each other
  scene       the real (b, c) of spheres 6 and 7 at every bounce of every path of a 48x32 frame of the reference scene at 16 samples
              (tests/pair67_ref.py: the oracle's bounce restated, checked against the oracle's colours)

"The miss value" is kMissT = 1e20 bit for bit wherever b*b is finite.  Where b*b overflows (|b| >= 2^64) and b < 0, the oracle's
t1 = b + sqrt(inf) is +inf, which passes "t > eps" and comes back as +inf, not as kMissT: the test then asks for t >= kMissT, which is
what "cannot be hit" means to the arg-min (strict '<' from kMissT on: the kernel's key of +inf is >= key(kMissT) as well), so leaving
the stage out changes nothing there either.

The predicate must also HOLD for at least a third of the scene's triples (it does for 0.913 of them: the ball is small and the light
is behind every ray that points down), so the test cannot pass by the predicate never holding."""
import numpy as np

import pair67_ref as pr

f = np.float32
EPS = np.array([0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -70, 2.0 ** -60, 1e-10, 1e-4, 0.5, 3.0e4, 2.0 ** 100], dtype=f)


def _check(b, c, eps, what):
    """-> how many triples satisfy the predicate; asserts that each of them is a miss."""
    b, c, eps = np.broadcast_arrays(np.asarray(b, f), np.asarray(c, f), np.asarray(eps, f))
    with np.errstate(all="ignore"):
        disc = b * b
        disc = disc - c
    assert disc.dtype == np.float32
    holds = pr.cannot_hit(b, c, disc)
    t = pr.intersect_post(b, disc, eps)
    with np.errstate(all="ignore"):
        overflow = np.isinf(b * b)                             # |b| >= 2^64: disc = inf, q = inf, t1 = b + inf = +inf (see the docstring)
    bad = holds & np.where(overflow, ~(t >= pr.MISS_T), t != pr.MISS_T)
    assert not bad.any(), (what, [(b[i].item().hex(), c[i].item().hex(), eps[i].item().hex(), t[i].item()) for i in np.argwhere(bad)[:5, 0]])
    return int(holds.sum()), holds.size


def _random_floats(rng, n, emin, emax):
    """random sign, exponent uniform in [emin, emax), random mantissa"""
    m = rng.uniform(1.0, 2.0, n)
    e = rng.randint(emin, emax, n)
    s = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    with np.errstate(all="ignore"):
        return (s * np.ldexp(m, e)).astype(f)


def test_random_triples():
    rng = np.random.RandomState(67)
    n, total, held = 1 << 20, 0, 0
    for emin, emax in ((-149, 128), (-10, 20), (-70, -50)):
        for eps in (f(0.0), f(1e-4), None):
            b, c = _random_floats(rng, n, emin, emax), _random_floats(rng, n, 2 * emin if emin > -70 else -149, min(2 * emax, 128))
            e = np.abs(_random_floats(rng, n, -149, 20)) if eps is None else eps
            h, m = _check(b, c, e, ("random", emin, emax))
            held, total = held + h, total + m
    print("random: predicate holds for", held, "of", total)
    assert total >= 9 * n and held > total // 10


def _neighbours(x, k=3):
    """x and its k float32 neighbours to either side"""
    x = np.atleast_1d(np.asarray(x, f))
    out = [x]
    lo, hi = x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, f(-np.inf)), np.nextafter(hi, f(np.inf))
        out += [lo, hi]
    return np.concatenate(out)


def test_structured_triples():
    rng = np.random.RandomState(76)
    edge = np.array([2.0 ** e for e in (-149, -140, -127, -126, -125, -76, -75, -74, -64, -63, -62, -61, -60, -59, -58, -30, -1, 0, 1, 30,
                                        62, 63, 64, 65, 100, 127)], dtype=np.float64)
    mags = _neighbours(np.concatenate([edge, 1.5 * edge[2:-1], 1.9999999 * edge[2:-1]]).astype(f))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=f)
    b = np.unique(np.concatenate([mags, -mags, special]).view(np.uint32)).view(f)          # ~1000 values
    # c: the same edges, and for every b a handful of values within a few ulps of b*b (disc on both sides of 0 and exactly 0)
    with np.errstate(all="ignore"):
        near = np.stack([_neighbours(x * x, 2) for x in b]).astype(f)                      # [nb][5]
    total = held = 0
    for eps in EPS:
        h, m = _check(b[:, None], b[None, :], eps, "edges x edges")                        # every c from the same set
        held, total = held + h, total + m
        h, m = _check(b[:, None], near, eps, "disc around 0")
        held, total = held + h, total + m
        h, m = _check(b[:, None], -near, eps, "c = -b*b")
        held, total = held + h, total + m
    # the guard's neighbourhood densely: b in -(2^-66 .. 2^-56), c denormal .. 2^-100 and around b*b
    bb = -np.abs(_random_floats(rng, 1 << 19, -66, -56))
    for c in (np.abs(_random_floats(rng, 1 << 19, -149, -100)), (bb.astype(np.float64) ** 2 * rng.uniform(0.5, 1.5, bb.size)).astype(f)):
        for eps in (f(0.0), f(2.0 ** -149), f(2.0 ** -70)):
            h, m = _check(bb, c, eps, "guard")
            held, total = held + h, total + m
    print("structured: predicate holds for", held, "of", total)
    assert total >= 10 ** 7 and held > total // 10


def test_scene_triples(oracle):
    b, c, disc = pr.trace(oracle, "ref")
    b, c = b[:, 6:8].ravel(), c[:, 6:8].ravel()
    assert np.array_equal((b * b - c).view(np.uint32), disc[:, 6:8].ravel().view(np.uint32))
    held = None
    for eps in EPS:
        h, m = _check(b, c, eps, "scene")
        held = h if held is None else held
        assert h == held                                       # the predicate does not depend on eps
    print("scene: predicate holds for", held, "of", b.size, "=", round(held / b.size, 4))
    assert b.size == 8 * 2 * pr.W * pr.H * 4 * pr.S
    assert 3 * held >= b.size                                  # not vacuous
    # both parts of the predicate carry weight: a sphere behind the ray whose line still crosses it
    behind = pr.cannot_hit(b, c, b * b - c) & (disc[:, 6:8].ravel() >= 0)
    print("scene: of these, disc >= 0 (sphere behind the ray):", int(behind.sum()))
    assert behind.sum() > b.size // 20
