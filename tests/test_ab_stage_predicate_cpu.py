"""The joint skip of the (A, B)-packed intersection (pt_trace2.h intersect2_ns8_planes, SKIP) leaves a sphere's root stage out when,
in every lane and for both of its paths, sphere_reachable_mask()'s statement holds:  disc < 0 or NaN,  or  b < -2^-60 and c > 2^-60.
A pair (b, c) that the statement marks must be a miss in the reference's own sequence -- disc = b*b - c, sqrtf, both roots, select_root
with the default eps, every operation in float32 as the oracle orders them (tests/pair67_ref.py intersect_post) -- or leaving the
stage out would change a frame.  Checked on more than 10^7 seeded pairs:

  random      signs and exponents over the whole float32 range, the scenes' magnitudes, and the guard's neighbourhood
  structured  +-0, denormals, |b| around 2^-60 and around 2^64, c in {-1024, -0, +0, 1024} (what a wall's c is at the surface a ray has
              just left), infinities and NaN, all crossed; at least a tenth of them must be marked and at least a tenth not
  scene       the (b, c) of all eight spheres at every bounce of every path of a 48x32 frame of the reference scene

"A miss" is kMissT = 1e20 bit for bit wherever b*b is finite.  Where b*b overflows (|b| >= 2^64) with b < 0 the sequence gives
t1 = b + sqrt(inf) = +inf, which passes "t > eps" and comes back as +inf: not below kMissT, so it wins no strict-'<' arg-min either,
and the check there is t >= kMissT.

The kernel evaluates the statement for a lane's two paths with two v_med3_f32, one v_max_f32 -- a NaN operand drops out -- and one
compare; that this is "marked in path A and marked in path B" is checked on the structured set crossed with itself."""
import numpy as np

import pair67_ref as pr

f = np.float32


def _eps(oracle):
    return f(oracle.make_params(16, 16, 16).eps)


def _check(b, c, eps, what):
    """-> (marked, total); asserts that every marked pair is a miss."""
    b, c = np.broadcast_arrays(np.asarray(b, f), np.asarray(c, f))
    with np.errstate(all="ignore"):
        disc = b * b
        disc = disc - c
        overflow = np.isinf(b * b)
    assert disc.dtype == np.float32
    marked = pr.cannot_hit(b, c, disc)
    t = pr.intersect_post(b, disc, eps)
    bad = marked & np.where(overflow, ~(t >= pr.MISS_T), t != pr.MISS_T)
    assert not bad.any(), (what, [(b[i].item().hex(), c[i].item().hex(), t[i].item()) for i in map(tuple, np.argwhere(bad)[:5])])
    return int(marked.sum()), marked.size


def _random_floats(rng, n, emin, emax):
    m = rng.uniform(1.0, 2.0, n)
    e = rng.randint(emin, emax, n)
    s = np.where(rng.rand(n) < 0.5, -1.0, 1.0)
    with np.errstate(all="ignore"):
        return (s * np.ldexp(m, e)).astype(f)


def _neighbours(x, k=2):
    x = np.atleast_1d(np.asarray(x, f))
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo, hi = np.nextafter(lo, f(-np.inf)), np.nextafter(hi, f(np.inf))
        out += [lo, hi]
    return np.concatenate(out)


def _structured():
    mags = _neighbours(np.array([2.0 ** e for e in (-149, -140, -127, -126, -75, -74, -61, -60, -59, -30, 0, 10, 30, 63, 64, 65, 100, 127)], dtype=f))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=f)
    b = np.unique(np.concatenate([mags, -mags, special]).view(np.uint32)).view(f)
    c = np.unique(np.concatenate([_neighbours(np.array([1024.0, -1024.0], dtype=f)), mags, -mags, special]).view(np.uint32)).view(f)
    return b, c


def test_random_pairs(oracle):
    rng = np.random.RandomState(1967)
    eps, n, total, marked = _eps(oracle), 1 << 21, 0, 0
    for emin, emax in ((-149, 128), (-10, 20), (-70, -50), (55, 70)):
        b = _random_floats(rng, n, emin, emax)
        c = _random_floats(rng, n, max(2 * emin, -149), min(2 * emax, 128))
        h, m = _check(b, c, eps, ("random", emin, emax))
        marked, total = marked + h, total + m
        h, m = _check(b, rng.choice(np.array([-1024.0, -0.0, 0.0, 1024.0], dtype=f), n), eps, ("random b, wall c", emin, emax))
        marked, total = marked + h, total + m
    print("random: marked", marked, "of", total)
    assert total >= 10 ** 7 and marked > total // 10


def test_structured_pairs(oracle):
    b, c = _structured()
    marked, total = _check(b[:, None], c[None, :], _eps(oracle), "structured")
    print("structured: marked", marked, "of", total)
    assert 10 * marked >= total and 10 * (total - marked) >= total


def test_scene_pairs(oracle):
    b, c, disc = pr.trace(oracle, "ref")
    eps = _eps(oracle)
    for k in range(8):
        marked, total = _check(b[:, k].ravel(), c[:, k].ravel(), eps, ("scene", k))
        print("scene: sphere", k, "marked", marked, "of", total, "=", round(marked / total, 4))
        if k in (2, 3, 4, 5):   # the room lies inside every wall's sphere (c < 0): a wall is not behind a ray that is inside the room
            assert marked < total // 10
    assert b[:, 6:8].size == 8 * 2 * pr.W * pr.H * 4 * pr.S


def _med3(disc, b, c):
    v = np.stack([disc, b, -c])
    with np.errstate(all="ignore"):
        return np.where(np.isnan(v).any(axis=0), np.fmin(np.fmin(v[0], v[1]), v[2]), np.sort(v, axis=0)[1])


def test_joint_form_is_both_paths_marked():
    b, c = _structured()
    bb, cc = (x.ravel() for x in np.meshgrid(b[::3], c[::3], indexing="ij"))
    with np.errstate(all="ignore"):
        disc = bb * bb - cc
        m = _med3(disc, bb, cc)
        joint = ~(np.fmax(m[:, None], m[None, :]) >= -pr.GUARD)          # v_max_f32: the operand that is not NaN; NaN when both are
    each = pr.cannot_hit(bb, cc, disc)
    assert np.array_equal(joint, each[:, None] & each[None, :])
    assert joint.any() and not joint.all()
