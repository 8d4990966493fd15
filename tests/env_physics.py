"""The environment's physics checks (include/render_mi355x.h "environment"): scenes, hand-made rays and their expectations, written in
float64 from geometry alone.  This module imports no restatement and none of the library: tests/test_environment_cpu.py runs
tests/materials_ref.py on these rays, tests/test_gpu_environment.py the kernels, and both meet the same numbers.

Every case is a handful of rays in buffer mode, COPIES copies of each (each copy another path index, so another random sequence),
seed 1.  The rule is the project's: |mean - expectation| <= Z_CAP * sigma / sqrt(COPIES) per ray and channel, sigma the copies' own
standard deviation, or |value - expectation| <= EXACT_TOL where all copies agree.

The real spheres of a case are followed by parked ones -- radius 0.5 far away below the scene, albedo 0 -- up to the sphere count a
scene form needs (8: the SGPR form; 9: tiles and the grid); the CPU test shows with the restatement that no path meets them."""
import numpy as np

COPIES = 16384
SEED = 1
Z_CAP, EXACT_TOL = 5.0, 1e-6
DIFF, SPEC, REFR = 1, 0, 2
SAMPLE_SUN = 1
OMC = 2.0 ** -4                      # the sun's cone: 1 - cos(half angle); half angle 20.36 degrees
ALB = 0.5


def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def table_of(rows, ns):
    """rows of (radius, x, y, z, emission rgb, albedo rgb), then parked spheres up to ns -> the zero-padded [10][ns] float32 table."""
    rows = [list(map(float, r)) for r in rows]
    for i in range(ns - len(rows)):
        rows.append([0.5, 1.0e4 + 100.0 * i, -1.0e4, 1.0e4, 0, 0, 0, 0, 0, 0])
    a = np.array(rows, dtype=np.float64)
    a[:, 0] = a[:, 0] ** 2
    out = np.zeros((ns * 10 + 127) // 128 * 128, dtype=np.float32)
    out[:10 * ns] = a.T.astype(np.float32).ravel()
    return out


def hit_unit_sphere(o, d):
    """The first point of the ray (o, d), d unit, on the unit sphere at the origin -> (point = normal), or None."""
    b = -np.dot(o, d)
    disc = b * b - (np.dot(o, o) - 1.0)
    if disc < 0:
        return None
    t = b - np.sqrt(disc)
    return None if t <= 0 else o + t * d


class Case:
    """One scene, environment and set of rays with the expectation of every ray.
    rows: the real spheres; mats: their codes; env: dict(horizon, zenith, sun_dir, sun_radiance, sun_omc); rays: float64 [n][6];
    want: float64 [n][3], or None where the case compares two launches instead; exact: every copy of a ray gives one value."""

    def __init__(self, name, rows, mats, env, rays, want, depth, exact, light=-1, lights=None):
        self.name, self.rows, self.mats, self.env, self.depth, self.exact = name, rows, list(mats), env, depth, exact
        self.rays64 = np.asarray(rays, dtype=np.float64)
        self.want = None if want is None else np.asarray(want, dtype=np.float64)
        self.light, self.lights = light, lights

    @property
    def nrays(self):
        return self.rays64.shape[0]

    def table(self, ns):
        return table_of(self.rows, ns)

    def materials(self, ns):
        return np.array(self.mats + [DIFF] * (ns - len(self.mats)), dtype=np.int32)

    def rays(self):
        """float32 [6][nrays * COPIES]: ray r's copies are paths [r * COPIES, (r + 1) * COPIES)."""
        return np.repeat(self.rays64.T, COPIES, axis=1).astype(np.float32)

    def paths(self):
        return np.arange(self.nrays * COPIES, dtype=np.uint64)

    def frame_shape(self):
        """(width, height, samples) of a frame with exactly nrays * COPIES paths, for the buffer entry's parameter record."""
        n = self.nrays * COPIES
        assert n % (4 * 64 * 64) == 0
        return 64, 64, n // (4 * 64 * 64)


def summarise(L):
    """L float32 [3][nrays * COPIES] -> (mean [nrays][3], sigma [nrays][3], same [nrays][3]: every copy gave one value), float64."""
    v = np.asarray(L, dtype=np.float64).reshape(3, -1, COPIES)
    return v.mean(axis=2).T, v.std(axis=2).T, (v.max(axis=2) == v.min(axis=2)).T


def compare(L, want, exact=False):
    """-> dict(zmax: the largest |mean - want| / (sigma / sqrt(COPIES)) over the components whose copies differ, exact: the largest
    |value - want| over those whose copies agree, differing: how many differ, finite).  exact=True: every component must agree."""
    mean, sigma, same = summarise(L)
    err = np.abs(mean - want)
    z = np.where(same, 0.0, err / np.where(same, 1.0, sigma / np.sqrt(COPIES)))
    return dict(zmax=float(z.max()), exact=float(np.where(same, err, 0.0).max()), differing=int((~same).sum()),
                finite=bool(np.isfinite(L).all()), all_same=bool(same.all()))


def passes(c, exact):
    return c["finite"] and c["zmax"] <= Z_CAP and c["exact"] <= EXACT_TOL and (c["all_same"] if exact else c["differing"] > 0)


# ---- rays at the unit sphere ----------------------------------------------------------------------------------------------------------
def _aimed(targets, eye_shift):
    """Rays from 4 * unit(n + eye_shift) towards the points n (unit) of the unit sphere -> ([n][6], the float64 hit points = normals)."""
    rays, normals = [], []
    for n in targets:
        n = unit(n)
        o = 4.0 * unit(n + np.asarray(eye_shift, dtype=np.float64))
        d = unit(n - o)
        p = hit_unit_sphere(o, d)
        assert p is not None and np.dot(p, n) > 0.9
        rays.append(np.concatenate([o, d]))
        normals.append(p)
    return np.array(rays), np.array(normals)


_TARGETS = [(0.0, 1.0, 0.0), (0.5, 0.8, 0.2), (-0.3, 0.9, -0.4), (0.2, 0.7, 0.6)]
_MISSES = [np.concatenate([[3.0, 3.0, 3.0], unit([0.2, 1.0, 0.1])]), np.concatenate([[0.0, -4.0, 0.0], unit([1.0, -0.2, 0.3])])]
_BALL = [1.0, 0, 0, 0, 0, 0, 0, ALB, ALB, ALB]
_NO_SUN = dict(sun_dir=(0, 1, 0), sun_radiance=(0, 0, 0), sun_omc=0.0)


def uniform_sky(depth):
    """Radiance 1 from everywhere, one DIFF sphere of albedo 0.5: a convex sphere alone sees only sky after one bounce -> exactly 0.5 at
    any depth >= 2, exactly 0 at depth 1 (the path has no second segment); a ray that misses is exactly 1."""
    rays, _ = _aimed(_TARGETS, (0.2, 0.1, -0.1))
    rays = np.concatenate([rays, np.array(_MISSES)])
    for r in _MISSES:
        assert hit_unit_sphere(r[:3], r[3:]) is None
    hit = ALB if depth >= 2 else 0.0
    want = [[hit] * 3] * len(_TARGETS) + [[1.0] * 3] * len(_MISSES)
    return Case("uniform_sky_d%d" % depth, [_BALL], [DIFF], dict(horizon=(1, 1, 1), zenith=(1, 1, 1), **_NO_SUN), rays, want, depth, True)


def gradient_sky():
    """A sky from `horizon` to `zenith` seen from a point with unit normal n: the cosine-weighted mean of t = 0.5 + 0.5 d.y over the
    hemisphere about n is 0.5 + n.y / 3 (the mean of d is 2/3 n), so E = albedo * (horizon + (zenith - horizon) * (0.5 + n.y / 3))."""
    hz, zn = np.array([0.25, 0.5, 0.75]), np.array([2.0, 1.0, 0.5])
    rays, normals = _aimed(_TARGETS + [(0.9, -0.3, 0.1), (0.0, -1.0, 0.0)], (0.1, -0.2, 0.15))
    want = [ALB * (hz + (zn - hz) * (0.5 + n[1] / 3.0)) for n in normals]
    return Case("gradient_sky", [_BALL], [DIFF], dict(horizon=tuple(hz), zenith=tuple(zn), **_NO_SUN), rays, want, 2, False)


SUN_W = unit([0.3, 1.0, 0.2])
SUN_RAD = np.array([4.0, 2.0, 8.0])


def sun_only(sample, depth=2):
    """A black sky and a sun of radiance R in the cone of 1 - cos = omc about w, wholly above the horizon of every hit point
    (n.w > sin(half angle) = 0.348): E = albedo * R * integral of cos / pi over the cone = albedo * R * (n.w) * omc * (2 - omc).
    The same with APT_ENV_SAMPLE_SUN on and off: a sun counted twice, or never, shows in one of the two."""
    rays, normals = _aimed(_TARGETS, (0.15, 0.1, -0.2))
    dots = normals @ SUN_W
    assert (dots > 0.5).all()
    want = [ALB * SUN_RAD * nw * OMC * (2.0 - OMC) for nw in dots]
    env = dict(horizon=(0, 0, 0), zenith=(0, 0, 0), sun_dir=tuple(SUN_W), sun_radiance=tuple(SUN_RAD), sun_omc=OMC, flags=SAMPLE_SUN if sample else 0)
    return Case("sun_%s_d%d" % ("sampled" if sample else "plain", depth), [_BALL], [DIFF], env, rays, want, depth, False)


def occluder():
    """The sun of sun_only behind a black sphere that covers its whole cone from every hit point (radius 60 at 100 w: it subtends more
    than 35 degrees from anywhere on the unit sphere, the cone 20.4): with the sun sampled every shadow segment is blocked and no
    bounce ray can reach the cone -> exactly 0."""
    rays, normals = _aimed(_TARGETS, (0.15, 0.1, -0.2))
    c = 100.0 * SUN_W
    for n in normals:                                        # the cone about w from n lies inside the occluder's disc
        to = c - n
        half = np.arcsin(60.0 / np.linalg.norm(to))
        assert half - np.arccos(np.dot(unit(to), SUN_W)) > np.arccos(1.0 - OMC) + 0.05
    env = dict(horizon=(0, 0, 0), zenith=(0, 0, 0), sun_dir=tuple(SUN_W), sun_radiance=tuple(SUN_RAD), sun_omc=OMC, flags=SAMPLE_SUN)
    rows = [_BALL, [60.0, *c, 0, 0, 0, 0, 0, 0]]
    return Case("occluder", rows, [DIFF, DIFF], env, rays, [[0.0] * 3] * len(rays), 3, True)


def mirror_ball(sample):
    """A mirror ball of albedo 0.75 reflects the ray (1, 0, 0) at the point (-s, s, 0), s = sqrt(1/2), straight up into the middle of a
    sun about +y; the second ray is turned to (0, 1, 0) rotated by 10 degrees, still inside the 20.4 degree cone.  SPEC never samples,
    so the miss adds the sun in full, with and without APT_ENV_SAMPLE_SUN: exactly albedo * (sky + sun) = 0.75 * (0.25 + 4)."""
    s = np.sqrt(0.5)
    rays = [np.concatenate([[-5.0 - s, s, 0.0], [1.0, 0.0, 0.0]])]
    a = np.radians(10.0)
    out = np.array([np.sin(a), np.cos(a), 0.0])              # wanted outgoing direction
    n = unit(out - np.array([1.0, 0.0, 0.0]))                # the normal that turns (1, 0, 0) into it
    rays.append(np.concatenate([n - 5.0 * np.array([1.0, 0.0, 0.0]), [1.0, 0.0, 0.0]]))
    env = dict(horizon=(0.25,) * 3, zenith=(0.25,) * 3, sun_dir=(0, 1, 0), sun_radiance=(4, 4, 4), sun_omc=OMC, flags=SAMPLE_SUN if sample else 0)
    ball = [1.0, 0, 0, 0, 0, 0, 0, 0.75, 0.75, 0.75]
    return Case("mirror_%s" % ("sampled" if sample else "plain"), [ball], [SPEC], env, rays, [[0.75 * 4.25] * 3] * 2, 2, True)


def glass_ball(sample):
    """A glass ball (radius 1.5 at 4 w) between three points of the DIFF sphere near its pole towards the sun and the sun, covering the whole cone from each of them:
    the sun reaches the points only through the glass.  With the sun sampled every shadow segment ends on the glass, and the light
    arrives on bounce rays that enter the ball, leave it and miss -- which they may count only because `sampled_sun` is cleared at
    the glass hits in between.  No closed form: the case is rendered with APT_ENV_SAMPLE_SUN on and off and the two must agree
    within the two standard errors (want is None); the plain one is the path tracer the other cases tie to closed forms."""
    rays, normals = _aimed([tuple(SUN_W), tuple(SUN_W + np.array([0.12, 0.0, 0.0])), tuple(SUN_W + np.array([0.0, 0.0, -0.12]))], (0.05, 0.05, -0.05))
    c = 4.0 * SUN_W
    for n in normals:
        to = c - n
        assert np.arcsin(1.5 / np.linalg.norm(to)) - np.arccos(np.dot(unit(to), SUN_W)) > np.arccos(1.0 - OMC) + 0.02
    env = dict(horizon=(0, 0, 0), zenith=(0, 0, 0), sun_dir=tuple(SUN_W), sun_radiance=tuple(SUN_RAD), sun_omc=OMC, flags=SAMPLE_SUN if sample else 0)
    rows = [_BALL, [1.5, *c, 0, 0, 0, 1, 1, 1]]
    return Case("glass_%s" % ("sampled" if sample else "plain"), rows, [DIFF, REFR], env, rays, None, 6, False)


def sun_and_lamp(sample=True):
    """The sun of sun_only and a sphere lamp (radius 0.5 at 8 u, emission e, albedo 0) that is wholly above the horizon of every hit
    point and clear of the sun's cone: E = albedo * (R * (n.w) * omc * (2 - omc) + e * (r / dist)^2 * cos), the sphere light's closed
    form.  Rendered with APT_FLAG_NEE (light 1) and with a light table listing the lamp: each DIFF bounce adds the lamp's sample,
    then the sun's."""
    rays, normals = _aimed(_TARGETS, (0.15, 0.1, -0.2))
    u = unit([-0.4, 0.9, -0.1])
    c, r, e = 8.0 * u, 0.5, np.array([64.0, 128.0, 32.0])
    assert np.arccos(np.dot(u, SUN_W)) > np.arccos(1.0 - OMC) + 0.3          # the lamp does not shade the cone
    want = []
    for n in normals:
        to = c - n
        dist = np.linalg.norm(to)
        cos = np.dot(to, n) / dist
        assert cos > r / dist + 0.1                                         # wholly above the horizon
        want.append(ALB * (SUN_RAD * np.dot(n, SUN_W) * OMC * (2.0 - OMC) + e * (r / dist) ** 2 * cos))
    env = dict(horizon=(0, 0, 0), zenith=(0, 0, 0), sun_dir=tuple(SUN_W), sun_radiance=tuple(SUN_RAD), sun_omc=OMC, flags=SAMPLE_SUN if sample else 0)
    rows = [_BALL, [r, *c, *e, 0, 0, 0]]
    return Case("sun_and_lamp", rows, [DIFF, DIFF], env, rays, want, 2, False, light=1, lights=[1])
