"""An expectation tree for glass and mirror shading, written from the physics and not from the renderer's contract, for the tests only.

In a scene whose only scattering surfaces are glass (n = 1.5, Schlick) and mirror balls, inside walls that emit and have albedo 0, the
expected radiance of a ray is a finite sum: at a glass hit the estimator reflects with some probability P and weight Re / P or refracts
with weight Tr / (1 - P), whose expectation is Re * L(reflected) + Tr * L(refracted) whatever P is.  radiance() walks that binary tree
in float64 (Python floats and NumPy float64), 2^depth leaves at most, with no random numbers.  The sample mean of N copies of the same
ray through the renderer -- each copy a different path index -- must agree with it within its own standard error; a component on which
all copies agree (a wall seen directly, a mirror-only chain, a trapped ray) must agree to float32 rounding.

Nothing here comes from the NumPy restatements of the kernels or from the public header: the refractive index, Schlick's R0, Snell's law
and the quadratic are stated from first principles.  The sphere a ray stands on is handled by geometry (leaving outward: not tested;
leaving inward: the far root 2 (c - o).d), not by an epsilon.

Scenes: box8 (the 8-sphere form), box9 (box8 and a second glass ball: tiles, and the grid form) and box8_glow (the glass ball also emits).
box9 needed no extra spheres: the grid builder produces a grid the material renderer accepts for its 9 spheres as they are.
"""
import math

import numpy as np

SPEC, DIFF, REFR = 0, 1, 2      # the material codes of the materials= table
N_GLASS = 1.5
GLASS, MIRROR = 6, 7            # the two balls every ray kind is aimed at
RAY_KINDS = ("glass from outside", "mirror", "inside the glass", "trapped in the glass")

# (r, centre, emission, albedo, code)
_BOX8 = [
    (1e4, (1e4 + 100, 50, 50), (1, 0, 0), (0, 0, 0), DIFF),
    (1e4, (-1e4, 50, 50), (0, 1, 0), (0, 0, 0), DIFF),
    (1e4, (50, 1e4 + 100, 50), (0, 0, 1), (0, 0, 0), DIFF),
    (1e4, (50, -1e4, 50), (1, 1, 0), (0, 0, 0), DIFF),
    (1e4, (50, 50, 1e4 + 100), (0, 1, 1), (0, 0, 0), DIFF),
    (1e4, (50, 50, -1e4), (1, 0, 1), (0, 0, 0), DIFF),
    (20, (40, 50, 50), (0, 0, 0), (1, 1, 1), REFR),
    (12, (78, 40, 55), (0, 0, 0), (.9, .8, .7), SPEC),
]
_BOX9 = _BOX8 + [(8, (70, 75, 30), (0, 0, 0), (.95, .9, 1), REFR)]


class Scene:
    """table: the zero-padded float32 [10][ns] sphere table the renderer takes (r^2 rounded from float64); materials: int32 codes.
    The tree reads the float32 table back as float64, so both sides see the same spheres."""

    def __init__(self, name, rows):
        self.name, self.ns = name, len(rows)
        flat = np.array([[r * r, *c, *e, *a] for r, c, e, a, _ in rows], dtype=np.float64)
        self.table = np.zeros((self.ns * 10 + 127) // 128 * 128, dtype=np.float32)
        self.table[:10 * self.ns] = flat.T.astype(np.float32).ravel()
        self.materials = np.array([row[4] for row in rows], dtype=np.int32)
        planes = self.table[:10 * self.ns].reshape(10, self.ns).astype(np.float64)
        self.r2, self.centre, self.emission, self.albedo = planes[0], planes[1:4].T.copy(), planes[4:7].T.copy(), planes[7:10].T.copy()
        self.walls = [k for k in range(self.ns) if not self.albedo[k].any()]


def box8():
    return Scene("box8", _BOX8)


def box9():
    return Scene("box9", _BOX9)


GLOW = (0.125, 0.25, 0.0625)


def box8_glow():
    """box8 with a glass ball that also emits.  In box8 and box9 a ray that meets total internal reflection is trapped in a ball that
    emits nothing, so a renderer that ENDS such a path instead of reflecting it returns the same colour, 0.  Here the trapped ray
    gathers GLOW at each of its `depth` hits (exactly depth * GLOW: powers of two), and every chain through the glass gathers it too."""
    rows = list(_BOX8)
    r, c, _, a, code = rows[GLASS]
    rows[GLASS] = (r, c, GLOW, a, code)
    return Scene("box8_glow", rows)


# ---- the tree ---------------------------------------------------------------------------------------------------------------------
def nearest_hit(o, d, scene, on=-1):
    """-> (t, k) of the nearest sphere along the unit direction d from o, (inf, -1) for none; `on`: the sphere o lies on."""
    best, which = math.inf, -1
    for k in range(scene.ns):
        oc = scene.centre[k] - o
        b = float(oc @ d)
        if k == on:
            t = 2.0 * b if b > 0.0 else math.inf        # on the surface: the other end of the chord, or nothing when leaving outward
        else:
            disc = b * b - (float(oc @ oc) - scene.r2[k])
            if disc < 0.0:
                continue
            q = math.sqrt(disc)
            t = b - q if b - q > 0.0 else (b + q if b + q > 0.0 else math.inf)
        if t < best:
            best, which = t, k
    return best, which


def radiance(o, d, depth, scene, on=-1):
    """The expected colour (float64 [3]) of a path of `depth` hits that starts at o along d."""
    if depth == 0:
        return np.zeros(3)
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    d = d / math.sqrt(float(d @ d))
    t, k = nearest_hit(o, d, scene, on)
    if k < 0:
        return np.zeros(3)
    if not scene.albedo[k].any():                       # a wall: its emission, and nothing is gathered after it
        return scene.emission[k].copy()
    x = o + t * d
    n = x - scene.centre[k]
    n = n / math.sqrt(float(n @ n))
    outside = float(d @ n) < 0.0
    if not outside:
        n = -n                                          # the normal against the ray
    cos_i = -float(d @ n)
    refl = d + 2.0 * cos_i * n
    L_refl = radiance(x, refl, depth - 1, scene, k)
    if scene.materials[k] == SPEC:
        return scene.emission[k] + scene.albedo[k] * L_refl
    assert scene.materials[k] == REFR
    n1, n2 = (1.0, N_GLASS) if outside else (N_GLASS, 1.0)
    sin_i = math.sqrt(max(0.0, 1.0 - cos_i * cos_i))
    sin_t = n1 / n2 * sin_i
    if sin_t >= 1.0:                                    # total internal reflection
        return scene.emission[k] + scene.albedo[k] * L_refl
    cos_t = math.sqrt(1.0 - sin_t * sin_t)
    tangent = (d + cos_i * n) / sin_i if sin_i > 0.0 else np.zeros(3)
    refr = tangent * sin_t - n * cos_t
    r0 = ((n2 - n1) / (n2 + n1)) ** 2
    cos_air = cos_i if outside else cos_t               # Schlick's cosine is the one on the air side
    re = r0 + (1.0 - r0) * (1.0 - cos_air) ** 5
    L_refr = radiance(x, refr, depth - 1, scene, k)
    return scene.emission[k] + scene.albedo[k] * (re * L_refl + (1.0 - re) * L_refr)


# ---- the rays ---------------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v)


def _perpendicular(rng, a):
    return _unit(np.cross(a, rng.normal(size=3)))


def rays(seed=5):
    """16 rays, four of each of RAY_KINDS in that order, rounded to float32 -> float32 [6][16]."""
    rng = np.random.default_rng(seed)
    r, c, e, a, _ = _BOX8[GLASS]
    g, rg = np.array(c, dtype=np.float64), float(r)
    m, rm = np.array(_BOX8[MIRROR][1], dtype=np.float64), float(_BOX8[MIRROR][0])
    out = []
    for frac in (0.3, 0.6, 0.9, 0.99):                  # the impact parameter as a fraction of the radius
        o = np.clip(g + 45.0 * _unit(rng.normal(size=3)), 2.0, 98.0)
        w = g - o
        sin_a = frac * rg / np.linalg.norm(w)
        out.append((o, math.sqrt(1.0 - sin_a * sin_a) * _unit(w) + sin_a * _perpendicular(rng, w)))
    for _ in range(4):                                  # from beside the glass ball, on the mirror's side, at the mirror ball
        o = g + (rg + 3.0 + 3.0 * rng.random()) * _unit(_unit(m - g) + 0.6 * rng.normal(size=3))
        w = m - o
        out.append((o, _unit(w + 0.7 * rm * rng.random() * _perpendicular(rng, w))))
    for _ in range(4):                                  # within half a radius of the centre: sin(incidence) <= 0.5 at every hit
        out.append((g + 0.5 * rg * rng.random() ** (1.0 / 3.0) * _unit(rng.normal(size=3)), _unit(rng.normal(size=3))))
    for _ in range(4):                                  # sin(incidence) = 0.925 > 1 / 1.5 at every hit, for ever
        a = _unit(rng.normal(size=3))
        out.append((g + 0.925 * rg * a, _perpendicular(rng, a)))
    return np.array([np.concatenate(od) for od in out], dtype=np.float64).T.astype(np.float32)


def copies(rays16, n):
    """Ray r in columns [r n, (r + 1) n) -> float32 [6][16 n]: whole waves hold one ray and differ by their path index only."""
    return np.ascontiguousarray(np.repeat(np.asarray(rays16, dtype=np.float32), n, axis=1))


def tree(rays16, depth, scene):
    """-> float64 [3][16]: radiance() of each (float32-rounded) ray."""
    r = np.asarray(rays16, dtype=np.float32).astype(np.float64)
    return np.array([radiance(r[:3, i], r[3:, i], depth, scene) for i in range(r.shape[1])]).T


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
Z_CAP = 5.0            # |mean - tree| <= 5 standard errors: a cap for fixed seeds, not a fit
EXACT_TOL = 1e-6       # all copies equal: at most 7 float32 products of factors <= 1, each within 2^-24 relative


def compare(L, want, n):
    """L: float32 [3][16 n] from copies(); want: tree() -> dict(finite, zmax: largest |z| over the components whose copies differ,
    exact: largest |value - tree| over those whose copies are all equal, where: the (ray, channel) of each)."""
    L = np.asarray(L)
    out = dict(finite=bool(np.isfinite(L).all()), zmax=0.0, exact=0.0, z_at=None, exact_at=None, differing=0)
    for r in range(want.shape[1]):
        for ch in range(3):
            x = L[ch, r * n:(r + 1) * n].astype(np.float64)
            if not np.isfinite(x).all():
                continue
            if x.min() == x.max():
                err = abs(x[0] - want[ch, r])
                if err > out["exact"]:
                    out["exact"], out["exact_at"] = err, (r, ch)
            else:
                out["differing"] += 1
                z = abs(x.mean() - want[ch, r]) / (x.std(ddof=1) / math.sqrt(n))
                if z > out["zmax"]:
                    out["zmax"], out["z_at"] = z, (r, ch)
    return out


def agrees(c):
    return c["finite"] and c["zmax"] <= Z_CAP and c["exact"] <= EXACT_TOL
