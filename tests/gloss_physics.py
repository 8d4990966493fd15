"""A float64 expectation for the rough-metal material, written from the physics and not from the renderer's contract, for the tests only.

A ray that hits a rough conductor at x with view direction v (towards the eye) returns

    L = emission + albedo * integral over the hemisphere of  D(h) G1(v) G1(l) / (4 (n.v) (n.l)) * (n.l) * Le(x, l)  dl

with the GGX (Trowbridge-Reitz) distribution D(h) = a^2 / (pi ((n.h)^2 (a^2 - 1) + 1)^2) of the half vector h = (v + l) / |v + l|, the
separable Smith term G1(w) = 2 (n.w) / ((n.w) + sqrt(a^2 + (1 - a^2) (n.w)^2)), a reflectance that is the albedo at every angle (the
material has no Fresnel term), and Le(x, l) the emission of the nearest sphere along l.  In the scenes below the rough ball is the only
surface that scatters -- everything else has albedo 0 -- so the integral is one level deep whatever the depth (>= 2), and direct light
sampling, a light table and roulette leave it unchanged.  expectation() evaluates it by a midpoint rule over (cos theta_l, phi_l), the
LIGHT direction: not the parametrisation the renderer samples in (visible normals), and with no random numbers.

Nothing here comes from the NumPy restatements of the kernels or from the public header.  Geometry is physics_ref's: the nearest hit
along a direction is physics_ref.nearest_hit's rule (the sphere stood on is handled by geometry, not by an epsilon), evaluated for whole
arrays of directions at once (emitted(); tests/test_gloss_cpu.py checks it against nearest_hit itself).

The stored expectations: tests/golden/gloss_expectations.json, written by tests/golden/make_gloss_expectations.py at resolution N_QUAD,
with the rule's own error next to each -- the difference to resolution 2 N_QUAD."""
import json
import math
import os

import numpy as np

import physics_ref as ph

GLOSS_CODE = 3
BALL = 6                         # the rough ball every ray is aimed at
DEPTH = 4
COPIES = 16384
FRACTIONS = (0.1, 0.25, 0.4, 0.55, 0.7, 0.8, 0.9, 0.95)      # impact parameters, as fractions of the radius
N_QUAD = 1024                    # cos theta cells; 2 N_QUAD phi cells
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gloss_expectations.json")


def gloss_word(alpha):
    q = min(65535, max(1, int(round(alpha * 65536.0))))
    return GLOSS_CODE | (q << 8)


def _rows(alpha, second):
    rows = list(ph._BOX8[:6])                                                        # six emitting walls of albedo 0
    rows.append((20, (40, 50, 50), ph.GLOW, (.9, .8, .7), gloss_word(alpha)))        # the rough ball (it also glows a little)
    rows.append((8, (78, 40, 55), (2, 1.5, .5), (0, 0, 0), ph.DIFF))                 # a small lamp
    if second:
        rows.append((8, (70, 75, 30), (.5, 2, 1), (0, 0, 0), ph.DIFF))
    return rows


def gloss8():
    return ph.Scene("gloss8", _rows(0.5, False))


def gloss9():
    """gloss8 with a narrower lobe and a second lamp: nine spheres, for the tile and grid forms."""
    return ph.Scene("gloss9", _rows(0.2, True))


def alpha_of(scene, k=BALL):
    """The roughness the material word of sphere k carries: q * 2^-16."""
    return ((int(scene.materials[k]) >> 8) & 0xFFFF) / 65536.0


def rays(seed=7):
    """Eight rays at the rough ball from outside, one per impact parameter of FRACTIONS, rounded to float32 -> float32 [6][8]."""
    rng = np.random.default_rng(seed)
    g, rg = np.array((40.0, 50.0, 50.0)), 20.0
    out = []
    for frac in FRACTIONS:
        o = np.clip(g + 45.0 * ph._unit(rng.normal(size=3)), 2.0, 98.0)
        w = g - o
        sin_a = frac * rg / np.linalg.norm(w)
        out.append(np.concatenate([o, math.sqrt(1.0 - sin_a * sin_a) * ph._unit(w) + sin_a * ph._perpendicular(rng, w)]))
    return np.array(out, dtype=np.float64).T.astype(np.float32)


def copies(rays8, n=COPIES):
    return ph.copies(rays8, n)


def emitted(x, dirs, scene, on):
    """Le(x, l) for unit directions dirs [m][3] from the point x on sphere `on` -> float64 [m][3]: physics_ref.nearest_hit's rule."""
    m = dirs.shape[0]
    best = np.full(m, math.inf)
    which = np.full(m, -1)
    for k in range(scene.ns):
        oc = scene.centre[k] - x
        b = dirs @ oc
        if k == on:
            t = np.where(b > 0.0, 2.0 * b, math.inf)
        else:
            disc = b * b - (float(oc @ oc) - scene.r2[k])
            q = np.sqrt(np.where(disc >= 0.0, disc, 0.0))
            t = np.where(disc < 0.0, math.inf, np.where(b - q > 0.0, b - q, np.where(b + q > 0.0, b + q, math.inf)))
        closer = t < best
        best, which = np.where(closer, t, best), np.where(closer, k, which)
    return np.where((which >= 0)[:, None], scene.emission[np.maximum(which, 0)], 0.0)


def _g1(c, a2):
    return 2.0 * c / (c + np.sqrt(a2 + (1.0 - a2) * c * c))


def radiance(o, d, scene, n=N_QUAD, rows=32):
    """The expected colour (float64 [3]) of a path of >= 2 hits from o along d, which must hit the rough ball first."""
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    d = d / math.sqrt(float(d @ d))
    t, k = ph.nearest_hit(o, d, scene)
    assert k == BALL and scene.albedo[k].any()
    a = alpha_of(scene, k)
    a2 = a * a
    x = o + t * d
    nrm = ph._unit(x - scene.centre[k])
    v = -d
    nv = float(v @ nrm)
    assert nv > 0.0
    e1 = ph._unit(np.cross(nrm, np.eye(3)[int(np.argmin(np.abs(nrm)))]))
    e2 = np.cross(nrm, e1)
    nphi = 2 * n
    phi = (np.arange(nphi) + 0.5) * (2.0 * math.pi / nphi)
    cphi, sphi = np.cos(phi), np.sin(phi)
    g1v = float(_g1(nv, a2))
    total = np.zeros(3)
    for lo in range(0, n, rows):
        mu = (np.arange(lo, min(n, lo + rows)) + 0.5) / n                            # cos theta_l = n.l
        st = np.sqrt(1.0 - mu * mu)
        l = ((st[:, None] * cphi[None, :])[..., None] * e1 + (st[:, None] * sphi[None, :])[..., None] * e2 + mu[:, None, None] * nrm).reshape(-1, 3)
        nl = np.repeat(mu, nphi)
        h = l + v
        nh = (h @ nrm) / np.sqrt(np.einsum("ij,ij->i", h, h))
        dist = a2 / (math.pi * (nh * nh * (a2 - 1.0) + 1.0) ** 2)
        f = dist * g1v * _g1(nl, a2) / (4.0 * nv * nl) * nl                          # the BRDF times (n.l)
        total += (f[:, None] * emitted(x, l, scene, k)).sum(axis=0)
    return scene.emission[k] + scene.albedo[k] * total * ((1.0 / n) * (2.0 * math.pi / nphi))


def expectation(rays8, scene, n=N_QUAD):
    """-> float64 [3][8]: radiance() of each (float32-rounded) ray."""
    r = np.asarray(rays8, dtype=np.float32).astype(np.float64)
    return np.array([radiance(r[:3, i], r[3:, i], scene, n) for i in range(r.shape[1])]).T


def load_fixture():
    """-> {scene name: (expect float64 [3][8], quad_err float64 [3][8])} and the fixture's own record of how it was made."""
    with open(FIXTURE) as f:
        doc = json.load(f)
    return {name: (np.array(s["expect"]), np.array(s["quad_err"])) for name, s in doc["scenes"].items()}, doc


def compare(L, want, n=COPIES):
    """physics_ref's rule, on 8 rays: |mean - want| <= 5 standard errors per ray and channel, 1e-6 where all copies agree; also the
    standard error of every component (0 where all copies agree) -> (physics_ref.compare's dict, se float64 [3][8])."""
    L = np.asarray(L)
    se = np.array([[L[ch, r * n:(r + 1) * n].astype(np.float64).std(ddof=1) / math.sqrt(n) for r in range(want.shape[1])] for ch in range(3)])
    return ph.compare(L, want, n), se
