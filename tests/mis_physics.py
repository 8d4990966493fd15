"""A float64 expectation for the direct light of one small lamp on a rough-metal ball, written from the physics and not from the
renderer's contract, for the tests of APT_FLAG_MIS only (in the manner of tests/gloss_physics.py).

The scene is two spheres in empty space: a rough conductor (GGX roughness a, separable Smith term, reflectance = albedo, no Fresnel
term) and a lamp of albedo 0.  A ray that hits the ball at x with view direction v (towards the eye) returns, at depth 2,

    L = albedo * integral over the lamp's cone of  D(h) G1(v) G1(l) / (4 (n.v) (n.l)) * (n.l) * V(x, l) * Le  dl

with D(h) = a^2 / (pi ((n.h)^2 (a^2 - 1) + 1)^2), h = (v + l) / |v + l|, G1(w) = 2 (n.w) / ((n.w) + sqrt(a^2 + (1 - a^2) (n.w)^2)), and
V = 1 where l leaves the ball's surface (n.l > 0): nothing else is in the scene, and a convex ball cannot be met again going outward.
quadrature() integrates over the cone of directions that meet the lamp -- (cos theta, phi) around the direction to its centre, cos
theta from cos_max to 1 -- by a midpoint rule, with no random numbers; its own error is taken as the difference between the rule at n
and at 2 n.  How the renderer samples (visible normals, the cone, both) does not enter, so the flagless estimator and the one with the
flag must both have this as their mean.

Nothing here comes from the NumPy restatements of the kernels or from the public header."""
import math

import numpy as np

GLOSS_CODE, DIFF_CODE = 3, 1
BALL, LAMP = 0, 1
BALL_R, BALL_C, BALL_ALBEDO = 20.0, (50.0, 40.0, 80.0), (0.9, 0.8, 0.7)
LAMP_E = (400.0, 300.0, 200.0)
N_QUAD = 512


def gloss_word(q):
    return GLOSS_CODE | (int(q) << 8)


def scene(q, lamp_r=2.0, lamp_c=(50.0, 85.0, 110.0)):
    """-> (the zero-padded float32 [10][2] table, the material words): the ball of roughness q * 2^-16 and the lamp."""
    rows = np.array([[BALL_R ** 2, *BALL_C, 0, 0, 0, *BALL_ALBEDO], [lamp_r ** 2, *lamp_c, *LAMP_E, 0, 0, 0]], dtype=np.float64)
    table = np.zeros(128, dtype=np.float32)
    table[:20] = rows.T.astype(np.float32).ravel()
    return table, np.array([gloss_word(q), DIFF_CODE], dtype=np.int32)


def mirror_ray(table, eye=(50.0, 52.0, 295.6), iterations=60):
    """A ray from `eye` to the point of the ball where the mirror direction points at the lamp's centre (found by fixed-point iteration
    on the half vector), rounded to float32 -> float32 [6]."""
    p = table[:20].reshape(10, 2).astype(np.float64)
    c, r, lc, e = p[1:4, BALL], math.sqrt(p[0, BALL]), p[1:4, LAMP], np.array(eye)
    n = (e - c) / np.linalg.norm(e - c)
    for _ in range(iterations):
        x = c + r * n
        a, b = (e - x) / np.linalg.norm(e - x), (lc - x) / np.linalg.norm(lc - x)
        n = (a + b) / np.linalg.norm(a + b)
    x = c + r * n
    d = (x - e) / np.linalg.norm(x - e)
    return np.concatenate([e, d]).astype(np.float32)


def _g1(c, a2):
    return 2.0 * c / (c + np.sqrt(a2 + (1.0 - a2) * c * c))


def quadrature(ray, table, q, n=N_QUAD):
    """The expected colour (float64 [3]) of a depth-2 path along the (float32) ray, which must hit the ball."""
    p = table[:20].reshape(10, 2).astype(np.float64)
    ray = np.asarray(ray, dtype=np.float32).astype(np.float64)
    o, d = ray[:3], ray[3:] / np.linalg.norm(ray[3:])
    c, r2 = p[1:4, BALL], p[0, BALL]
    oc = c - o
    b = float(oc @ d)
    disc = b * b - (float(oc @ oc) - r2)
    assert disc > 0.0 and b - math.sqrt(disc) > 0.0
    x = o + (b - math.sqrt(disc)) * d
    nrm = (x - c) / np.linalg.norm(x - c)
    v = -d
    nv = float(v @ nrm)
    assert nv > 0.0
    a = q / 65536.0
    a2 = a * a
    w = p[1:4, LAMP] - x
    dist2 = float(w @ w)
    assert dist2 > p[0, LAMP]
    w = w / math.sqrt(dist2)
    cos_max = math.sqrt(1.0 - p[0, LAMP] / dist2)
    e1 = np.cross(w, np.eye(3)[int(np.argmin(np.abs(w)))])
    e1 = e1 / np.linalg.norm(e1)
    e2 = np.cross(w, e1)
    nphi = 2 * n
    phi = (np.arange(nphi) + 0.5) * (2.0 * math.pi / nphi)
    mu = cos_max + (np.arange(n) + 0.5) * ((1.0 - cos_max) / n)
    st = np.sqrt(1.0 - mu * mu)
    l = ((st[:, None] * np.cos(phi)[None, :])[..., None] * e1 + (st[:, None] * np.sin(phi)[None, :])[..., None] * e2
         + mu[:, None, None] * w).reshape(-1, 3)
    nl = l @ nrm
    h = l + v
    nh = (h @ nrm) / np.sqrt(np.einsum("ij,ij->i", h, h))
    dist = a2 / (math.pi * (nh * nh * (a2 - 1.0) + 1.0) ** 2)
    ok = nl > 0.0
    cl = np.where(ok, nl, 1.0)
    f = np.where(ok, dist * _g1(nv, a2) * _g1(cl, a2) / (4.0 * nv), 0.0)                 # BRDF * (n.l) * V
    total = f.sum() * ((1.0 - cos_max) / n) * (2.0 * math.pi / nphi)
    return p[7:10, BALL] * p[4:7, LAMP] * total


def expectation(ray, table, q, n=N_QUAD):
    """-> (want float64 [3], quad_err float64 [3]): the rule at 2 n, and its difference to the rule at n."""
    fine = quadrature(ray, table, q, 2 * n)
    return fine, np.abs(fine - quadrature(ray, table, q, n))
