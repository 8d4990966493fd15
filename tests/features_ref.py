"""NumPy restatement of the first-hit feature planes (include/render_mi355x.h "features": coverage, depth, normal and albedo of the first
surface under each pixel), for the tests only.

The rays are camera_ref.rays -- the material frame launches' own, tent filter and thin lens included --, the first hit is
materials_ref._intersect with no skip sphere, and the normal is the bounce's nl, one separately rounded float32 operation per step in
the header's order (f32() fails on a float64 intermediate).  A pixel's value is the float64 sum of its 4 * samples per-path values in
ascending path order -- a Python loop over the paths, no cumsum and no pairwise np.sum --, divided by float64(4 * samples) and rounded once
to float32.  reverse=True sums in descending path order instead: what the tests hold the ascending order against."""
import numpy as np

import camera_ref as cr
import materials_ref as mr
from materials_ref import F, f32

D = np.float64
PLANES = 8
COVERAGE, DEPTH, NORMAL, ALBEDO = 0, 1, 2, 5


def path_values(rays, spheres, ns, eps):
    """The eight per-path values of the rays float32 [6][n] in the scene `spheres` (the padded [10][Ns] table) -> float32 [8][n]."""
    rays = np.asarray(rays, dtype=F).reshape(6, -1)
    n = rays.shape[1]
    sph = np.asarray(spheres, dtype=F).ravel()[:10 * ns].reshape(10, ns)
    geo = (sph[1], sph[2], sph[3], sph[0])
    out = np.zeros((PLANES, n), dtype=F)
    step = max(1, (1 << 20) // ns) if ns > 64 else 1 << 16               # the [paths][spheres] arrays of one chunk stay at ~4 MB
    with np.errstate(all="ignore"):
        for lo in range(0, n, step):
            o = [rays[k, lo:lo + step] for k in range(3)]
            d = [rays[k, lo:lo + step] for k in range(3, 6)]
            tmin, k = mr._intersect(o, d, geo, F(eps), np.full(o[0].size, -1, dtype=np.int64))
            hit = k >= 0
            g = np.where(hit, k, 0)
            h = [o[i] + d[i] * tmin for i in range(3)]
            nr = [h[i] - sph[1 + i][g] for i in range(3)]
            ln = np.sqrt(mr.dot(*nr, *nr))
            nu = [nr[i] / ln for i in range(3)]
            into = mr.dot(*d, *nu) < F(0)
            nl = [np.where(into, nu[i], -nu[i]) for i in range(3)]
            vals = [np.ones(o[0].size, dtype=F), tmin] + nl + [sph[7 + i][g] for i in range(3)]
            f32(tmin, ln, *h, *nr, *nu, *vals)
            for c in range(PLANES):
                out[c, lo:lo + step] = np.where(hit, vals[c], F(0))
    return out


def pixel_means(values, samples, reverse=False):
    """float32 [8][pixels * 4 * samples] per-path values -> float32 [8][pixels]: the sequential float64 sum, / float64(4 * S), one rounding."""
    n = 4 * samples
    v = f32(np.asarray(values)).astype(D).reshape(PLANES, -1, n)
    acc = np.zeros(v.shape[:2], dtype=D)
    for k in (range(n - 1, -1, -1) if reverse else range(n)):
        acc = acc + v[:, :, k]
    assert acc.dtype == D
    return (acc / D(n)).astype(F)


def planes(rec, w, h, s, seed, spheres, ns, eps, pixel_begin=0, pixel_count=None, reverse=False):
    """apt_render_frame_features for the camera record `rec` (camera_ref: default_record(w, h) when no camera is set) -> float32
    [8][pixel_count], band-relative and x-major."""
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    rays = cr.rays(rec, w, h, s, seed=seed, path_begin=pixel_begin * 4 * s, path_count=pixel_count * 4 * s)
    return pixel_means(path_values(rays, spheres, ns, eps), s, reverse)
