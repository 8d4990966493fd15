"""NumPy restatement of the per-sphere material renderer (include/render_mi355x.h "per-sphere materials"), for the tests only.

float32 arrays vectorised over paths, every constant an np.float32 (NumPy >= 2 promotes by NEP 50: float32 op float32 stays float32),
one separately rounded operation per step in the header's order; NumPy's float32 sqrt and division are IEEE.  The polynomial and
glass constants are read from the header itself.  Camera rays come from the oracle's counter generator and colours are decoded by the
oracle's decode_color, both existing and exact.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = np.uint64
MISS = F(1e20)
SPEC, DIFF, REFR = 0, 1, 2


def _header_constants():
    text = open(os.path.join(ROOT, "include", "render_mi355x.h")).read()
    return {m.group(1): F(float.fromhex(m.group(2))) for m in re.finditer(r"#define (APT_MAT_\w+)\s+(-?0x[0-9a-fA-Fp.+-]+)f", text)}


C = _header_constants()
S_COEF = [C[f"APT_MAT_S{k}"] for k in (1, 3, 5, 7, 9, 11)]
C_COEF = [F(1.0)] + [C[f"APT_MAT_C{k}"] for k in (2, 4, 6, 8, 10, 12)]


def f32(*arrays):
    """Every intermediate of the restatement is float32: fails loudly on a float64 one."""
    for a in arrays:
        assert np.asarray(a).dtype == np.float32, np.asarray(a).dtype
    return arrays[0] if len(arrays) == 1 else arrays


def splitmix64(x):
    x = np.asarray(x, dtype=U)
    with np.errstate(over="ignore"):
        x = x + U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
    return x ^ (x >> U(31))


def mat_key(seed, path):
    return splitmix64(U(seed) ^ splitmix64(path) ^ U(0x6A09E667F3BCC909))


def rr_key(seed, path):
    return splitmix64(U(seed) ^ splitmix64(path))


def uniforms(mkey, d):
    with np.errstate(over="ignore"):
        h = splitmix64(mkey + U(0x9E3779B97F4A7C15) * U(d + 1))
    u1 = (h >> U(40)).astype(F) * F(2.0 ** -24)
    u2 = ((h >> U(16)) & U(0xFFFFFF)).astype(F) * F(2.0 ** -24)
    return f32(u1, u2)


def sincos(u1):
    """(sin, cos) of 2*pi*u1: quadrant / fraction of u1 * 4, the header's polynomial pair, swap / negate."""
    x = u1 * F(4)
    q = x.astype(np.int32)
    fr = x - q.astype(F)
    z = fr * fr
    p = S_COEF[5]
    for k in (4, 3, 2, 1, 0):
        p = S_COEF[k] + z * p
    s = fr * p
    c = C_COEF[6]
    for k in (5, 4, 3, 2, 1, 0):
        c = C_COEF[k] + z * c
    a, b = np.where(q & 1, c, s), np.where(q & 1, s, c)
    sn = np.where(q >= 2, -a, a)
    cs = np.where((q == 1) | (q == 2), -b, b)
    return f32(sn, cs)


def dot(ax, ay, az, bx, by, bz):
    r = F(0) + ax * bx
    r = r + ay * by
    return f32(r + az * bz)


def basis(nx, ny, nz):
    """Duff et al. 2017 orthonormal basis (t, b) of the unit vector n."""
    sg = np.copysign(F(1), nz).astype(F)
    a = F(-1) / (sg + nz)
    b = (nx * ny) * a
    t = (F(1) + ((sg * nx) * nx) * a, sg * b, (-sg) * nx)
    bt = (b, sg + (ny * ny) * a, -ny)
    f32(*t, *bt)
    return t, bt


def fresnel(c):
    """Re, Tr of the header's REFR branch for c = 1 - cos."""
    c5 = (((c * c) * c) * c) * c
    re = C["APT_MAT_R0"] + C["APT_MAT_1MR0"] * c5
    return f32(re, F(1) - re)


def _intersect(o, d, geo, eps, skip):
    """-> (tmin, idx): render_do_ex's K-mode test of every sphere, the skip sphere excluded; idx -1 = no hit."""
    cx, cy, cz, r2 = geo
    ocx, ocy, ocz = cx[None, :] - o[0][:, None], cy[None, :] - o[1][:, None], cz[None, :] - o[2][:, None]
    b = ocx * d[0][:, None]
    b = b + ocy * d[1][:, None]
    b = b + ocz * d[2][:, None]
    c = ocx * ocx
    c = c + ocy * ocy
    c = c + ocz * ocz
    c = c - r2[None, :]
    disc = b * b
    disc = disc - c
    q = np.sqrt(disc)
    t0, t1 = b - q, b + q
    t = np.where(t0 > eps, t0, t1)
    t = np.where(t > eps, t, MISS)
    f32(t)
    rows = np.nonzero(skip >= 0)[0]
    t[rows, skip[rows]] = MISS
    idx = np.argmin(t, axis=1)                           # first minimum = lowest index on ties, like the strict '<' scan
    tmin = t[np.arange(t.shape[0]), idx]
    return tmin, np.where(tmin < MISS, idx, -1)


def trace(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start=0, chunk=1 << 16):
    """rays float32 [6][n], spheres the padded [10][Ns] table, materials uint32/int32 [Ns], paths uint64 [n] (path indices)
    -> (L float32 [3][n], bad bool [n]: the path hit a bad material code)."""
    rays = np.asarray(rays, dtype=F).reshape(6, -1)
    n = rays.shape[1]
    L = np.zeros((3, n), dtype=F)
    bad_all = np.zeros(n, dtype=bool)
    step = max(1, (1 << 20) // ns) if ns > 64 else chunk   # the [paths][spheres] arrays of one chunk stay at ~4 MB
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        L[:, lo:hi], bad_all[lo:hi] = _trace_chunk(rays[:, lo:hi], spheres, materials, ns, depth, eps, seed,
                                                    np.asarray(paths, dtype=U)[lo:hi], rr_start)
    return L, bad_all


def _trace_chunk(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start):
    sph = np.asarray(spheres, dtype=F).ravel()[:10 * ns].reshape(10, ns)
    codes = np.asarray(materials).astype(np.int64).view(np.int64) & 0xFFFFFFFF
    eps = F(eps)
    o = [rays[k].copy() for k in range(3)]
    d = [rays[k].copy() for k in range(3, 6)]
    n = o[0].size
    T = [np.ones(n, F) for _ in range(3)]
    L = [np.zeros(n, F) for _ in range(3)]
    skip = np.full(n, -1, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    bad_any = np.zeros(n, dtype=bool)
    mkey, rkey = mat_key(seed, paths), rr_key(seed, paths)
    with np.errstate(all="ignore"):
        for dd in range(depth):
            tmin, k = _intersect(o, d, (sph[1], sph[2], sph[3], sph[0]), eps, skip)
            g = np.where(k < 0, 0, k)
            code = codes[g]
            hit = live & (k >= 0)
            bad = hit & (code > 2)
            bad_any |= bad
            live = hit & ~bad
            # point and normal (render_do_ex's K-mode)
            h = [o[i] + d[i] * tmin for i in range(3)]
            nr = [h[i] - sph[1 + i][g] for i in range(3)]
            ln = np.sqrt(dot(*nr, *nr))
            nu = [nr[i] / ln for i in range(3)]
            # light, throughput
            Ln = [L[i] + T[i] * sph[4 + i][g] for i in range(3)]
            Tn = [T[i] * sph[7 + i][g] for i in range(3)]
            ddn = dot(*d, *nu)
            into = ddn < F(0)
            nl = [np.where(into, nu[i], -nu[i]) for i in range(3)]
            u1, u2 = uniforms(mkey, dd)
            # SPEC / reflection
            k2 = ddn * F(2)
            refl = [d[i] - nu[i] * k2 for i in range(3)]
            # DIFF
            sn, cs = sincos(u1)
            r = np.sqrt(u2)
            (tx, ty, tz), (bx, by, bz) = basis(*nl)
            cr, sr, w = cs * r, sn * r, np.sqrt(F(1) - u2)
            v = [(tx * cr + bx * sr) + nl[0] * w, (ty * cr + by * sr) + nl[1] * w, (tz * cr + bz * sr) + nl[2] * w]
            vl = np.sqrt(dot(*v, *v))
            diff = [v[i] / vl for i in range(3)]
            # REFR
            dn = np.where(into, ddn, -ddn)
            nnt = np.where(into, C["APT_MAT_NNT_IN"], F(1.5))
            cos2t = F(1) - (nnt * nnt) * (F(1) - dn * dn)
            tir = cos2t < F(0)
            gg = dn * nnt + np.sqrt(cos2t)
            gg = np.where(into, gg, -gg)
            v = [d[i] * nnt - nu[i] * gg for i in range(3)]
            vl = np.sqrt(dot(*v, *v))
            tdir = [v[i] / vl for i in range(3)]
            cc = F(1) - np.where(into, -ddn, dot(*tdir, *nu))
            re, tr = fresnel(cc)
            P = F(0.25) + F(0.5) * re
            take_r = u1 < P
            wt = np.where(take_r, re / P, tr / (F(1) - P))
            is_d, is_r = code == DIFF, (code == REFR) & ~tir
            refract = is_r & ~take_r
            newd = [np.where(is_d, diff[i], np.where(refract, tdir[i], refl[i])) for i in range(3)]
            Tn = [np.where(is_r, Tn[i] * wt, Tn[i]) for i in range(3)]
            outward = np.where(refract, ~into, into)
            f32(*h, *Ln, *Tn, *newd)
            for i in range(3):
                L[i] = np.where(live, Ln[i], L[i])
                T[i] = np.where(live, Tn[i], T[i])
                d[i] = np.where(live, newd[i], d[i])
                o[i] = np.where(live, h[i], o[i])
            skip = np.where(live, np.where(outward, k, -1), skip)
            if rr_start and dd + 1 >= rr_start:
                T = roulette(T, live, rkey, dd)
            if not live.any():
                break
    return np.stack(L), bad_any


def roulette(T, alive, key, bounce):
    """APT_FLAG_RR (include/render_mi355x.h) on the throughput."""
    q = T[0]
    q = np.where(T[1] > q, T[1], q)
    q = np.where(T[2] > q, T[2], q)
    act = alive & (q > F(0))
    p = np.where(q < F(0.05), F(0.05), q)
    p = np.where(p > F(0.95), F(0.95), p)
    with np.errstate(over="ignore"):
        h = splitmix64(key + U(0x9E3779B97F4A7C15) * U(bounce + 1))
    u = (h >> U(40)).astype(F) * F(2.0 ** -24)
    kill = act & (u >= p)
    inv = F(1) / p
    f32(u, inv, *T)
    return [np.where(kill, F(0), np.where(act, t * inv, t)) for t in T]


def render_frame(params, spheres, materials, pixel_begin=0, pixel_count=None):
    """-> (fb float32 [3][count], u8 [count][3], bad [N]) of apt_render_frame_materials for `params` (an oracle.Params)."""
    from oracle import oracle
    w, h, s = params.width, params.height, params.samples
    rays = oracle.gen_rays_counter(params)
    n = rays.shape[1]
    rr = (params.rr_start or 3) if params.flags & oracle.FLAG_RR else 0
    L, bad = trace(rays, spheres, materials, params.num_spheres, params.depth, params.eps, params.seed, np.arange(n, dtype=U), rr)
    _, fb, u8 = oracle.decode_color(L, w, h, s)
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    return fb[:, pixel_begin:pixel_begin + pixel_count], u8[pixel_begin:pixel_begin + pixel_count], bad
