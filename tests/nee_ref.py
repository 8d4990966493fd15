"""NumPy restatement of the material renderer with direct light sampling (include/render_mi355x.h "per-sphere materials", the
"Direct light sampling" part: APT_FLAG_NEE), for the tests only.

Same discipline as tests/materials_ref.py, whose pieces it uses: float32 arrays vectorised over paths, every constant an np.float32,
one separately rounded operation per step in the header's order, f32() on the intermediates.  With nee=False every operation is
materials_ref.trace's, so the colours are its colours bit for bit (tests/test_nee_cpu.py asserts that).
"""
import numpy as np

import materials_ref as mr
from materials_ref import C, DIFF, F, REFR, U, basis, dot, f32, fresnel, sincos, splitmix64, uniforms

FLAG_NEE = 32
NEE_SALT = U(0xBB67AE8584CAA73B)


def nee_key(seed, path):
    return splitmix64(U(seed) ^ splitmix64(path) ^ NEE_SALT)


def light_sample(h, nl, nkey, bounce, lc, lr2):
    """The header's `sample` step for hit points h with oriented normals nl -> (ok: h strictly outside the light, l, cosl, wgt)."""
    w0 = [lc[i] - h[i] for i in range(3)]
    d2 = dot(*w0, *w0)
    ok = d2 > lr2
    x = lr2 / d2
    cmax = np.sqrt(F(1) - x)
    omc = x / (F(1) + cmax)
    v1, v2 = uniforms(nkey, bounce)
    cos_a = F(1) - v1 * omc
    sin_a = np.sqrt(F(1) - cos_a * cos_a)
    sp, cp = sincos(v2)
    dl = np.sqrt(d2)
    w = [w0[i] / dl for i in range(3)]
    (ax, ay, az), (bx, by, bz) = basis(*w)
    ca, sa = cp * sin_a, sp * sin_a
    q = [(ax * ca + bx * sa) + w[0] * cos_a, (ay * ca + by * sa) + w[1] * cos_a, (az * ca + bz * sa) + w[2] * cos_a]
    ql = np.sqrt(dot(*q, *q))
    l = [q[i] / ql for i in range(3)]
    cosl = dot(*l, *nl)
    wgt = cosl * (F(2) * omc)
    f32(d2, x, cmax, omc, cos_a, sin_a, *l, cosl, wgt)
    return ok, l, cosl, wgt


def trace(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start=0, light=-1, nee=False, chunk=1 << 16):
    """materials_ref.trace with APT_FLAG_NEE (nee=True: `light` is the light sphere, 0 <= light < ns)
    -> (L float32 [3][n], bad bool [n], segments int: traced segments, shadow segments included)."""
    rays = np.asarray(rays, dtype=F).reshape(6, -1)
    n = rays.shape[1]
    L = np.zeros((3, n), dtype=F)
    bad_all = np.zeros(n, dtype=bool)
    segments = 0
    step = max(1, (1 << 20) // ns) if ns > 64 else chunk
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        L[:, lo:hi], bad_all[lo:hi], seg = _trace_chunk(rays[:, lo:hi], spheres, materials, ns, depth, eps, seed,
                                                         np.asarray(paths, dtype=U)[lo:hi], rr_start, light, nee)
        segments += seg
    return L, bad_all, segments


def _trace_chunk(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start, light, nee):
    assert not nee or 0 <= light < ns
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
    sampled = np.zeros(n, dtype=bool)
    bad_any = np.zeros(n, dtype=bool)
    segments = 0
    mkey, rkey, nkey = mr.mat_key(seed, paths), mr.rr_key(seed, paths), nee_key(seed, paths)
    geo = (sph[1], sph[2], sph[3], sph[0])
    if nee:
        lc, lr2, lem = [sph[1 + i][light] for i in range(3)], sph[0][light], [sph[4 + i][light] for i in range(3)]
    with np.errstate(all="ignore"):
        for dd in range(depth):
            tmin, k = mr._intersect(o, d, geo, eps, skip)
            g = np.where(k < 0, 0, k)
            code = codes[g]
            hit = live & (k >= 0)
            bad = hit & (code > 2)
            bad_any |= bad
            live = hit & ~bad
            segments += int(live.sum())
            h = [o[i] + d[i] * tmin for i in range(3)]
            nr = [h[i] - sph[1 + i][g] for i in range(3)]
            ln = np.sqrt(dot(*nr, *nr))
            nu = [nr[i] / ln for i in range(3)]
            # light: not the light's emission again when the previous bounce sampled it
            Ln = [L[i] + T[i] * sph[4 + i][g] for i in range(3)]
            if nee:
                noem = sampled & (k == light)
                Ln = [np.where(noem, L[i], Ln[i]) for i in range(3)]
            Tn = [T[i] * sph[7 + i][g] for i in range(3)]
            ddn = dot(*d, *nu)
            into = ddn < F(0)
            nl = [np.where(into, nu[i], -nu[i]) for i in range(3)]
            u1, u2 = uniforms(mkey, dd)
            k2 = ddn * F(2)
            refl = [d[i] - nu[i] * k2 for i in range(3)]
            sn, cs = sincos(u1)
            r = np.sqrt(u2)
            (tx, ty, tz), (bx, by, bz) = basis(*nl)
            cr, sr, w = cs * r, sn * r, np.sqrt(F(1) - u2)
            v = [(tx * cr + bx * sr) + nl[0] * w, (ty * cr + by * sr) + nl[1] * w, (tz * cr + bz * sr) + nl[2] * w]
            vl = np.sqrt(dot(*v, *v))
            diff = [v[i] / vl for i in range(3)]
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
            # sample + shadow: DIFF hits of live paths, never at the last bounce
            new_sampled = np.zeros(n, dtype=bool)
            if nee and dd + 1 < depth:
                ok, l, cosl, wgt = light_sample(h, nl, nkey, dd, lc, lr2)
                can = live & is_d & (k != light) & ok
                want = can & (cosl > F(0))
                rows = np.nonzero(want)[0]
                segments += rows.size
                if rows.size:
                    sskip = np.where(into, k, -1)[rows]
                    _, ks = mr._intersect([h[i][rows] for i in range(3)], [l[i][rows] for i in range(3)], geo, eps, sskip)
                    vis = np.zeros(n, dtype=bool)
                    vis[rows] = ks == light
                    add = [(Tn[i] * lem[i]) * wgt for i in range(3)]
                    f32(*add)
                    Ln = [np.where(vis, Ln[i] + add[i], Ln[i]) for i in range(3)]
                new_sampled = can
            f32(*h, *Ln, *Tn, *newd)
            for i in range(3):
                L[i] = np.where(live, Ln[i], L[i])
                T[i] = np.where(live, Tn[i], T[i])
                d[i] = np.where(live, newd[i], d[i])
                o[i] = np.where(live, h[i], o[i])
            skip = np.where(live, np.where(outward, k, -1), skip)
            sampled = np.where(live, new_sampled, sampled)
            if rr_start and dd + 1 >= rr_start:
                T = mr.roulette(T, live, rkey, dd)
            if not live.any():
                break
    return np.stack(L), bad_any, segments


def render_frame(params, spheres, materials, pixel_begin=0, pixel_count=None):
    """-> (fb float32 [3][count], u8 [count][3], bad [N]) of apt_render_frame_materials for `params` (an oracle.Params); APT_FLAG_NEE
    is read from params.flags and the light from params.light_index."""
    from oracle import oracle
    w, h, s = params.width, params.height, params.samples
    rays = oracle.gen_rays_counter(params)
    n = rays.shape[1]
    rr = (params.rr_start or 3) if params.flags & oracle.FLAG_RR else 0
    L, bad, _ = trace(rays, spheres, materials, params.num_spheres, params.depth, params.eps, params.seed, np.arange(n, dtype=U), rr,
                      light=params.light_index, nee=bool(params.flags & FLAG_NEE))
    _, fb, u8 = oracle.decode_color(L, w, h, s)
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    return fb[:, pixel_begin:pixel_begin + pixel_count], u8[pixel_begin:pixel_begin + pixel_count], bad
