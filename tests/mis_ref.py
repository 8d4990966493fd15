"""NumPy restatement of the material renderer WITH APT_FLAG_MIS (include/render_mi355x.h "Multiple importance sampling"), for the tests
only: tests/test_gpu_mis.py compares the kernels of mis.hip against this module bit for bit.

Written from the header's text.  The leaves -- the streams, sincos, dot, basis, the GLOSS and light samplers, the hit test, roulette,
the light table, the environment -- are materials_ref's own, by import; the bounce loop is restated here once more, with the flag's
three changes (the GLOSS hit's light sample, the weighted emission at the next hit, G1(l) after the shadow segment).  With mis=False the
loop is materials_ref's, and tests/test_mis_cpu.py holds it to materials_ref bit for bit; folding the flag into materials_ref's loop is a
later change of its own.

float32 throughout, one separately rounded operation per step in the header's order, as in materials_ref."""
import numpy as np

import materials_ref as mr
from materials_ref import (DIFF, GLOSS, REFR, C, F, U, Env, Table, basis, decode, dot, f32, fresnel, gloss_sample, in_sun,  # noqa: F401
                           light_key, light_sample, mat_key, nee_key, roulette, rr_key, sincos, sky, sun_key, sun_sample, uniforms, _intersect)

FLAG_MIS = 128
PI = F(float.fromhex("0x1.921fb6p+1"))        # RN(pi)
TWO_PI = F(float.fromhex("0x1.921fb6p+2"))    # RN(2 * pi)
INF = F(np.inf)


def g1(a2, z):
    """G1 of the separable Smith term for a frame direction of z component z."""
    return f32((F(2) * z) / (z + np.sqrt(a2 + (F(1) - a2) * (z * z))))


def ggx_d(a2, m):
    """D(m) of a unit half vector in the frame: k = (m.x^2 + m.y^2) + a2 * m.z^2; a2 / ((pi * k) * k)."""
    k = (m[0] * m[0] + m[1] * m[1]) + a2 * (m[2] * m[2])
    return f32(a2 / ((PI * k) * k))


def light_pdf(r2, d2, P):
    """P / (2 * pi * omc) with "Direct light sampling"'s x, cmax and omc."""
    x = r2 / d2
    cmax = np.sqrt(F(1) - x)
    omc = x / (F(1) + cmax)
    return f32(P / (TWO_PI * omc))


def gloss_frame(d, nl, alpha, u1, u2):
    """The GLOSS block's v and drawn m (both in the frame (t, bt, nl)) and the frame itself -> (v, m, t, bt)."""
    t, bt = basis(*nl)
    w = [-d[0], -d[1], -d[2]]
    v = [dot(*w, *t), dot(*w, *bt), dot(*w, *nl)]
    s0x, s0y = alpha * v[0], alpha * v[1]
    sl = np.sqrt(dot(s0x, s0y, v[2], s0x, s0y, v[2]))
    sx, sy, sz = s0x / sl, s0y / sl, v[2] / sl
    sn, cs = sincos(u1)
    z = (F(1) - u2) * (F(1) + sz) - sz
    r2 = F(1) - z * z
    r = np.sqrt(np.where(r2 > F(0), r2, F(0)))
    m0 = [alpha * (r * cs + sx), alpha * (r * sn + sy), z + sz]
    ml = np.sqrt(dot(*m0, *m0))
    m = [m0[i] / ml for i in range(3)]
    f32(*v, *m)
    return v, m, t, bt


def trace(rays, spheres, materials, ns, depth, eps, seed, paths, env=None, rr_start=0, light=-1, nee=False, table=None, gloss=True,
          chunk=1 << 16, mis=False):
    """materials_ref.trace with mis=: the launch carries APT_FLAG_MIS (read only with `gloss` and with `nee` or a table)."""
    rays = np.asarray(rays, dtype=F).reshape(6, -1)
    n = rays.shape[1]
    tb = None if table is None else (table if isinstance(table, Table) else Table(table))
    assert tb is None or tb.ns == ns
    L = np.zeros((3, n), dtype=F)
    bad_all = np.zeros(n, dtype=bool)
    segments = 0
    step = max(1, (1 << 20) // ns) if ns > 64 else chunk
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        L[:, lo:hi], bad_all[lo:hi], seg = _trace_chunk(rays[:, lo:hi], spheres, materials, ns, depth, eps, seed,
                                                         np.asarray(paths, dtype=U)[lo:hi], rr_start, light, nee and tb is None, tb, gloss, env, mis)
        segments += seg
    return L, bad_all, segments


def _trace_chunk(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start, light, nee, tb, gloss, env, mis):
    assert not nee or 0 <= light < ns
    sph = np.asarray(spheres, dtype=F).ravel()[:10 * ns].reshape(10, ns)
    codes, alphas = decode(materials, gloss)
    top = GLOSS if gloss else REFR
    has_gloss = gloss and bool((codes == GLOSS).any())
    lit = nee or tb is not None
    mis = bool(mis) and has_gloss and lit
    sun = env is not None and env.samples_sun
    eps = F(eps)
    o = [rays[k].copy() for k in range(3)]
    d = [rays[k].copy() for k in range(3, 6)]
    n = o[0].size
    T = [np.ones(n, F) for _ in range(3)]
    L = [np.zeros(n, F) for _ in range(3)]
    skip = np.full(n, -1, dtype=np.int64)
    live = np.ones(n, dtype=bool)
    sampled = np.zeros(n, dtype=bool)
    sampled_sun = np.zeros(n, dtype=bool)
    kprev = np.full(n, -1, dtype=np.int64)
    glprev = np.zeros(n, dtype=bool)                     # mis: the last sampling bounce was a GLOSS one ...
    pbprev = np.zeros(n, F)                              # ... and drew its direction under this density
    bad_any = np.zeros(n, dtype=bool)
    segments = 0
    mkey, rkey = mat_key(seed, paths), rr_key(seed, paths)
    nkey = nee_key(seed, paths) if lit else None
    lkey = light_key(seed, paths) if tb is not None else None
    skey = sun_key(seed, paths) if sun else None
    geo = (sph[1], sph[2], sph[3], sph[0])
    if mis and tb is not None:                           # P[i] = cdf[i] - cdf[i-1], exact; per entry and per listed sphere
        P_entry = f32(tb.cdf - np.concatenate([np.zeros(1, F), tb.cdf[:-1]]))
        P_sphere = np.zeros(ns, F)
        P_sphere[tb.idx] = P_entry
    with np.errstate(all="ignore"):
        for dd in range(depth):
            tmin, k = _intersect(o, d, geo, eps, skip)
            g = np.where(k < 0, 0, k)
            code = codes[g]
            if env is not None:
                miss = live & (k < 0)
                s = sky(env, d[1])
                Lm = [L[i] + T[i] * s[i] for i in range(3)]
                add_sun = in_sun(env, d) & ~sampled_sun
                Lm = [np.where(add_sun, Lm[i] + T[i] * env.sun_radiance[i], Lm[i]) for i in range(3)]
                f32(*Lm)
                L = [np.where(miss, Lm[i], L[i]) for i in range(3)]
            hit = live & (k >= 0)
            bad = hit & (code > top)
            bad_any |= bad
            live = hit & ~bad
            segments += int(live.sum())
            h = [o[i] + d[i] * tmin for i in range(3)]
            nr = [h[i] - sph[1 + i][g] for i in range(3)]
            ln = np.sqrt(dot(*nr, *nr))
            nu = [nr[i] / ln for i in range(3)]
            # light: left out after a DIFF sample that stood for it, weighted after a GLOSS sample, else in full
            Ln = [L[i] + T[i] * sph[4 + i][g] for i in range(3)]
            if lit:
                w0 = [sph[1 + i][g] - o[i] for i in range(3)]
                d2o = f32(dot(*w0, *w0))
                if nee:
                    noem = sampled & (k == light)
                else:
                    noem = sampled & tb.listed[g] & (g != kprev) & (d2o > sph[0][g])
                if mis:
                    pl = light_pdf(sph[0][g], d2o, F(1) if nee else P_sphere[g])
                    tot = pbprev + pl
                    wb = np.where((tot > F(0)) & (tot < INF), pbprev / tot, F(1))
                    Lw = [L[i] + (T[i] * sph[4 + i][g]) * wb for i in range(3)]
                    f32(wb, *Lw)
                    Ln = [np.where(noem & glprev, Lw[i], Ln[i]) for i in range(3)]
                    noem = noem & ~glprev
                Ln = [np.where(noem, L[i], Ln[i]) for i in range(3)]
            Tn = [T[i] * sph[7 + i][g] for i in range(3)]
            Ta = Tn                                          # T after `T *= albedo`: what every light sample of this bounce uses
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
            re_, tr = fresnel(cc)
            P = F(0.25) + F(0.5) * re_
            take_r = u1 < P
            wt = np.where(take_r, re_ / P, tr / (F(1) - P))
            is_d, is_r = code == DIFF, (code == REFR) & ~tir
            is_g = np.zeros(n, dtype=bool)
            refract = is_r & ~take_r
            newd = [np.where(is_d, diff[i], np.where(refract, tdir[i], refl[i])) for i in range(3)]
            Tw = [np.where(is_r, Tn[i] * wt, Tn[i]) for i in range(3)]
            outward = np.where(refract, ~into, into)
            ended = None
            up = np.zeros(n, dtype=bool)
            if has_gloss:
                gdir, gw, up = gloss_sample(d, nl, alphas[g], u1, u2)
                is_g = code == GLOSS
                newd = [np.where(is_g, gdir[i], newd[i]) for i in range(3)]
                Tw = [np.where(is_g, Tn[i] * gw, Tw[i]) for i in range(3)]   # (with mis: after the shadow segment, which uses Ta)
                ended = live & is_g & ~up
            Tn = Tw
            # sample + shadow: DIFF hits of live paths and, with mis, GLOSS hits (whether or not their own direction was accepted: a path
            # that ends here still adds its light sample); never at the last bounce
            new_sampled = np.zeros(n, dtype=bool)
            new_gl = np.zeros(n, dtype=bool)
            new_pb = np.zeros(n, F)
            if lit and dd + 1 < depth:
                bounce = live & is_d
                gbounce = live & is_g if mis else np.zeros(n, dtype=bool)
                if nee:
                    j = np.full(n, light, dtype=np.int64)
                    Pj = np.ones(n, F)
                    ok, l, cosl, wgt = light_sample(h, nl, nkey, dd, [sph[1 + i][light] for i in range(3)], sph[0][light])
                    can = (bounce | gbounce) & (k != light) & ok
                    new_sampled = can
                else:
                    u, _ = uniforms(lkey, dd)
                    i_sel = np.searchsorted(tb.cdf, u, side="right")
                    assert i_sel.max() < tb.n and u.dtype == F
                    j = tb.idx[i_sel]
                    ok, l, cosl, wgt = light_sample(h, nl, nkey, dd, [sph[1 + i][j] for i in range(3)], sph[0][j])
                    wgt = wgt * tb.invp[i_sel]
                    can = (bounce | gbounce) & (j != k) & ok
                    new_sampled = bounce | gbounce
                    if mis:
                        Pj = P_entry[i_sel]
                want = can & (cosl > F(0))
                if mis:
                    alpha = alphas[g]
                    a2 = alpha * alpha
                    vf, mf, tf, btf = gloss_frame(d, nl, alpha, u1, u2)
                    g1v = g1(a2, vf[2])
                    new_pb = f32((g1v * ggx_d(a2, mf)) / (F(4) * vf[2]))
                    new_gl = gbounce
                    wl = [dot(*l, *tf), dot(*l, *btf), dot(*l, *nl)]
                    hm0 = [vf[i] + wl[i] for i in range(3)]
                    hl = np.sqrt(dot(*hm0, *hm0))
                    hm = [hm0[i] / hl for i in range(3)]
                    pb = (g1v * ggx_d(a2, hm)) / (F(4) * vf[2])
                    w0 = [sph[1 + i][j] - h[i] for i in range(3)]
                    pl = light_pdf(sph[0][j], dot(*w0, *w0), Pj)
                    tot = pb + pl
                    wg = g1(a2, wl[2]) * (pb / tot)
                    f32(pb, pl, tot, wg)
                    wgt = np.where(is_g, wg, wgt)
                    want = want & (~is_g | ((tot > F(0)) & (tot < INF)))
                rows = np.nonzero(want)[0]
                segments += rows.size
                if rows.size:
                    sskip = np.where(into, k, -1)[rows]
                    _, ks = _intersect([h[i][rows] for i in range(3)], [l[i][rows] for i in range(3)], geo, eps, sskip)
                    vis = np.zeros(n, dtype=bool)
                    vis[rows] = ks == j[rows]
                    add = [(Ta[i] * sph[4 + i][j]) * wgt for i in range(3)]
                    f32(wgt, *add)
                    Ln = [np.where(vis, Ln[i] + add[i], Ln[i]) for i in range(3)]
            new_sampled_sun = np.zeros(n, dtype=bool)
            if sun and dd + 1 < depth:                       # the sun stays a DIFF-only matter
                bounce = live & is_d
                l, cosl, wgt = sun_sample(env, nl, skey, dd)
                new_sampled_sun = bounce
                want = bounce & (cosl > F(0))
                rows = np.nonzero(want)[0]
                segments += rows.size
                if rows.size:
                    sskip = np.where(into, k, -1)[rows]
                    _, ks = _intersect([h[i][rows] for i in range(3)], [l[i][rows] for i in range(3)], geo, eps, sskip)
                    vis = np.zeros(n, dtype=bool)
                    vis[rows] = ks < 0
                    add = [(Tn[i] * env.sun_radiance[i]) * wgt for i in range(3)]
                    f32(wgt, *add)
                    Ln = [np.where(vis, Ln[i] + add[i], Ln[i]) for i in range(3)]
            f32(*h, *Ln, *Tn, *newd)
            for i in range(3):
                L[i] = np.where(live, Ln[i], L[i])
                T[i] = np.where(live, Tn[i], T[i])
                d[i] = np.where(live, newd[i], d[i])
                o[i] = np.where(live, h[i], o[i])
            skip = np.where(live, np.where(outward, k, -1), skip)
            if lit:
                sampled = np.where(live, new_sampled, sampled)
                kprev = np.where(live, k, kprev)
                glprev = np.where(live, new_gl, glprev)
                pbprev = np.where(live, new_pb, pbprev)
            if sun:
                sampled_sun = np.where(live, new_sampled_sun, sampled_sun)
            if ended is not None:
                live = live & ~ended
            if rr_start and dd + 1 >= rr_start:
                T = roulette(T, live, rkey, dd)
            if not live.any():
                break
    f32(*L)
    return np.stack(L), bad_any, segments


def render_frame(params, spheres, materials, env=None, table=None, pixel_begin=0, pixel_count=None, rays=None, mis=None):
    """materials_ref.render_frame with mis=: None reads APT_FLAG_MIS from params.flags, like the other flags."""
    from oracle import oracle
    w, h, s = params.width, params.height, params.samples
    if rays is None:
        rays = oracle.gen_rays_counter(params)
    n = rays.shape[1]
    rr = (params.rr_start or 3) if params.flags & mr.FLAG_RR else 0
    mis = bool(params.flags & FLAG_MIS) if mis is None else bool(mis)
    L, bad, seg = trace(rays, spheres, materials, params.num_spheres, params.depth, params.eps, params.seed, np.arange(n, dtype=U), env, rr,
                        light=params.light_index, nee=bool(params.flags & mr.FLAG_NEE), table=table, gloss=bool(params.flags & mr.FLAG_GLOSS),
                        mis=mis)
    _, fb, u8 = oracle.decode_color(L, w, h, s)
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    return fb[:, pixel_begin:pixel_begin + pixel_count], u8[pixel_begin:pixel_begin + pixel_count], bad, seg
