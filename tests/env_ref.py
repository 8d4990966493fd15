"""NumPy restatement of the material renderer with an environment (include/render_mi355x.h "environment": a sky and a sun for the paths
that leave the scene), for the tests only.

The whole bounce in one place, beside tests/gloss_ref.py's and not inside it: plain, direct light sampling (nee=True, the sphere
`light`), a light table (table=the words), the rough-metal material and roulette, each with the environment's three changes -- the
miss, `sampled_sun` cleared at every hit, the sun sample after a DIFF bounce.  Same discipline as tests/materials_ref.py, whose
primitives it uses: float32 arrays vectorised over paths, every constant an np.float32, one separately rounded operation per step in
the header's order, f32() on the intermediates -- f32 fails on a float64 one.  With env=None, or with an environment whose radiances
are all 0 and that has no sun, its colours are materials_ref's, nee_ref's, lights_ref's and gloss_ref's bit for bit
(tests/test_environment_cpu.py asserts that)."""
import re

import numpy as np

from gloss_ref import GLOSS, Table, decode, gloss_sample, light_sample
from materials_ref import C, DIFF, F, REFR, ROOT, U, _intersect, basis, dot, f32, fresnel, mat_key, roulette, rr_key, sincos, splitmix64, uniforms

FLAG_RR, FLAG_NEE, FLAG_GLOSS = 2, 32, 64
ENV_SAMPLE_SUN = 1
NEE_SALT = U(0xBB67AE8584CAA73B)
LIGHT_SALT = U(0x3C6EF372FE94F82B)


def _sun_salt():
    import os
    text = open(os.path.join(ROOT, "include", "render_mi355x.h")).read()
    return U(int(re.search(r"#define APT_ENV_SUN_SALT\s+(0x[0-9A-Fa-f]+)ull", text).group(1), 16))


SUN_SALT = _sun_salt()
assert int(SUN_SALT) not in (0, 0x6A09E667F3BCC909, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B, 0xA54FF53A5F1D36F1)


class Env:
    """An apt_environment as the kernels read it: float32 fields."""

    def __init__(self, horizon=(0, 0, 0), zenith=(0, 0, 0), sun_dir=(0, 1, 0), sun_radiance=(0, 0, 0), sun_omc=0.0, flags=0):
        self.horizon = [F(x) for x in horizon]
        self.zenith = [F(x) for x in zenith]
        self.sun_dir = [F(x) for x in sun_dir]
        self.sun_radiance = [F(x) for x in sun_radiance]
        self.sun_omc = F(sun_omc)
        self.flags = int(flags)

    @classmethod
    def from_ctypes(cls, e):
        """From the record the library built (ascendpathtracing_amd._lib.ApEnvironment): the fields as they are."""
        return cls(list(e.horizon), list(e.zenith), list(e.sun_dir), list(e.sun_radiance), e.sun_omc, e.flags)

    @property
    def samples_sun(self):
        return bool(self.flags & ENV_SAMPLE_SUN) and self.sun_omc > F(0)


def sky(env, dy):
    """The miss step's sky radiance along directions with y component dy -> three float32 arrays."""
    t = dy * F(0.5) + F(0.5)
    t = np.where(t > F(0), t, F(0))
    t = np.where(t < F(1), t, F(1))
    out = [env.horizon[c] + (env.zenith[c] - env.horizon[c]) * t for c in range(3)]
    f32(t, *out)
    return out


def in_sun(env, d):
    """The miss step's cone test: sun_omc > 0 and dot(d, sun_dir) >= 1.0f - sun_omc."""
    if not env.sun_omc > F(0):
        return np.zeros(d[0].shape, dtype=bool)
    return f32(dot(*d, *env.sun_dir)) >= F(1) - env.sun_omc


def sun_sample(env, nl, skey, bounce):
    """The header's `sun sample` step -> (l, cosl, wgt): "Direct light sampling" with w = sun_dir and omc = sun_omc."""
    omc = env.sun_omc
    w = env.sun_dir
    v1, v2 = uniforms(skey, bounce)
    cos_a = F(1) - v1 * omc
    sin_a = np.sqrt(F(1) - cos_a * cos_a)
    sp, cp = sincos(v2)
    (ax, ay, az), (bx, by, bz) = basis(*[np.full(v1.shape, x, F) for x in w])
    ca, sa = cp * sin_a, sp * sin_a
    q = [(ax * ca + bx * sa) + w[0] * cos_a, (ay * ca + by * sa) + w[1] * cos_a, (az * ca + bz * sa) + w[2] * cos_a]
    ql = np.sqrt(dot(*q, *q))
    l = [q[i] / ql for i in range(3)]
    cosl = dot(*l, *nl)
    wgt = cosl * (F(2) * omc)
    f32(cos_a, sin_a, *l, cosl, wgt)
    return l, cosl, wgt


def trace(rays, spheres, materials, ns, depth, eps, seed, paths, env=None, rr_start=0, light=-1, nee=False, table=None, gloss=True,
          chunk=1 << 16):
    """rays float32 [6][n], spheres the padded [10][Ns] table, materials the words [Ns], paths uint64 [n] (path indices); env: an Env or
    None (no environment); gloss: the launch carries APT_FLAG_GLOSS; nee / light: APT_FLAG_NEE; table: the *_lights entries
    -> (L float32 [3][n], bad bool [n], segments int: the lights' and the sun's shadow segments included)."""
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
                                                         np.asarray(paths, dtype=U)[lo:hi], rr_start, light, nee and tb is None, tb, gloss, env)
        segments += seg
    return L, bad_all, segments


def _trace_chunk(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start, light, nee, tb, gloss, env):
    assert not nee or 0 <= light < ns
    sph = np.asarray(spheres, dtype=F).ravel()[:10 * ns].reshape(10, ns)
    codes, alphas = decode(materials, gloss)
    top = GLOSS if gloss else REFR
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
    bad_any = np.zeros(n, dtype=bool)
    segments = 0
    mkey, rkey = mat_key(seed, paths), rr_key(seed, paths)
    nkey = splitmix64(U(seed) ^ splitmix64(paths) ^ NEE_SALT)
    lkey = splitmix64(U(seed) ^ splitmix64(paths) ^ LIGHT_SALT)
    skey = splitmix64(U(seed) ^ splitmix64(paths) ^ SUN_SALT)
    geo = (sph[1], sph[2], sph[3], sph[0])
    with np.errstate(all="ignore"):
        for dd in range(depth):
            # hit, code
            tmin, k = _intersect(o, d, geo, eps, skip)
            g = np.where(k < 0, 0, k)
            code, alpha = codes[g], alphas[g]
            # miss: the sky, and the sun unless the bounce before sampled it; the path ends
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
            # point
            h = [o[i] + d[i] * tmin for i in range(3)]
            nr = [h[i] - sph[1 + i][g] for i in range(3)]
            ln = np.sqrt(dot(*nr, *nr))
            nu = [nr[i] / ln for i in range(3)]
            # light: an emission that the previous bounce's sample stood for is left out
            noem = np.zeros(n, dtype=bool)
            if nee:
                noem = sampled & (k == light)
            elif tb is not None:
                w0 = [sph[1 + i][g] - o[i] for i in range(3)]
                noem = sampled & tb.listed[g] & (g != kprev) & (f32(dot(*w0, *w0)) > sph[0][g])
            Ln = [np.where(noem, L[i], L[i] + T[i] * sph[4 + i][g]) for i in range(3)]
            Tn = [T[i] * sph[7 + i][g] for i in range(3)]
            # orient, draws
            ddn = dot(*d, *nu)
            into = ddn < F(0)
            nl = [np.where(into, nu[i], -nu[i]) for i in range(3)]
            u1, u2 = uniforms(mkey, dd)
            # reflect (SPEC, and the reflection of REFR)
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
            re_, tr = fresnel(cc)
            P = F(0.25) + F(0.5) * re_
            take_r = u1 < P
            wt = np.where(take_r, re_ / P, tr / (F(1) - P))
            # GLOSS
            gdir, gw, up = gloss_sample(d, nl, alpha, u1, u2)
            is_d, is_r, is_g = code == DIFF, (code == REFR) & ~tir, code == GLOSS
            refract = is_r & ~take_r
            newd = [np.where(is_d, diff[i], np.where(is_g, gdir[i], np.where(refract, tdir[i], refl[i]))) for i in range(3)]
            Tn = [np.where(is_r, Tn[i] * wt, np.where(is_g, Tn[i] * gw, Tn[i])) for i in range(3)]
            outward = np.where(refract, ~into, into)
            ended = live & is_g & ~up                                    # drawn below the horizon: the path ends, L keeps its value
            # sample + shadow: DIFF hits of live paths, never at the last bounce
            new_sampled = np.zeros(n, dtype=bool)
            if (nee or tb is not None) and dd + 1 < depth:
                bounce = live & is_d
                if nee:
                    j = np.full(n, light, dtype=np.int64)
                    ok, l, cosl, wgt = light_sample(h, nl, nkey, dd, [sph[1 + i][light] for i in range(3)], sph[0][light])
                    can = bounce & (k != light) & ok
                    new_sampled = can
                else:
                    u, _ = uniforms(lkey, dd)
                    i_sel = np.searchsorted(tb.cdf, u, side="right")          # the first entry with u < cdf[i]
                    assert i_sel.max() < tb.n and u.dtype == F
                    j = tb.idx[i_sel]
                    ok, l, cosl, wgt = light_sample(h, nl, nkey, dd, [sph[1 + i][j] for i in range(3)], sph[0][j])
                    wgt = wgt * tb.invp[i_sel]
                    can = bounce & (j != k) & ok
                    new_sampled = bounce                                     # sampled, whatever the chosen light allowed
                want = can & (cosl > F(0))
                rows = np.nonzero(want)[0]
                segments += rows.size
                if rows.size:
                    sskip = np.where(into, k, -1)[rows]
                    _, ks = _intersect([h[i][rows] for i in range(3)], [l[i][rows] for i in range(3)], geo, eps, sskip)
                    vis = np.zeros(n, dtype=bool)
                    vis[rows] = ks == j[rows]
                    add = [(Tn[i] * sph[4 + i][j]) * wgt for i in range(3)]
                    f32(wgt, *add)
                    Ln = [np.where(vis, Ln[i] + add[i], Ln[i]) for i in range(3)]
            # sun sample: after the light's; the sun is visible iff the shadow segment finds no sphere
            new_sampled_sun = np.zeros(n, dtype=bool)
            if env is not None and env.samples_sun and dd + 1 < depth:
                bounce = live & is_d
                l, cosl, wgt = sun_sample(env, nl, skey, dd)
                new_sampled_sun = bounce                                     # sampled, whatever follows
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
            sampled = np.where(live, new_sampled, sampled)
            sampled_sun = np.where(live, new_sampled_sun, sampled_sun)      # cleared at every hit, set by a sampling DIFF bounce
            kprev = np.where(live, k, kprev)
            live = live & ~ended
            if rr_start and dd + 1 >= rr_start:
                T = roulette(T, live, rkey, dd)
            if not live.any():
                break
    f32(*L)
    return np.stack(L), bad_any, segments


def render_frame(params, spheres, materials, env=None, table=None, pixel_begin=0, pixel_count=None, rays=None):
    """-> (fb float32 [3][count], u8 [count][3], bad [N], segments) of apt_render_frame_materials (table: apt_render_frame_lights) with the
    environment `env` set, for `params` (an oracle.Params); APT_FLAG_NEE / APT_FLAG_GLOSS / APT_FLAG_RR are read from params.flags.
    rays: a camera's (camera_ref.rays)."""
    from oracle import oracle
    w, h, s = params.width, params.height, params.samples
    if rays is None:
        rays = oracle.gen_rays_counter(params)
    n = rays.shape[1]
    rr = (params.rr_start or 3) if params.flags & FLAG_RR else 0
    L, bad, seg = trace(rays, spheres, materials, params.num_spheres, params.depth, params.eps, params.seed, np.arange(n, dtype=U), env, rr,
                        light=params.light_index, nee=bool(params.flags & FLAG_NEE), table=table, gloss=bool(params.flags & FLAG_GLOSS))
    _, fb, u8 = oracle.decode_color(L, w, h, s)
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    return fb[:, pixel_begin:pixel_begin + pixel_count], u8[pixel_begin:pixel_begin + pixel_count], bad, seg
