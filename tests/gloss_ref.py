"""NumPy restatement of the material renderer with the rough-metal material (include/render_mi355x.h "per-sphere materials": the GLOSS
block and APT_FLAG_GLOSS), for the tests only.

The whole bounce in one place, in all three light modes: plain, direct light sampling (nee=True, the sphere `light`) and a light table
(table=the words).  Same discipline as tests/materials_ref.py, whose primitives it uses: float32 arrays vectorised over paths, every
constant an np.float32, one separately rounded operation per step in the header's order, f32() on the intermediates -- f32 fails on a
float64 one.  On a table without gloss words its colours are materials_ref's, nee_ref's and lights_ref's bit for bit
(tests/test_gloss_cpu.py asserts that), with and without the flag."""
import numpy as np

from materials_ref import C, DIFF, F, REFR, U, _intersect, basis, dot, f32, fresnel, mat_key, roulette, rr_key, sincos, splitmix64, uniforms

GLOSS = 3
FLAG_RR, FLAG_NEE, FLAG_GLOSS = 2, 32, 64
NEE_SALT = U(0xBB67AE8584CAA73B)
LIGHT_SALT = U(0x3C6EF372FE94F82B)
LIGHTS_MAGIC, LIGHTS_HEAD = 0x4C474854, 16


def word(q):
    """APT_MAT_GLOSS_WORD(q)."""
    return GLOSS | (int(q) << 8)


def decode(materials, gloss):
    """The material words as the kernels read them -> (code int64 [Ns]: 0..2, 3 = gloss, anything else bad; alpha float32 [Ns])."""
    w = np.asarray(materials).astype(np.int64) & 0xFFFFFFFF
    if not gloss:
        return w, np.zeros(w.size, F)
    q = (w >> 8) & 0xFFFF
    well = ((w & 0xFF) == GLOSS) & (q != 0) & ((w >> 24) == 0)
    code = np.where(w <= 2, w, np.where(well, GLOSS, 15))
    alpha = q.astype(F) * F(2.0 ** -16)
    return code, f32(alpha)


def flags_of(materials):
    """apt_materials_flags_host restated."""
    code, _ = decode(materials, True)
    return FLAG_GLOSS if (code == GLOSS).any() else 0


def gloss_sample(d, nl, alpha, u1, u2):
    """The header's GLOSS block for directions d at oriented normals nl -> (new direction, g = G1(l), up: l.z > 0)."""
    (tx, ty, tz), (bx, by, bz) = basis(*nl)
    w = [-d[0], -d[1], -d[2]]
    vx, vy, vz = dot(*w, tx, ty, tz), dot(*w, bx, by, bz), dot(*w, *nl)
    s0x, s0y = alpha * vx, alpha * vy
    sl = np.sqrt(dot(s0x, s0y, vz, s0x, s0y, vz))
    sx, sy, sz = s0x / sl, s0y / sl, vz / sl
    sn, cs = sincos(u1)
    z = (F(1) - u2) * (F(1) + sz) - sz
    r2 = F(1) - z * z
    r = np.sqrt(np.where(r2 > F(0), r2, F(0)))
    m0x, m0y, m0z = alpha * (r * cs + sx), alpha * (r * sn + sy), z + sz
    ml = np.sqrt(dot(m0x, m0y, m0z, m0x, m0y, m0z))
    mx, my, mz = m0x / ml, m0y / ml, m0z / ml
    vm2 = F(2) * dot(vx, vy, vz, mx, my, mz)
    lx, ly, lz = mx * vm2 - vx, my * vm2 - vy, mz * vm2 - vz
    a2 = alpha * alpha
    g = (F(2) * lz) / (lz + np.sqrt(a2 + (F(1) - a2) * (lz * lz)))
    q = [(tx * lx + bx * ly) + nl[0] * lz, (ty * lx + by * ly) + nl[1] * lz, (tz * lx + bz * ly) + nl[2] * lz]
    ql = np.sqrt(dot(*q, *q))
    newd = [q[i] / ql for i in range(3)]
    f32(vx, vy, vz, sx, sy, sz, z, r, mx, my, mz, lx, ly, lz, g, *newd)
    return newd, g, lz > F(0)


def light_sample(h, nl, nkey, bounce, lc, lr2):
    """The header's `sample` step of "Direct light sampling" -> (ok: h strictly outside the light, l, cosl, wgt)."""
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


class Table:
    """A light table (the header's "several lights" layout) as the kernels read it."""

    def __init__(self, words):
        t = np.ascontiguousarray(words).view(np.uint32).ravel()
        assert t[0] == LIGHTS_MAGIC and t.size == t[3]
        self.ns, self.n = int(t[1]), int(t[2])
        n = self.n
        self.idx = t[LIGHTS_HEAD:LIGHTS_HEAD + n].astype(np.int64)
        self.cdf = t[LIGHTS_HEAD + n:LIGHTS_HEAD + 2 * n].view(F).copy()
        self.invp = t[LIGHTS_HEAD + 2 * n:LIGHTS_HEAD + 3 * n].view(F).copy()
        bits = t[LIGHTS_HEAD + 3 * n:]
        self.listed = ((bits[np.arange(self.ns) >> 5] >> (np.arange(self.ns) & 31).astype(np.uint32)) & 1).astype(bool)


def trace(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start=0, light=-1, nee=False, table=None, gloss=True, chunk=1 << 16):
    """rays float32 [6][n], spheres the padded [10][Ns] table, materials the words [Ns], paths uint64 [n] (path indices); gloss: the
    launch carries APT_FLAG_GLOSS; nee / light: APT_FLAG_NEE; table: the *_lights entries (then nee / light are not read)
    -> (L float32 [3][n], bad bool [n]: the path hit a bad material word, segments int: shadow segments included)."""
    rays = np.asarray(rays, dtype=F).reshape(6, -1)
    n = rays.shape[1]
    tb = None if table is None else (table if isinstance(table, Table) else Table(table))
    assert tb is None or tb.ns == ns
    L = np.zeros((3, n), dtype=F)
    bad_all = np.zeros(n, dtype=bool)
    segments = 0
    step = max(1, (1 << 20) // ns) if ns > 64 else chunk   # the [paths][spheres] arrays of one chunk stay at ~4 MB
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        L[:, lo:hi], bad_all[lo:hi], seg = _trace_chunk(rays[:, lo:hi], spheres, materials, ns, depth, eps, seed,
                                                         np.asarray(paths, dtype=U)[lo:hi], rr_start, light, nee and tb is None, tb, gloss)
        segments += seg
    return L, bad_all, segments


def _trace_chunk(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start, light, nee, tb, gloss):
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
    kprev = np.full(n, -1, dtype=np.int64)
    bad_any = np.zeros(n, dtype=bool)
    segments = 0
    mkey, rkey = mat_key(seed, paths), rr_key(seed, paths)
    nkey = splitmix64(U(seed) ^ splitmix64(paths) ^ NEE_SALT)
    lkey = splitmix64(U(seed) ^ splitmix64(paths) ^ LIGHT_SALT)
    geo = (sph[1], sph[2], sph[3], sph[0])
    with np.errstate(all="ignore"):
        for dd in range(depth):
            # hit, code
            tmin, k = _intersect(o, d, geo, eps, skip)
            g = np.where(k < 0, 0, k)
            code, alpha = codes[g], alphas[g]
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
            re, tr = fresnel(cc)
            P = F(0.25) + F(0.5) * re
            take_r = u1 < P
            wt = np.where(take_r, re / P, tr / (F(1) - P))
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
            f32(*h, *Ln, *Tn, *newd)
            for i in range(3):
                L[i] = np.where(live, Ln[i], L[i])
                T[i] = np.where(live, Tn[i], T[i])
                d[i] = np.where(live, newd[i], d[i])
                o[i] = np.where(live, h[i], o[i])
            skip = np.where(live, np.where(outward, k, -1), skip)
            sampled = np.where(live, new_sampled, sampled)
            kprev = np.where(live, k, kprev)
            live = live & ~ended
            if rr_start and dd + 1 >= rr_start:
                T = roulette(T, live, rkey, dd)
            if not live.any():
                break
    return np.stack(L), bad_any, segments


def render_frame(params, spheres, materials, table=None, pixel_begin=0, pixel_count=None, rays=None):
    """-> (fb float32 [3][count], u8 [count][3], bad [N]) of apt_render_frame_materials (table: apt_render_frame_lights) for `params` (an
    oracle.Params); APT_FLAG_NEE / APT_FLAG_GLOSS / APT_FLAG_RR are read from params.flags.  rays: a camera's (camera_ref.rays)."""
    from oracle import oracle
    w, h, s = params.width, params.height, params.samples
    if rays is None:
        rays = oracle.gen_rays_counter(params)
    n = rays.shape[1]
    rr = (params.rr_start or 3) if params.flags & FLAG_RR else 0
    L, bad, _ = trace(rays, spheres, materials, params.num_spheres, params.depth, params.eps, params.seed, np.arange(n, dtype=U), rr,
                      light=params.light_index, nee=bool(params.flags & FLAG_NEE), table=table, gloss=bool(params.flags & FLAG_GLOSS))
    _, fb, u8 = oracle.decode_color(L, w, h, s)
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    return fb[:, pixel_begin:pixel_begin + pixel_count], u8[pixel_begin:pixel_begin + pixel_count], bad
