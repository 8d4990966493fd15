"""NumPy restatement of the material renderer with a light table (include/render_mi355x.h "several lights": the *_lights entries) and
of the table's construction (apt_build_lights_host), for the tests only.

Same discipline as tests/nee_ref.py and tests/materials_ref.py, whose pieces it uses: float32 arrays vectorised over paths, every
constant an np.float32, one separately rounded operation per step in the header's order, f32() on the intermediates.  The bounce is
nee_ref's; what differs is which light a bounce samples (one per path, by a fourth stream), the weight's invp factor, and the rule that
leaves an emission out at the next hit.  With a one-light table it equals nee_ref.trace(nee=True) bit for bit
(tests/test_lights_cpu.py asserts that)."""
import numpy as np

import materials_ref as mr
import nee_ref as nr
from materials_ref import C, DIFF, F, REFR, U, basis, dot, f32, fresnel, sincos, splitmix64, uniforms

LIGHT_SALT = U(0x3C6EF372FE94F82B)
MAGIC = 0x4C474854
HEAD = 16
DEV_LIGHTS_MISMATCH = 32


def light_key(seed, path):
    return splitmix64(U(seed) ^ splitmix64(path) ^ LIGHT_SALT)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def build_table(spheres, ns, indices=None):
    """apt_build_lights_host restated -> uint32 array, or ValueError where the library refuses.  float64 scalars, one operation at a
    time in the header's order (Python floats ARE IEEE float64; no pairwise numpy sums)."""
    sph = np.asarray(spheres, dtype=F).ravel()[:10 * ns].reshape(10, ns)
    if ns == 0:
        raise ValueError("num_spheres is 0")
    if indices is None:
        g = [k for k in range(ns) if sph[4][k] > 0 or sph[5][k] > 0 or sph[6][k] > 0]
    else:
        g = [int(k) for k in indices]
    if not g:
        raise ValueError("empty")
    if any(not 0 <= k < ns for k in g):
        raise ValueError("out of range")
    if len(set(g)) != len(g):
        raise ValueError("duplicate")
    n = len(g)
    w = []
    W = 0.0
    for k in g:
        e = (float(sph[4][k]) + float(sph[5][k])) + float(sph[6][k])
        p = e * float(sph[0][k])
        p = p if 0.0 < p < float("inf") else 0.0
        w.append(p)
        W = W + p
    by_power = 0.0 < W < float("inf")
    fl = 0.5 / float(n)
    m, S, before = [], 0.0, 0
    for i in range(n):
        a = (0.5 * w[i]) / W if by_power else fl
        S = S + (a + fl)
        mi = 1 << 24 if i + 1 == n else int(np.floor(S * 16777216.0 + 0.5))
        if mi <= before or mi > 1 << 24:
            raise ValueError("a probability below 2^-24")
        m.append(mi)
        before = mi
    nbits = (ns + 31) // 32
    out = np.zeros(HEAD + 3 * n + nbits, dtype=np.uint32)
    bits = np.zeros(nbits, dtype=np.uint32)
    for k in g:
        bits[k >> 5] |= np.uint32(1 << (k & 31))
    out[:5] = [MAGIC, ns, n, out.size, bits[0]]
    out[HEAD:HEAD + n] = g
    mm = np.array(m, dtype=np.int64)
    cdf = mm.astype(F) * F(2.0 ** -24)
    P = np.diff(mm, prepend=0).astype(F) * F(2.0 ** -24)
    invp = F(1) / P
    assert cdf.dtype == F and invp.dtype == F
    out[HEAD + n:HEAD + 2 * n] = cdf.view(np.uint32)
    out[HEAD + 2 * n:HEAD + 3 * n] = invp.view(np.uint32)
    out[HEAD + 3 * n:] = bits
    return out


class Table:
    """A light table as the kernels read it."""

    def __init__(self, words):
        t = np.ascontiguousarray(words).view(np.uint32).ravel()
        assert t[0] == MAGIC and t.size == t[3]
        self.ns, self.n = int(t[1]), int(t[2])
        n = self.n
        self.idx = t[HEAD:HEAD + n].astype(np.int64)
        self.cdf = t[HEAD + n:HEAD + 2 * n].view(F).copy()
        self.invp = t[HEAD + 2 * n:HEAD + 3 * n].view(F).copy()
        bits = t[HEAD + 3 * n:]
        self.listed = ((bits[np.arange(self.ns) >> 5] >> (np.arange(self.ns) & 31).astype(np.uint32)) & 1).astype(bool)

    def prob(self):
        return np.diff(self.cdf.astype(np.float64), prepend=0.0)


def check_table_invariants(words):
    t = Table(words)
    m = t.cdf.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(m, np.round(m)) and (np.diff(m, prepend=0.0) >= 1).all() and m[-1] == 2.0 ** 24     # on the grid, increasing, ends at 1
    P = (np.diff(m, prepend=0.0) * 2.0 ** -24).astype(F)
    assert np.array_equal((F(1) / P).view(np.uint32), t.invp.view(np.uint32))
    assert t.listed.sum() == t.n and t.listed[t.idx].all() and len(set(t.idx.tolist())) == t.n
    return t


# ---- the renderer ---------------------------------------------------------------------------------------------------------------
def trace(rays, spheres, materials, ns, depth, eps, seed, paths, table, rr_start=0, chunk=1 << 16):
    """The *_lights entries' paths -> (L float32 [3][n], bad bool [n], segments int: shadow segments included).  table: the words."""
    rays = np.asarray(rays, dtype=F).reshape(6, -1)
    n = rays.shape[1]
    tb = table if isinstance(table, Table) else Table(table)
    assert tb.ns == ns
    L = np.zeros((3, n), dtype=F)
    bad_all = np.zeros(n, dtype=bool)
    segments = 0
    step = max(1, (1 << 20) // ns) if ns > 64 else chunk
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        L[:, lo:hi], bad_all[lo:hi], seg = _trace_chunk(rays[:, lo:hi], spheres, materials, ns, depth, eps, seed,
                                                         np.asarray(paths, dtype=U)[lo:hi], rr_start, tb)
        segments += seg
    return L, bad_all, segments


def _S(c, r2, same, h):
    """The predicate S for lights with centres c and r2 seen from h; `same`: the light is the sphere we stand on."""
    w0 = [c[i] - h[i] for i in range(3)]
    d2 = dot(*w0, *w0)
    f32(d2)
    return ~same & (d2 > r2)


def _trace_chunk(rays, spheres, materials, ns, depth, eps, seed, paths, rr_start, tb):
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
    kprev = np.full(n, -1, dtype=np.int64)
    bad_any = np.zeros(n, dtype=bool)
    segments = 0
    mkey, rkey, nkey, lkey = mr.mat_key(seed, paths), mr.rr_key(seed, paths), nr.nee_key(seed, paths), light_key(seed, paths)
    geo = (sph[1], sph[2], sph[3], sph[0])
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
            nr_ = [h[i] - sph[1 + i][g] for i in range(3)]
            ln = np.sqrt(dot(*nr_, *nr_))
            nu = [nr_[i] / ln for i in range(3)]
            # light: the emission of a listed sphere is left out when the previous bounce was a sampling bounce and S held for it there
            noem = sampled & tb.listed[g] & _S([sph[1 + i][g] for i in range(3)], sph[0][g], g == kprev, o)
            Ln = [np.where(noem, L[i], L[i] + T[i] * sph[4 + i][g]) for i in range(3)]
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
            # sample + shadow: DIFF hits of live paths, never at the last bounce; one light of the table per path
            new_sampled = np.zeros(n, dtype=bool)
            if dd + 1 < depth:
                u, _ = uniforms(lkey, dd)
                i_sel = np.searchsorted(tb.cdf, u, side="right")          # the first entry with u < cdf[i]
                assert i_sel.max() < tb.n and u.dtype == F
                j = tb.idx[i_sel]
                lc, lr2 = [sph[1 + i][j] for i in range(3)], sph[0][j]
                ok, l, cosl, wgt0 = nr.light_sample(h, nl, nkey, dd, lc, lr2)
                wgt = wgt0 * tb.invp[i_sel]
                bounce = live & is_d
                can = bounce & (j != k) & ok                                 # S(j, k, h)
                want = can & (cosl > F(0))
                rows = np.nonzero(want)[0]
                segments += rows.size
                if rows.size:
                    sskip = np.where(into, k, -1)[rows]
                    _, ks = mr._intersect([h[i][rows] for i in range(3)], [l[i][rows] for i in range(3)], geo, eps, sskip)
                    vis = np.zeros(n, dtype=bool)
                    vis[rows] = ks == j[rows]
                    add = [(Tn[i] * sph[4 + i][j]) * wgt for i in range(3)]
                    f32(wgt, *add)
                    Ln = [np.where(vis, Ln[i] + add[i], Ln[i]) for i in range(3)]
                new_sampled = bounce                                         # sampled, whatever the chosen light allowed
            f32(*h, *Ln, *Tn, *newd)
            for i in range(3):
                L[i] = np.where(live, Ln[i], L[i])
                T[i] = np.where(live, Tn[i], T[i])
                d[i] = np.where(live, newd[i], d[i])
                o[i] = np.where(live, h[i], o[i])
            skip = np.where(live, np.where(outward, k, -1), skip)
            sampled = np.where(live, new_sampled, sampled)
            kprev = np.where(live, k, kprev)
            if rr_start and dd + 1 >= rr_start:
                T = mr.roulette(T, live, rkey, dd)
            if not live.any():
                break
    return np.stack(L), bad_any, segments


def render_frame(params, spheres, materials, table, pixel_begin=0, pixel_count=None):
    """-> (fb float32 [3][count], u8 [count][3], bad [N]) of apt_render_frame_lights for `params` (an oracle.Params)."""
    from oracle import oracle
    w, h, s = params.width, params.height, params.samples
    rays = oracle.gen_rays_counter(params)
    n = rays.shape[1]
    rr = (params.rr_start or 3) if params.flags & oracle.FLAG_RR else 0
    L, bad, _ = trace(rays, spheres, materials, params.num_spheres, params.depth, params.eps, params.seed, np.arange(n, dtype=U), table, rr)
    _, fb, u8 = oracle.decode_color(L, w, h, s)
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    return fb[:, pixel_begin:pixel_begin + pixel_count], u8[pixel_begin:pixel_begin + pixel_count], bad


# ---- scenes the tests share ----------------------------------------------------------------------------------------------------------
def table_of(rows):
    """rows of (radius, centre, emission, albedo) -> the zero-padded [10][Ns] table."""
    rows = np.array(rows, dtype=np.float64)
    rows[:, 0] = rows[:, 0] ** 2
    ns = rows.shape[0]
    out = np.zeros((ns * 10 + 127) // 128 * 128, dtype=np.float32)
    out[:10 * ns] = rows.T.astype(np.float32).ravel()
    return out


def demo_two_lights(gen_data):
    """The demo scene (9 spheres, glass ball) with the mirror ball, sphere 6 (APT_MAT_SPEC), given emission next to the stock light 7."""
    sph, mat = gen_data.gen_spheres_materials()
    sph = np.array(sph, dtype=F)
    sph[:90].reshape(10, 9)[4:7, 6] = [F(3.0), F(6.0), F(9.0)]
    return sph, np.asarray(mat, dtype=np.int32), 9


def furnace(lamp):
    """The white furnace of tests/test_gpu_materials.py (albedo 0.5, emission 0.25, radius 1000 around the camera; render it with
    eps = 0.5); lamp: a small bright sphere inside it as sphere 1."""
    rows = [[1000.0, 50.0, 52.0, 295.6, 0.25, 0.25, 0.25, 0.5, 0.5, 0.5]]
    if lamp:
        rows.append([20.0, 120.0, 200.0, -100.0, 30.0, 20.0, 10.0, 0.0, 0.0, 0.0])
    return table_of(rows), np.full(len(rows), DIFF, dtype=np.int32), len(rows)


def two_lamps(gen_data):
    """The 8-sphere DIFF scene with spheres 6 and 7 both lamps, of different colour and radius (sphere 6 keeps its place: the mirror
    ball's, on the floor; sphere 7 is smallpt's lamp under the ceiling)."""
    sph, mat, ns, _ = gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 8, 7
    sph = gen_data.with_lamps(sph, ns, [6, 7], radius=[4.0, 1.5], centres=[(27.0, 16.5, 47.0), (50.0, 81.6 - 16.5, 81.6)],
                              emission=[(60.0, 30.0, 15.0), 400.0])
    mat = mat.copy()
    mat[6] = DIFF
    return sph, mat, ns


def sixteen_lamps(gen_data, ns=1030, seed=5):
    """gen_scene's big scene with 16 of its small spheres turned into lamps of unequal power (radius 0.6 .. 2.1, emission 20 .. 320)."""
    sph, mat = gen_data.gen_scene_materials(ns, seed=seed)
    idx = [6 + 61 * i for i in range(16)]
    sph = gen_data.with_lamps(sph, ns, idx, radius=[0.6 + 0.1 * i for i in range(16)],
                              emission=[(20.0 * (i + 1), 10.0 * (i + 1), 5.0 * (16 - i)) for i in range(16)])
    return sph, np.asarray(mat, dtype=np.int32), ns, idx


def three_lights_point(j, per):
    """One point of the closed-form scene: a floor sphere under three listed sphere lights, two unoccluded with different radius,
    distance and emission, one below the horizon -> (rays [6][per], table, materials, ns, paths, the closed form per channel)."""
    R, alb = 1000.0, 0.75
    lights = [(2.0, (0.0, 10.0, 0.0), (50.0, 20.0, 5.0)), (1.0, (6.0, 7.0, -3.0), (10.0, 80.0, 40.0)), (3.0, (0.0, -2000.0 - 20.0, 0.0), (70.0, 70.0, 70.0))]
    rows = [[R, 0, -R, 0, 0, 0, 0, alb, alb, alb]] + [[r, *c, *e, 0, 0, 0] for r, c, e in lights]
    sph = table_of(rows)
    mat = np.array([DIFF] * 4, dtype=np.int32)
    px = 2.0 * j - 6.0
    tgt = np.array([px, np.sqrt(R * R - px * px) - R, 0.0])                           # on the floor sphere
    o = tgt + np.array([0.0, 5.0, 0.5])
    dd = (tgt - o) / np.linalg.norm(tgt - o)
    rays = np.tile(np.concatenate([o, dd])[:, None], (1, per)).astype(F)
    paths = np.arange(j * per, (j + 1) * per, dtype=np.uint64)
    nrm = (tgt - np.array([0.0, -R, 0.0])) / R
    want = np.zeros(3)
    for r, c, e in lights[:2]:
        w = np.array(c) - tgt
        dist = np.linalg.norm(w)
        want += alb * np.array(e) * (r / dist) ** 2 * (w @ nrm) / dist
    return rays, sph, mat, 4, paths, want
