"""CPU-only: APT_FLAG_MIS (include/render_mi355x.h "Multiple importance sampling") in the restatement tests/materials_ref.py
(trace(mis=True)) -- the flagless bytes wherever the flag is not read, the float64 quadrature of tests/mis_physics.py (which shares no
text with it) where it is, its finiteness at the edges of the roughness and of the geometry, the variance it is there to remove, and the
Python side of the flag.  What the flag computes, and that the flagless trace is what it was before the flag existed, is held by the
recorded bytes of tests/test_restatement_frozen.py.

The physics rule: N copies of one ray, |mean - expectation| <= 5 joint standard errors per channel, the joint standard error being
sqrt(se^2 + quad_err^2) with se the standard error of the mean and quad_err the quadrature's own error (its difference between n and
2 n cells)."""
import math

import numpy as np
import pytest

import lights_ref as lr
import materials_ref as mr
import mis_physics as mp
from gpu_harness import host, scene, sky_and_sun  # noqa: F401

F, U = np.float32, np.uint64
EPS = 1e-4
QS = {"0.05": 3277, "0.3": 19661, "1-2^-16": 65535}      # gen_data.gloss(alpha)'s q
N_COPIES = 16384


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _same(a, b):
    return _bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


# ---- the flag's Python side ---------------------------------------------------------------------------------------------------------
def test_the_flag_and_materials_flags(host):
    from ascendpathtracing_amd import _lib
    assert _lib.APT_FLAG_MIS == 128 == host.APT_FLAG_MIS == mr.FLAG_MIS
    gd = host.gen_data
    glossy, plain = [1, gd.gloss(0.3), 0], [1, 2, 0]
    assert gd.gloss(0.05) >> 8 == QS["0.05"] and gd.gloss(0.3) >> 8 == QS["0.3"] and gd.gloss(1 - 2.0 ** -16) >> 8 == QS["1-2^-16"]
    assert gd.materials_flags(glossy) == gd.materials_flags(glossy, mis=False) == host.APT_FLAG_GLOSS
    assert gd.materials_flags(glossy, mis=True) == host.APT_FLAG_GLOSS | host.APT_FLAG_MIS
    assert gd.materials_flags(plain, mis=True) == 0 == gd.materials_flags(plain)
    import re
    header = open(mr.ROOT + "/include/render_mi355x.h").read()
    assert re.search(r"APT_FLAG_MIS\s*=\s*128u", header) and re.search(r"#define APT_ABI_VERSION\s+3\b", header)


# ---- where the flag is not read -----------------------------------------------------------------------------------------------------
def _rays(oracle, ns, w, h, s, depth, seed):
    return oracle.gen_rays_counter(oracle.make_params(w, h, s, depth=depth, num_spheres=ns, seed=seed))


@pytest.mark.parametrize("name", ["gloss8-lamp", "gloss9-lamp", "open8", "open40"])
def test_where_the_flag_is_not_read_the_result_is_the_flagless_bytes(host, oracle, name):
    sc = scene(host, name)
    env = mr.Env.from_ctypes(sky_and_sun(host, True))
    for depth in (1, 2, 5):
        rays = _rays(oracle, sc.ns, 12, 8, 1, depth, depth)
        paths = np.arange(rays.shape[1], dtype=U)
        for kw in (dict(light=sc.light, nee=True), dict(table=sc.table), {}):
            for e in (None, env):
                for rr in (0, 2):
                    a = (rays, sc.sph, sc.mat, sc.ns, depth, EPS, depth, paths, e, rr)
                    if depth == 1 or not kw:                                   # depth 1, or no light mode: the flag is not read
                        assert _same(mr.trace(*a, mis=True, **kw), mr.trace(*a, **kw)), (name, depth, kw.keys(), rr)
                    plain = (rays, sc.sph, sc.plain, sc.ns, depth, EPS, depth, paths, e, rr)
                    assert _same(mr.trace(*plain, mis=True, **kw), mr.trace(*plain, **kw)), (name, depth, "no gloss word")
                    assert _bits_equal(mr.trace(*a, mis=True, gloss=False, **kw)[0], mr.trace(*a, gloss=False, **kw)[0])   # no APT_FLAG_GLOSS


@pytest.mark.parametrize("name", ["gloss8-lamp", "gloss9-lamp", "open40"])
def test_a_one_light_table_is_nee_with_the_flag(host, oracle, name):
    sc = scene(host, name)
    one = lr.build_table(sc.sph, sc.ns, [sc.light])
    changed = 0
    for depth in (2, 3, 5):
        rays = _rays(oracle, sc.ns, 12, 8, 2, depth, 7 + depth)
        a = (rays, sc.sph, sc.mat, sc.ns, depth, EPS, 7 + depth, np.arange(rays.shape[1], dtype=U), None, 2 if depth == 5 else 0)
        nee = mr.trace(*a, light=sc.light, nee=True, mis=True)
        assert _same(mr.trace(*a, table=one, mis=True), nee), (name, depth)
        assert np.isfinite(nee[0]).all()
        changed += not _bits_equal(nee[0], mr.trace(*a, light=sc.light, nee=True)[0])
    assert changed, "the flag changed no image of this scene"


# ---- physics ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", list(QS))
@pytest.mark.parametrize("mode", ["nee", "table"])
def test_both_estimators_have_the_quadrature_as_their_mean(alpha, mode):
    q = QS[alpha]
    table, mat = mp.scene(q)
    ray = mp.mirror_ray(table)
    want, quad_err = mp.expectation(ray, table, q)
    assert (want > 0).all() and (quad_err < 1e-3 * want).all()
    rays = np.tile(ray[:, None], (1, N_COPIES))
    kw = dict(light=mp.LAMP, nee=True) if mode == "nee" else dict(table=lr.build_table(table, 2, [mp.LAMP]))
    se = {}
    for mis in (False, True):
        L, bad, _ = mr.trace(rays, table, mat, 2, 2, EPS, 5, np.arange(N_COPIES, dtype=U), mis=mis, **kw)
        assert not bad.any() and np.isfinite(L).all()
        L = L.astype(np.float64)
        mean, se[mis] = L.mean(axis=1), L.std(axis=1, ddof=1) / math.sqrt(N_COPIES)
        joint = np.sqrt(se[mis] ** 2 + quad_err ** 2)
        print(alpha, mode, "mis" if mis else "flagless", "mean", mean, "want", want, "joint se", joint, "off by", np.abs(mean - want) / joint)
        assert (se[mis] > 0).all(), "no copy found the lamp: the scene shows nothing"
        assert (np.abs(mean - want) <= 5.0 * joint).all(), (alpha, mode, mis, mean, want, joint)
    assert (se[True] < se[False]).all()


# ---- finiteness ---------------------------------------------------------------------------------------------------------------------
def _aimed(table, fractions, per, seed=11):
    """Rays at the ball from the reference eye's side, `per` of each impact parameter (a fraction of the radius)."""
    rng = np.random.default_rng(seed)
    p = table[:20].reshape(10, 2).astype(np.float64)
    c, r = p[1:4, mp.BALL], math.sqrt(p[0, mp.BALL])
    out = []
    for frac in fractions:
        for _ in range(per):
            o = c + 90.0 * (lambda v: v / np.linalg.norm(v))(rng.normal(size=3) + np.array([0.0, 1.0, 2.0]))
            w = c - o
            side = np.cross(w, rng.normal(size=3))
            side /= np.linalg.norm(side)
            sin_a = frac * r / np.linalg.norm(w)
            out.append(np.concatenate([o, math.sqrt(1.0 - sin_a * sin_a) * w / np.linalg.norm(w) + sin_a * side]))
    return np.array(out).T.astype(F)


@pytest.mark.parametrize("q", [1, 65535])
@pytest.mark.parametrize("lamp", ["small", "touching", "huge"])
def test_every_colour_is_finite_at_the_edges(q, lamp):
    r, c = {"small": (2.0, (50.0, 85.0, 110.0)), "touching": (5.0, (50.0, 40.0 + mp.BALL_R + 5.0, 80.0)), "huge": (60.0, (50.0, 125.0, 80.0))}[lamp]
    table, mat = mp.scene(q, lamp_r=r, lamp_c=c)
    rays = _aimed(table, (0.0, 0.5, 0.99, 0.9999, 0.999999), 400)
    n = rays.shape[1]
    for kw in (dict(light=mp.LAMP, nee=True), dict(table=lr.build_table(table, 2, [mp.LAMP, mp.BALL]))):
        for depth, rr in ((2, 0), (4, 2)):
            L, bad, seg = mr.trace(rays, table, mat, 2, depth, EPS, 9, np.arange(n, dtype=U), None, rr, mis=True, **kw)
            assert not bad.any() and np.isfinite(L).all() and (L >= 0).all(), (q, lamp, depth)
            assert seg > 0 and L.any()


# ---- variance -----------------------------------------------------------------------------------------------------------------------
# Measured on the restatement (this test's own numbers, alpha = 0.3, the lamp of mis_physics.scene): the summed per-pixel variance
# over the 9 pixels that the ball covers entirely is 748.06 without the flag and 0.18267 with it, a ratio of 2.44e-4.  The bound is the
# geometric mean of that ratio and 1: a clear gain, not a fit to the noise.
MEASURED_RATIO = 2.44e-4


def test_the_flag_removes_the_variance_of_a_small_lamps_highlight(oracle):
    w, h, s, seeds, q = 16, 12, 1, 32, QS["0.3"]
    table, mat = mp.scene(q)
    geo = tuple(table[:20].reshape(10, 2)[[1, 2, 3, 0]])
    pre, cover = {False: [], True: []}, None
    for seed in range(seeds):
        rays = oracle.gen_rays_counter(oracle.make_params(w, h, s, depth=2, num_spheres=2, seed=seed))
        n = rays.shape[1]
        if cover is None:                                                       # pixels all of whose camera rays meet the ball
            with np.errstate(all="ignore"):
                _, k = mr._intersect([rays[i] for i in range(3)], [rays[i] for i in range(3, 6)], geo, F(EPS), np.full(n, -1))
            cover = oracle.decode_color(np.tile((k == mp.BALL).astype(F), (3, 1)), w, h, s)[0][:, 0] == 1.0
            assert cover.sum() >= 8
        for mis in (False, True):
            L, bad, _ = mr.trace(rays, table, mat, 2, 2, EPS, seed, np.arange(n, dtype=U), light=mp.LAMP, nee=True, mis=mis)
            assert not bad.any() and np.isfinite(L).all()
            pre[mis].append(oracle.decode_color(L, w, h, s)[0][cover])          # the float64 mean before the clip, per pixel
    var = {m: float(np.array(pre[m]).var(axis=0, ddof=1).sum()) for m in pre}
    ratio = var[True] / var[False]
    print("variance without the flag %.6g, with it %.6g, ratio %.4g" % (var[False], var[True], ratio))
    assert var[False] > 0 and ratio <= math.sqrt(MEASURED_RATIO * 1.0)
