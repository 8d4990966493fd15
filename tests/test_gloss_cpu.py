"""CPU-only: the rough-metal material (include/render_mi355x.h GLOSS, APT_FLAG_GLOSS) -- the restatement tests/materials_ref.py with
APT_FLAG_GLOSS against itself without the flag, bit for bit, where no gloss word is in play, against the float64 expectation of tests/gloss_physics.py (which
shares no text with it) where one is, the agreement of its three light modes, its near-mirror limit, and the host helpers.

The physics rule is tests/physics_ref.py's: 16384 copies of each ray, |mean - expectation| <= 5 standard errors per ray and channel,
1e-6 where all copies agree.  The expectation's own error (the difference between the midpoint rule at n and at 2n, stored in the
fixture) must stay below a fifth of that standard error for every component."""
import ctypes
import math

import numpy as np
import pytest

import gloss_physics as gp
import lights_ref as lr
import materials_ref as mr
import physics_ref as ph

F = np.float32
EPS, SEED = 1e-4, 1
LIGHT, TABLE_LIGHTS = 0, [0, 2]          # walls, as tests/test_gpu_glass_physics.py


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data
    pkg.gen_data = gen_data
    return pkg


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the restatement against the existing ones ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["demo9", "gen1030"])
def test_without_gloss_words_the_flag_changes_nothing_in_the_three_light_modes(apt, scene, oracle):
    if scene == "demo9":
        sph, mat, ns, light, lights, (w, h) = *lr.demo_two_lights(apt.gen_data), 7, [7, 6], (12, 8)
    else:
        sph, mat, ns, idx = lr.sixteen_lamps(apt.gen_data)
        light, lights, (w, h) = ns - 1, [ns - 1, idx[5]], (8, 6)
    assert mr.flags_of(mat) == 0
    table = lr.build_table(sph, ns, lights)
    for depth in range(1, 9):
        rr = 0 if depth == 1 else 1 + depth % 3
        rays = oracle.gen_rays_counter(oracle.make_params(w, h, 1, depth=depth, num_spheres=ns, seed=depth))
        paths = np.arange(rays.shape[1], dtype=np.uint64)
        a = (rays, sph, mat, ns, depth, EPS, depth, paths)
        for kw in ({}, dict(light=light, nee=True), dict(table=table)):    # the flag changes nothing on such a table
            without = mr.trace(*a, rr_start=rr, gloss=False, **kw)
            with_flag = mr.trace(*a, rr_start=rr, gloss=True, **kw)
            assert _bits_equal(with_flag[0], without[0]), (depth, kw)
            assert np.array_equal(with_flag[1], without[1]) and with_flag[2] == without[2] > 0


def test_a_float64_intermediate_is_refused():
    d = [np.zeros(4, F), np.zeros(4, F), -np.ones(4, F)]
    nl = [np.zeros(4, F), np.zeros(4, F), np.ones(4, F)]
    u = np.full(4, 0.25, F)
    mr.gloss_sample(d, nl, np.full(4, 0.5, F), u, u)
    with pytest.raises(AssertionError):
        mr.gloss_sample(d, nl, np.full(4, 0.5, np.float64), u, u)


# ---- the restatement against physics --------------------------------------------------------------------------------------------------
class Physics:
    def __init__(self):
        self.rays8 = gp.rays()
        self.rays = gp.copies(self.rays8)
        self.paths = np.arange(8 * gp.COPIES, dtype=np.uint64)
        self.fixture, self.doc = gp.load_fixture()
        self.scenes = {n: getattr(gp, n)() for n in ("gloss8", "gloss9")}

    def trace(self, name, mode, rr):
        sc = self.scenes[name]
        kw = dict(light=LIGHT, nee=True) if mode == "nee" else (dict(table=lr.build_table(sc.table, sc.ns, TABLE_LIGHTS)) if mode == "table" else {})
        L, bad, _ = mr.trace(self.rays, sc.table, sc.materials, sc.ns, gp.DEPTH, EPS, SEED, self.paths, rr_start=1 if rr else 0, **kw)
        assert not bad.any()
        return L


@pytest.fixture(scope="module")
def physics():
    return Physics()


def test_fixture_is_what_the_physics_gives(physics):
    """The stored expectations, recomputed; emitted() against physics_ref.nearest_hit itself on directions of its own."""
    assert physics.doc["n_quad"] == gp.N_QUAD and physics.doc["depth"] == gp.DEPTH
    for name, sc in physics.scenes.items():
        want, _ = physics.fixture[name]
        assert np.abs(gp.expectation(physics.rays8, sc) - want).max() <= 1e-12
        assert physics.doc["scenes"][name]["alpha"] == gp.alpha_of(sc)
        rng = np.random.default_rng(3)
        x = sc.centre[gp.BALL] + math.sqrt(sc.r2[gp.BALL]) * ph._unit(np.array([1.0, 2.0, -0.5]))
        dirs = np.array([ph._unit(v) for v in rng.normal(size=(256, 3))])
        got = gp.emitted(x, dirs, sc, gp.BALL)
        for i, dv in enumerate(dirs):
            _, k = ph.nearest_hit(x, dv, sc, gp.BALL)
            assert np.array_equal(got[i], sc.emission[k] if k >= 0 else np.zeros(3))


@pytest.mark.parametrize("rr", [False, True], ids=["", "rr"])
@pytest.mark.parametrize("mode", ["plain", "nee", "table"])
@pytest.mark.parametrize("name", ["gloss8", "gloss9"])
def test_restatement_against_physics(physics, name, mode, rr):
    want, quad_err = physics.fixture[name]
    c, se = gp.compare(physics.trace(name, mode, rr), want)
    print("%s %-5s%s  max |z| %.2f at %s over %d components, all-equal error %.2e, quadrature error / (standard error / 5) <= %.3f" % (
        name, mode, " rr" if rr else "", c["zmax"], c["z_at"], c["differing"], c["exact"], (quad_err / (se / 5)).max()))
    assert c["finite"] and c["differing"] >= 8
    assert (quad_err <= se / 5).all()
    assert c["zmax"] <= ph.Z_CAP and c["exact"] <= ph.EXACT_TOL


# ---- the light modes agree ------------------------------------------------------------------------------------------------------------
def test_plain_nee_and_table_agree_in_the_demo_scene(apt, oracle):
    """The demo scene with smallpt's lamp and the mirror ball as a gloss ball: the mean of a 32x24 frame at depth 5 is the same in the
    three modes, within 5 standard errors of the difference per channel.  The modes share the bounce stream, so the paths are paired:
    the standard error is that of the per-pixel differences, over the seeds together."""
    sph, mat = apt.gen_data.gen_spheres_materials(gloss=0.25)
    sph = apt.gen_data.with_lamp(sph, 9, 7)
    sph[:90].reshape(10, 9)[4:7, 6] = [F(3.0), F(6.0), F(9.0)]         # the gloss ball glows too: the table's second light
    ns, w, h, s = 9, 32, 24, 2
    assert mr.flags_of(mat) == mr.FLAG_GLOSS and (np.asarray(mat)[6] & 0xFF) == mr.GLOSS
    table = lr.build_table(sph, ns, [7, 6])
    px = {"plain": [], "nee": [], "table": []}
    for seed in (1, 2, 3):
        rays = oracle.gen_rays_counter(oracle.make_params(w, h, s, depth=5, num_spheres=ns, seed=seed))
        a = (rays, sph, mat, ns, 5, EPS, seed, np.arange(rays.shape[1], dtype=np.uint64))
        for mode, kw in (("plain", {}), ("nee", dict(light=7, nee=True)), ("table", dict(table=table))):
            L, bad, _ = mr.trace(*a, **kw)
            assert not bad.any()
            px[mode].append(L.astype(np.float64).reshape(3, w * h, 4 * s).mean(axis=2))
    px = {k: np.concatenate(v, axis=1) for k, v in px.items()}
    for a_, b_ in (("plain", "nee"), ("plain", "table"), ("nee", "table")):
        diff = px[a_] - px[b_]
        se = diff.std(axis=1, ddof=1) / math.sqrt(diff.shape[1])
        z = np.abs(diff.mean(axis=1)) / se
        print(a_, b_, "means", px[a_].mean(axis=1), px[b_].mean(axis=1), "|z|", z)
        assert (se > 0).all() and (z <= 5.0).all()


# ---- the near-mirror limit ------------------------------------------------------------------------------------------------------------
def test_q_of_one_is_a_mirror():
    """alpha = 2^-16: the sampled direction is the mirror direction to 1e-3 and the weight is at least 0.999.

    Which draws: GGX has a heavy tail at every alpha, so "every draw" cannot hold -- the half vector's tilt is
    alpha * sqrt((1 - z) / (1 + z)) with 1 + z = 2 (1 - u2) for s = (0, 0, 1), at most alpha * sqrt(1 / (1 - u2)), and the reflected direction moves by
    twice that: 2 alpha / sqrt(1 - u2) <= 1e-3 iff 1 - u2 >= (2 alpha / 1e-3)^2 = 9.3e-4.  So the bound is asserted for every draw
    with 1 - u2 >= 2^-10 = 9.77e-4 (all but 2^-10 of them; the limit 2 * 2^-16 / 2^-5 = 9.77e-4), at incidences up to 87 degrees
    (cos > 0.05), and the weight for every draw that stays above the horizon.  Measured on the 62 233 draws below: 57 in the tail, 23 of them
    beyond 1e-3 (the largest 2.8e-3); the largest outside the tail 8.8e-4."""
    rng = np.random.default_rng(11)
    n = 1 << 16
    nl = rng.normal(size=(3, n))
    nl = (nl / np.linalg.norm(nl, axis=0)).astype(F)
    d = rng.normal(size=(3, n))
    d = d / np.linalg.norm(d, axis=0)
    d = np.where((d * nl).sum(axis=0) > 0, -d, d)                       # against the normal
    cos = -(d * nl.astype(np.float64)).sum(axis=0)
    keep = cos > 0.05
    d, nl = d[:, keep].astype(F), nl[:, keep]
    u1, u2 = mr.uniforms(mr.mat_key(5, np.arange(d.shape[1], dtype=np.uint64)), 0)
    newd, g, up = mr.gloss_sample(list(d), list(nl), np.full(d.shape[1], 2.0 ** -16, F), u1, u2)
    dn = (d.astype(np.float64) * nl).sum(axis=0)
    mirror = d.astype(np.float64) - 2.0 * dn * nl
    dev = np.abs(np.array(newd, dtype=np.float64) - mirror).max(axis=0)
    body = (1.0 - u2.astype(np.float64)) >= 2.0 ** -10
    print("draws %d, in the tail %d, beyond 1e-3: %d (largest %.2e), largest outside the tail %.2e, smallest weight %.6f" % (
        dev.size, (~body).sum(), (dev > 1e-3).sum(), dev.max(), dev[body].max(), g[up].min()))
    assert body.sum() >= 0.998 * dev.size
    assert up[body].all() and dev[body].max() <= 1e-3
    assert g[up].min() >= 0.999 and g[up].max() <= 1.0


# ---- host helpers ---------------------------------------------------------------------------------------------------------------------
def test_gloss_words_and_flags(apt):
    gd, L = apt.gen_data, apt._lib.lib()
    assert apt._lib.APT_FLAG_GLOSS == 64 == mr.FLAG_GLOSS and apt._lib.MAT_GLOSS == 3 == mr.GLOSS and apt.APT_FLAG_GLOSS == 64
    assert gd.gloss(0.5) == 3 | (32768 << 8) == mr.word(32768) == gp.gloss_word(0.5)
    assert gd.gloss(0.2) == gp.gloss_word(0.2) and (gd.gloss(0.2) >> 8) == 13107
    assert gd.gloss(0.0) == 3 | (1 << 8) and gd.gloss(-1) == 3 | (1 << 8) and gd.gloss(1.0) == gd.gloss(7.0) == 3 | (65535 << 8)
    assert gd.gloss(1.0) >> 24 == 0
    flags = lambda t: (gd.materials_flags(np.array(t, dtype=np.int64)), mr.flags_of(np.array(t, dtype=np.int64)))
    assert flags([1, 0, 2]) == (0, 0)
    assert flags([1, gd.gloss(0.3), 2]) == (64, 64)
    assert flags([1, 3, 2]) == (0, 0)                                     # q == 0
    assert flags([3 | (5 << 8) | (1 << 24)]) == (0, 0)                    # a high bit
    assert flags([4 | (5 << 8)]) == (0, 0)                                # another code
    assert flags([0x80000003]) == (0, 0)
    assert flags([3 | (1 << 24), 4, gd.gloss(1.0)]) == (64, 64)           # one well-formed word is enough
    assert flags([]) == (0, 0)
    assert L.apt_materials_flags_host(None, ctypes.c_uint32(5)) == 0
    one = (ctypes.c_uint32 * 1)(gd.gloss(0.5))
    assert L.apt_materials_flags_host(one, ctypes.c_uint32(0)) == 0 and L.apt_materials_flags_host(one, ctypes.c_uint32(1)) == 64
    code, alpha = mr.decode([gd.gloss(0.5), 3, 1, 3 | (1 << 8) | (1 << 24), 4 | (9 << 8)], True)
    assert code.tolist() == [3, 15, 1, 15, 15] and alpha[0] == F(0.5)
    sph, mat = gd.gen_spheres_materials(gloss=0.25)
    sph0, mat0 = gd.gen_spheres_materials()
    assert np.array_equal(sph, sph0) and mat[6] == gd.gloss(0.25) and np.array_equal(np.delete(mat, 6), np.delete(mat0, 6)) and mat0[6] == 0
    assert gd.materials_flags(mat) == 64 and gd.materials_flags(mat0) == 0


def test_symbols_are_exported_and_declared(apt):
    text = open(mr.ROOT + "/include/render_mi355x.h").read()
    assert "APT_FLAG_GLOSS = 64u" in text and "APT_MAT_GLOSS = 3" in text and "#define APT_MAT_GLOSS_WORD(q)" in text
    assert "uint32_t apt_materials_flags_host(const uint32_t *materials_host, uint32_t num_spheres);" in text
    assert "#define APT_ABI_VERSION 3 " in text
    assert "apt_materials_flags_host" in apt._lib.ABI_SYMBOLS and hasattr(apt._lib.lib(), "apt_materials_flags_host")
