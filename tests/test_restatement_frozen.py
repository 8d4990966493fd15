"""CPU-only: the NumPy restatement tests/materials_ref.py against recorded bytes (tests/golden/restatement_hashes.json).

The restatement once existed as six modules, one per material feature, each with a bounce loop of its own.  Before they were folded
into one, every case below was run through the module that owned it and the SHA-256 of the colours, of the bad-material mask and the
segment count were written down.  The one loop must still give those bytes, in every mode a module had: plain, APT_FLAG_NEE on and off,
a light table, the rough-metal material with and without APT_FLAG_GLOSS, an environment with the sun sampled and not, a black one, none,
and APT_FLAG_MIS next to either light mode.
tests/golden/make_restatement_hashes.py writes the file again from this case list, for the day the header's arithmetic changes on purpose.

Rays: the oracle's counter generator at 24 x 16, samples 2 (3072 paths), seed 7, eps 1e-4; every 12th of them (256 paths) in the
1030-sphere scenes, whose [paths][spheres] arrays are the slow ones.  Every case at depth 1 and 5 and at rr_start 0 and 2; the cases of
APT_FLAG_MIS, which is not read at depth 1, at depth 2 and 5, and their roughness edges (256 copies of mis_physics.mirror_ray) at depth 2."""
import hashlib
import json
import os

import numpy as np
import pytest

import lights_ref as lr
import materials_ref as mr
import mis_physics as mp
from gpu_harness import host, scene as harness_scene  # noqa: F401

W, H, S, SEED, EPS = 24, 16, 2, 7, 1e-4
VARIANTS = [(depth, rr) for depth in (1, 5) for rr in (0, 2)]
MIS_VARIANTS = [(depth, rr) for depth in (2, 5) for rr in (0, 2)]
MIS_ROOMS = ("gloss8-lamp", "gloss9-lamp", "open40")                          # gpu_harness's scenes, their own light and table
MIS_EDGES = (1, 19661, 65535)                                                 # the q of mis_physics.scene(q): the edges of the roughness
HASHES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "restatement_hashes.json")


def glossy(gd, mat, every):
    """tests/test_gpu_environment.py's gloss mix: every `every`-th mirror of a generated table becomes rough metal of its own roughness."""
    mat = np.array(mat, dtype=np.int32)
    for i in np.nonzero(mat == mr.SPEC)[0][::every]:
        mat[i] = gd.gloss((600 + (int(i) * 977) % 64000) / 65536.0)
    return mat


def scenes(gd):
    """name -> (spheres, materials, ns)."""
    room_mat = np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    out = {"demo9": (*gd.gen_spheres_materials(), 9), "room8": (gd.gen_spheres(), room_mat, 8)}
    word7 = room_mat.copy()
    word7[2] = 7                                                            # a wall with a material word that no launch accepts
    out["room8_word7"] = (gd.gen_spheres(), word7, 8)
    out["gen1030"] = lr.sixteen_lamps(gd)[:3]
    out["demo9_lamp"] = (gd.with_lamp(gd.gen_spheres_materials()[0], 9, 7), gd.gen_spheres_materials()[1], 9)
    out["demo9_two_lights"] = lr.demo_two_lights(gd)
    out["two_lamps"] = lr.two_lamps(gd)
    sph, mat, ns = lr.two_lamps(gd)
    mat = mat.copy()
    mat[6] = gd.gloss(0.3)
    out["two_lamps_gloss"] = (sph, mat, ns)
    sph, mat = gd.gen_spheres_open()
    out["open8"] = (gd.with_lamps(sph, 8, [5, 4], radius=8.0, emission=[(30.0, 20.0, 10.0), 12.0]), mat, 8)
    sph, mat = gd.gen_scene_open(40, seed=2)
    out["open40"] = (gd.with_lamps(sph, 40, [7, 19], radius=[1.5, 2.0], emission=[(40.0, 30.0, 20.0), 25.0]), glossy(gd, mat, 2), 40)
    return {k: (np.asarray(v[0], dtype=np.float32), np.asarray(v[1], dtype=np.int32), int(v[2])) for k, v in out.items()}


def mis_scenes(pkg):
    """name -> (spheres, materials, ns, light, the scene's own table) of the APT_FLAG_MIS cases."""
    out = {}
    for name in MIS_ROOMS:
        sc = harness_scene(pkg, name)
        out["harness/" + name] = (sc.sph, sc.mat, sc.ns, sc.light, sc.table)
    for q in MIS_EDGES:
        sph, mat = mp.scene(q)
        out["mirror/q%d" % q] = (sph, mat, 2, mp.LAMP, lr.build_table(sph, 2, [mp.LAMP]))
    return out


def _modes(light, lights):
    """plain / nee / table of one scene -> (suffix, arguments)."""
    return [("plain", {}), ("nee", dict(light=light, nee=True)), ("table", dict(lights=lights))]


def cases():
    """(name, owner: the module that traced the case before there was one, scene, arguments) -- arguments: light / nee / mis as trace()
    takes them (light "own": the scene's), lights: the spheres of a light table ("own": the scene's table), gloss (default False), env: None,
    "black", "sampled" or "plain" (environment())."""
    out = [("materials/" + s, "materials_ref", s, {}) for s in ("demo9", "room8", "gen1030", "room8_word7")]
    out += [("nee/on", "nee_ref", "demo9_lamp", dict(light=7, nee=True)), ("nee/off", "nee_ref", "demo9_lamp", dict(light=7, nee=False))]
    out += [("lights/demo9", "lights_ref", "demo9_two_lights", dict(lights=[7, 6])), ("lights/two_lamps", "lights_ref", "two_lamps", dict(lights=[7, 6])),
            ("lights/sixteen_lamps", "lights_ref", "gen1030", dict(lights=[6 + 61 * i for i in range(16)])),
            ("lights/one_light", "lights_ref", "demo9_lamp", dict(lights=[7]))]
    for mode, kw in _modes(7, [7, 6]):
        out.append(("gloss/" + mode, "gloss_ref", "two_lamps_gloss", dict(kw, gloss=True)))
        out.append(("gloss/%s_without_the_flag" % mode, "gloss_ref", "two_lamps_gloss", dict(kw, gloss=False)))   # the word is then bad
    for scene, light, lights in (("open8", 5, [5, 4]), ("open40", 7, [7, 19])):
        for mode, kw in _modes(light, lights):
            for env in ("sampled", "plain", "black", None):
                out.append(("env/%s_%s_%s" % (scene, mode, env or "none"), "env_ref", scene, dict(kw, gloss=True, env=env)))
    for mode, kw in _modes("own", "own")[1:]:
        for name in MIS_ROOMS:
            for env in (None, "sampled"):
                out.append(("mis/%s_%s_%s" % (name, mode, env or "none"), "mis_ref", "harness/" + name, dict(kw, gloss=True, mis=True, env=env)))
        for q in MIS_EDGES:
            out.append(("mis/mirror_q%d_%s" % (q, mode), "mis_ref", "mirror/q%d" % q, dict(kw, gloss=True, mis=True)))
    return out


def variants(case):
    """The (depth, rr_start) pairs of a case."""
    if case[1] != "mis_ref":
        return VARIANTS
    return [(2, 0)] if case[2].startswith("mirror/") else MIS_VARIANTS


def environment(gd, Env, what):
    """The case's `env` as an Env (the class is the caller's: the module that owns the case)."""
    if what is None:
        return None
    if what == "black":
        return Env()
    return Env.from_ctypes(gd.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(30.0, 28.0, 24.0),
                                          sun_angle_deg=8.0, sample_sun=what == "sampled"))


def rays_of(oracle, ns, mirror=None):
    """-> (rays [6][n], path indices [n]); mirror: the table of a mis_physics scene, for 256 copies of its mirror_ray."""
    if mirror is not None:
        return np.tile(mp.mirror_ray(mirror)[:, None], (1, 256)), np.arange(256, dtype=np.uint64)
    rays = oracle.gen_rays_counter(oracle.make_params(W, H, S, depth=5, seed=SEED))
    paths = np.arange(rays.shape[1], dtype=np.uint64)
    assert rays.shape[1] == 3072
    step = 12 if ns > 1000 else 1
    return np.ascontiguousarray(rays[:, ::step]), paths[::step]


def key(name, depth, rr):
    return "%s depth %d rr_start %d" % (name, depth, rr)


def digest(L, bad, segments):
    assert L.dtype == np.float32 and L.ndim == 2 and L.shape[0] == 3 and bad.dtype == np.bool_ and bad.shape == (L.shape[1],)
    return {"L": hashlib.sha256(np.ascontiguousarray(L).tobytes()).hexdigest(),
            "bad": hashlib.sha256(np.ascontiguousarray(bad).tobytes()).hexdigest(), "segments": int(segments)}


def dump(results):
    return json.dumps(results, indent=1, sort_keys=True) + "\n"


def restated(gd, oracle, world, case, depth, rr, **change):
    """The case (change: with these arguments changed) through tests/materials_ref.py -> its digest."""
    _, _, scene, kw = case
    sph, mat, ns, *own = world[scene]
    rays, paths = rays_of(oracle, ns, sph if scene.startswith("mirror/") else None)
    kw = dict(kw, **change)
    lights = kw.pop("lights", None)
    table = None if lights is None else (own[1] if lights == "own" else lr.build_table(sph, ns, lights))
    if kw.get("light") == "own":
        kw["light"] = own[0]
    env = environment(gd, mr.Env, kw.pop("env", None))
    return digest(*mr.trace(rays, sph, mat, ns, depth, EPS, SEED, paths, env=env, rr_start=rr, table=table, gloss=kw.pop("gloss", False), **kw))


@pytest.fixture(scope="module")
def gd(host):
    return host.gen_data


@pytest.fixture(scope="module")
def world(host):
    return {**scenes(host.gen_data), **mis_scenes(host)}


@pytest.fixture(scope="module")
def recorded():
    with open(HASHES) as f:
        return json.load(f)


def test_the_file_holds_the_case_list_and_nothing_else(recorded):
    names = [c[0] for c in cases()]
    assert len(set(names)) == len(names)
    assert sorted(recorded) == sorted(key(c[0], d, rr) for c in cases() for d, rr in variants(c))
    assert {c[1] for c in cases()} == {"materials_ref", "nee_ref", "lights_ref", "gloss_ref", "env_ref", "mis_ref"}


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_restatement_gives_the_recorded_bytes(gd, oracle, world, recorded, case):
    for depth, rr in variants(case):
        assert restated(gd, oracle, world, case, depth, rr) == recorded[key(case[0], depth, rr)], (case[0], depth, rr)
