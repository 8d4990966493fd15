"""Scenes that break intersection and light-sampling code, for the material renderer's tests (tests/test_degenerate_scenes_cpu.py on the
restatement alone, tests/test_gpu_degenerate_scenes.py on the kernels).  A plain module beside materials_ref.py, imported the same way.

Every scene keeps the reference room's six walls (gen_data.gen_spheres()), so it is closed and paths live to full depth, and comes with
4096 rays whose origins are uniform inside the room and which are aimed at a randomly chosen small sphere with a jitter of one radius --
half of them at the spheres the scene is about.  A ray component that is not finite (a target with a NaN or inf member) is replaced by
0.5: those rays have a direction that is not of unit length.  Everything is drawn from fixed seeds.

build(gen_data, name) -> Degenerate(sph, mat, ns, lights, light, rays, about):
  sph     the zero-padded [10][ns] table        mat    the material words           lights  the spheres the light table lists
  light   the light of APT_FLAG_NEE             rays   float32 [6][4096]            about   the spheres the scene is about

The many-sphere scenes have 6 walls + 90 small spheres (6 .. 95) + the stock light (96): LDS tiles without a grid, mat_hit_grid with one.
Sphere 60 is a second, small lamp of GLASS that overlaps its DIFF neighbour 61: a ray refracted into the lamp finds the part of the
neighbour that lies inside it, a shading point inside a light.

  twins      10 .. 19 share one record, codes cycling DIFF / SPEC / REFR with different albedos; 30 .. 33 share another, 32 an emitter
             (not the lowest of its group: hits and shadow segments end on 30); 40 .. 45 have radius 0; light_index the overlapping
             lamp 60, which can be hit here: a sample taken from inside it would drop its emission at the next hit
  nested     ten glass shells concentric around DIFF cores (10 .. 29: the shell's index above its core's, and below it, in turn); core
             10 is a lamp (seen through glass only) and itself of glass around a DIFF kernel, 32: three deep, and every shading point
             on the kernel lies inside the light; lamp 31, the light of APT_FLAG_NEE, inside a glass shell of its own radius, 30 (a
             lower-indexed twin: every hit and every shadow segment ends on the shell), around a DIFF kernel, 33; two overlapping
             glass spheres 34, 35; glass sphere 36 cut by the left wall; the table lists 60, 10 and 31, the stock light is unlisted
  values     members as the mirror renderer's grid test has them: a NaN and an inf centre, an inf and a NaN radius (10 .. 13);
             a radius of 0, aimed at exactly (14: a hit has h == c, so its normal and the path's next direction are NaN); the albedos
             (NaN, .5, .5), (-0.5, 2.5, 0) and 0 on DIFF spheres (20 .. 22), the first two on a mirror and on glass as well (23, 24);
             gloss words of the smallest and the largest roughness the encoding admits (25, 26)
  lights     listed light 21 whose unlisted twin 20 has the lower index; listed lights 30, 31, twins of each other and of radius 9, so that
             some rays start inside them and meet the same listed sphere twice in a row (the table's g != kprev); listed light 40 of
             radius 0 (apt_build_lights_host accepts it: its power is 0, so it keeps the uniform half of its probability); light_index
             the overlapping lamp 60, which here has a lower-indexed glass twin, 59
  cluster40  10 .. 49 share one record, mixed codes: one cell list above kGridSortInline = 32, which the device builder hands to the host
  tiles1030  gen_scene_materials(1030, seed=5) with 1023 and 1024, the last sphere of the first LDS tile and the first of the second,
             made twins of different material, in the middle of the room
  twins8     exactly 8 spheres (the SGPR form): floor and ceiling wall twins (4, 5: one packed pair; 4 DIFF, 5 a mirror), the ball a
             glass twin of the front wall (3, 6: across pairs); sphere 7 is the ceiling's record with an emission, so the room stays closed
  values8    exactly 8 spheres: the ball's centre NaN, the albedo (NaN, .5, .5) on the light (here a lamp of radius 5) and NOT on a wall,
             where the other two unusual albedos are (0 and 1): a wall with a NaN albedo turns more than half of the paths NaN, far
             above the 1 / 16 that the CPU test allows; the two gloss words on walls 3 and 4"""
import collections

import numpy as np

import materials_ref as mr

F = np.float32
N_RAYS = 4096
ROOM = ((1.0, 99.0), (0.0, 81.6), (0.0, 170.0))
MANY = ("twins", "nested", "values", "lights", "cluster40", "tiles1030")       # more than 8 spheres: tiles, and a grid
EIGHT = ("twins8", "values8")
NAMES = MANY + EIGHT
FINITE = tuple(n for n in NAMES if not n.startswith("values"))                 # every member, albedo and ray finite
LAMP, NEIGHBOUR = 60, 61
GLOSS_MIN, GLOSS_MAX = mr.word(1), mr.word(65535)
ALBEDOS = ((np.nan, 0.5, 0.5), (-0.5, 2.5, 0.0), (0.0, 0.0, 0.0))

Degenerate = collections.namedtuple("Degenerate", "sph mat ns lights light rays about")


def _pad(tab):
    flat = np.ascontiguousarray(tab, dtype=F).ravel()
    return np.concatenate([flat, np.zeros((-flat.size) % 128, dtype=F)])


def _record(tab, k, radius=None, centre=None, emission=None, albedo=None):
    if radius is not None:
        tab[0, k] = F(np.float64(radius) ** 2)
    if centre is not None:
        tab[1:4, k] = centre
    if emission is not None:
        tab[4:7, k] = emission
    if albedo is not None:
        tab[7:10, k] = albedo


def _twin(tab, of, k):
    """Sphere k gets sphere `of`'s record -- radius and centre; emission and albedo stay its own."""
    tab[0:4, k] = tab[0:4, of]


def _clutter(gen_data, seed):
    """The 97-sphere base: walls, 90 small spheres of random place, size, albedo and code, the stock light; the glass lamp and its neighbour."""
    room = np.asarray(gen_data.gen_spheres(), dtype=F)[:80].reshape(10, 8)
    rng = np.random.RandomState(seed)
    ns = 97
    tab = np.zeros((10, ns), dtype=F)
    tab[:, :6], tab[:, 96] = room[:, :6], room[:, 7]
    small = slice(6, 96)
    tab[1, small] = rng.uniform(12, 88, 90)
    tab[2, small] = rng.uniform(8, 72, 90)
    tab[3, small] = rng.uniform(15, 150, 90)
    tab[0, small] = rng.uniform(2.0, 5.0, 90) ** 2
    tab[7:10, small] = rng.uniform(0.3, 0.9, (3, 90))
    mat = np.full(ns, mr.DIFF, dtype=np.int32)
    mat[small] = rng.choice([mr.DIFF, mr.DIFF, mr.SPEC, mr.REFR], 90)
    _record(tab, LAMP, 3.5, (50.0, 40.0, 90.0), (40.0, 30.0, 20.0), (0.9, 0.9, 0.9))
    _record(tab, NEIGHBOUR, 4.0, (54.0, 40.0, 90.0), albedo=(0.7, 0.6, 0.5))
    mat[LAMP], mat[NEIGHBOUR] = mr.REFR, mr.DIFF
    return tab, mat, rng


def aimed_rays(tab, about, small, rng, n=N_RAYS, floor=0.5):
    """Origins uniform in the room, each ray aimed at one of `about` (the first half) or `small` (the second) with a jitter of one radius,
    of `floor` at least: with floor = 0 a sphere of radius 0 is aimed at exactly, and a hit on it has no normal."""
    about, small = np.asarray(about), np.asarray(small)
    k = np.concatenate([about[rng.randint(0, about.size, n // 2)], small[rng.randint(0, small.size, n - n // 2)]])
    o = np.stack([rng.uniform(lo, hi, n) for lo, hi in ROOM])
    jitter = rng.normal(0.0, 1.0, (3, n))
    with np.errstate(all="ignore"):
        t = tab.astype(np.float64)
        tgt = t[1:4, k] + jitter * np.maximum(np.sqrt(t[0, k]), floor) - o
        d = tgt / np.linalg.norm(tgt, axis=0)
        rays = np.concatenate([o, d]).astype(F)
    return np.where(np.isfinite(rays), rays, F(0.5))


def _room_points(rng, n):
    """For the 8-sphere scenes, which have no small sphere to aim at: targets uniform in the room, as one-point 'spheres'."""
    t = np.zeros((10, n), dtype=F)
    t[1:4] = np.stack([rng.uniform(lo, hi, n) for lo, hi in ROOM])
    return t


def build(gen_data, name):
    if name in EIGHT:
        return _build8(gen_data, name)
    if name == "tiles1030":
        sph, mat = gen_data.gen_scene_materials(1030, seed=5)
        ns = 1030
        tab = np.array(sph, dtype=F)[:10 * ns].reshape(10, ns)
        mat = np.array(mat, dtype=np.int32)
        _record(tab, 1023, 4.0, (50.0, 40.0, 85.0), albedo=(0.8, 0.3, 0.2))
        _twin(tab, 1023, 1024)
        tab[7:10, 1024] = (0.2, 0.4, 0.9)
        mat[1023], mat[1024] = mr.DIFF, mr.SPEC
        about = [1023, 1024]
        rays = aimed_rays(tab, about, np.arange(6, ns - 1), np.random.RandomState(1030))
        return Degenerate(_pad(tab), mat, ns, [ns - 1], ns - 1, rays, about)
    seed = {"twins": 11, "nested": 12, "values": 13, "lights": 14, "cluster40": 15}[name]
    tab, mat, rng = _clutter(gen_data, seed)
    ns, lights, light = 97, [96, LAMP], 96
    cycle = (mr.DIFF, mr.SPEC, mr.REFR)
    if name == "twins":
        _record(tab, 10, 4.0, (30.0, 30.0, 60.0))
        for k in range(11, 20):
            _twin(tab, 10, k)
        mat[10:20] = [cycle[i % 3] for i in range(10)]
        _record(tab, 30, 3.5, (70.0, 45.0, 100.0))
        for k in (31, 32, 33):
            _twin(tab, 30, k)
        mat[30:34] = (mr.DIFF, mr.SPEC, mr.DIFF, mr.REFR)
        _record(tab, 32, emission=(25.0, 15.0, 8.0))
        tab[0, 40:46] = 0.0
        lights, light, about = [96, LAMP, 32], LAMP, list(range(10, 20)) + [30, 31, 32, 33, LAMP, NEIGHBOUR] + list(range(40, 46))
    elif name == "nested":
        for i in range(10):
            core, shell = (10 + 2 * i, 11 + 2 * i) if i % 2 == 0 else (11 + 2 * i, 10 + 2 * i)
            tab[1:4, shell] = tab[1:4, core]
            tab[0, core], tab[0, shell] = F(2.5 ** 2), F(4.5 ** 2)
            mat[core], mat[shell] = mr.DIFF, mr.REFR
            tab[7:10, shell] = 0.95
        _record(tab, 10, emission=(60.0, 50.0, 40.0), albedo=(0.9, 0.9, 0.9))   # the lamp: glass too, around a DIFF kernel
        mat[10] = mr.REFR
        _record(tab, 32, 1.2, tab[1:4, 10].copy(), albedo=(0.8, 0.7, 0.6))
        mat[32] = mr.DIFF
        _record(tab, 31, 3.0, (65.0, 30.0, 70.0), (30.0, 40.0, 50.0), (0.0, 0.0, 0.0))
        _twin(tab, 31, 30)
        mat[30], mat[31] = mr.REFR, mr.DIFF
        tab[7:10, 30] = 0.95
        _record(tab, 33, 1.2, tab[1:4, 31].copy(), albedo=(0.6, 0.7, 0.8))     # a DIFF kernel inside this lamp as well
        mat[33] = mr.DIFF
        _record(tab, 34, 5.0, (35.0, 20.0, 50.0), albedo=(0.9, 0.95, 0.9))
        _record(tab, 35, 5.0, (40.0, 21.0, 51.0), albedo=(0.95, 0.9, 0.9))
        _record(tab, 36, 8.0, (3.0, 30.0, 80.0), albedo=(0.9, 0.9, 0.95))
        mat[34:37] = mr.REFR
        lights, light, about = [LAMP, 10, 31], 31, list(range(10, 34)) + [32, 32, 33, 33, 34, 35, 36, LAMP, NEIGHBOUR]
    elif name == "values":
        tab[1, 10], tab[2, 11], tab[0, 12], tab[0, 13], tab[0, 14] = np.nan, np.inf, np.inf, np.nan, 0.0
        for k, a in zip((20, 21, 22, 23, 24), ALBEDOS + ALBEDOS[:2]):
            _record(tab, k, 4.5, albedo=a)
        mat[20:25] = (mr.DIFF, mr.DIFF, mr.DIFF, mr.SPEC, mr.REFR)
        tab[0, 25:27] = F(4.5 ** 2)
        mat[25], mat[26] = GLOSS_MIN, GLOSS_MAX
        about = list(range(10, 15)) + list(range(20, 27)) + [LAMP, NEIGHBOUR]
    elif name == "lights":
        _record(tab, 21, 3.0, (30.0, 50.0, 70.0), (20.0, 30.0, 40.0), (0.5, 0.5, 0.5))
        _twin(tab, 21, 20)
        _record(tab, 30, 9.0, (70.0, 25.0, 110.0), (35.0, 25.0, 15.0), (0.6, 0.6, 0.6))
        _twin(tab, 30, 31)
        _record(tab, 31, emission=(10.0, 20.0, 45.0))
        _record(tab, 40, 0.0, emission=(10.0, 10.0, 10.0))
        mat[[20, 21, 30, 31, 40]] = mr.DIFF
        _twin(tab, LAMP, LAMP - 1)                             # the light of APT_FLAG_NEE has a lower-indexed twin too, of glass like itself
        mat[LAMP - 1] = mr.REFR
        tab[7:10, LAMP - 1] = 0.9
        lights, light, about = [96, LAMP, 21, 30, 31, 40], LAMP, [20, 21, 30, 31, 40, LAMP - 1, LAMP, NEIGHBOUR]
    else:
        assert name == "cluster40"
        _record(tab, 10, 4.0, (50.0, 35.0, 80.0))
        for k in range(11, 50):
            _twin(tab, 10, k)
        mat[10:50] = [cycle[(i * 7 + i // 3) % 3] for i in range(40)]
        about = list(range(10, 50)) + [LAMP, NEIGHBOUR]
    rays = aimed_rays(tab, about, np.arange(6, 96), rng, floor=0.0 if name == "values" else 0.5)
    return Degenerate(_pad(tab), mat, ns, lights, light, rays, about)


def _build8(gen_data, name):
    tab = np.array(gen_data.gen_spheres(), dtype=F)[:80].reshape(10, 8).copy()
    mat = np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    rng = np.random.RandomState({"twins8": 21, "values8": 22}[name])
    if name == "twins8":
        tab[0:4, 7] = tab[0:4, 5]                              # the ceiling's record, emitting: it closes the room in the ceiling's place
        tab[4:7, 7], tab[7:10, 7] = (2.0, 1.5, 1.0), (0.4, 0.4, 0.4)
        _twin(tab, 4, 5)                                       # floor and ceiling wall: one packed pair
        _twin(tab, 3, 6)                                       # front wall and ball: across pairs
        tab[7:10, 3] = (0.6, 0.5, 0.4)
        mat[4], mat[5], mat[3], mat[6] = mr.DIFF, mr.SPEC, mr.DIFF, mr.REFR
        about = [3, 4, 5, 6]
        pts = _room_points(rng, 64)
        pts[2, :32], pts[3, 32:] = 0.0, 170.0                  # on the floor and on the front wall: where the twins are
    else:
        tab[1, 6] = np.nan
        _record(tab, 7, 5.0, (50.0, 60.0, 81.6), (60.0, 60.0, 60.0))   # a lamp below the ceiling in the light's place
        for k, a in zip((7, 0, 1), ALBEDOS):                   # the NaN on the lamp, which few paths meet: on a whole wall it would
            tab[7:10, k] = a                                   # turn most of the image NaN
        tab[7:10, 3] = (0.7, 0.7, 0.7)
        mat[3], mat[4] = GLOSS_MIN, GLOSS_MAX
        about = [0, 1, 3, 4, 6]
        pts = _room_points(rng, 64)
        pts[1, :32] = rng.choice([1.0, 99.0], 32)              # on the left and right wall
        pts[3, 32:48], pts[2, 48:] = 0.0, 0.0                  # on the back wall and on the floor
    both = np.concatenate([tab, pts], axis=1)
    small = np.arange(8, 8 + 64) if name == "twins8" else np.array([6] + list(range(8, 8 + 64, 4)))   # values8: the NaN-centred ball too
    rays = aimed_rays(both, np.arange(8, 8 + 64), small, rng)
    return Degenerate(_pad(tab), mat, 8, [7], 7, rays, about)
