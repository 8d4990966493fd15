"""GPU: the rough-metal material (include/render_mi355x.h GLOSS, APT_FLAG_GLOSS) through the C-ABI, bit for bit against the NumPy
restatement tests/materials_ref.py with the status word clean -- frames of every scene form, light mode and accumulation arm, a camera
with a lens, a pixel range; hand-made rays in buffer mode; the flag's rules -- and against the float64 expectation of
tests/gloss_physics.py (tests/golden/gloss_expectations.json), which shares no text with either.

Without the feature the bitwise frame, buffer and physics cases fail: a library that does not read APT_FLAG_GLOSS reports every gloss
word as APT_DEV_BAD_MATERIAL and ends the path there."""
import ctypes

import numpy as np
import pytest

import gloss_physics as gp
import lights_ref as lr
import materials_ref as mr
import physics_ref as ph
from gpu_harness import Scene, apt, assert_bits_equal, dev, same, scene  # noqa: F401

pytestmark = pytest.mark.gpu
MODES = ["plain", "nee", "table"]
W, H = 48, 32
# (samples, depth): samples 1, 3 and 8 are the GROUP == 1 arm, its longer leaf, and the GROUP == 8 arm
CASES = [(1, 1), (3, 5), (8, 8)]
BIG_CASES = [(1, 8), (3, 5), (8, 1)]     # 1030 spheres: the same sample counts and depths, paired so that the restatement stays quick


_scenes = {}


def _scene(apt, name):
    """gloss8: gen_spheres' 8 spheres with the mirror ball as a gloss ball (the SGPR form), the ball also a lamp; demo9: the demo scene
    with the gloss ball and the glass ball (one tile); big: 1030 generated spheres, every second mirror a gloss sphere of its own
    roughness (two LDS tiles, and the grid)."""
    if name not in _scenes:
        gd = apt.gen_data
        if name == "gloss8":
            sph, mat, ns = lr.two_lamps(gd)                                # spheres 6 and 7 are lamps
            mat = mat.copy()
            mat[6] = gd.gloss(0.3)
            _scenes[name] = Scene(apt, sph, mat, ns, [7, 6], 7)
        elif name == "demo9":
            sph, mat = gd.gen_spheres_materials(gloss=0.25)
            sph = np.array(sph, dtype=np.float32)
            sph[:90].reshape(10, 9)[4:7, 6] = [3.0, 6.0, 9.0]              # the gloss ball glows: the table's second light
            _scenes[name] = Scene(apt, sph, mat, 9, [7, 6], 7)
        else:
            sph, mat, ns, idx = lr.sixteen_lamps(gd)
            mat = np.array(mat, dtype=np.int32)
            mirrors = np.nonzero(mat == mr.SPEC)[0][::2]
            assert mirrors.size > 100
            for i in mirrors:
                mat[i] = mr.word(600 + (int(i) * 977) % 64000)
            _scenes[name] = Scene(apt, sph, mat, ns, [ns - 1, idx[5]], ns - 1, grid=True)
        assert _scenes[name].mat_flags == apt.APT_FLAG_GLOSS
    return _scenes[name]


FORMS = [("gloss8", False), ("demo9", False), ("big", False), ("big", True)]
FORM_IDS = ["8", "tiles9", "tiles1030", "grid1030"]


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rr", [False, True], ids=["", "rr"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_frames_equal_the_restatement(apt, name, grid, mode, rr):
    sc = _scene(apt, name)
    for s_, depth in (BIG_CASES if name == "big" else CASES):
        p = sc.params(W, H, s_, depth, mode=mode, rr=rr, seed=10 + s_, grid=grid)
        got = sc.frame(p, mode)
        same(got, sc.frame_ref(p, mode))
        assert got[0].max() > 0
        if grid:
            same(got, sc.frame(sc.params(W, H, s_, depth, mode=mode, rr=rr, seed=10 + s_), mode))     # the grid form is the tile form


def test_frame_with_a_camera_and_a_lens(apt):
    sc = _scene(apt, "gloss8")
    cam = apt.gen_data.camera(width=W, height=H, aperture=2.5, eye=(20.0, 60.0, 160.0), target=(27.0, 16.5, 47.0), up=(0.1, 1.0, 0.05),
                              vfov_deg=40.0, offset=0.0)
    for mode, (s_, depth) in zip(MODES, CASES[::-1]):
        p = sc.params(W, H, s_, depth, mode=mode, rr=True, seed=21)
        same(sc.frame(p, mode, cam), sc.frame_ref(p, mode, cam))


@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_a_pixel_range_without_the_byte_frame(apt, name, grid):
    """Pixels [517, 517 + 700) of the frame through the C entry itself with fb_u8 NULL."""
    import torch
    sc = _scene(apt, name)
    s_, depth = 8, (2 if name == "big" else 5)
    p = sc.params(W, H, s_, depth, seed=31, grid=grid)
    b, c = 517, 700
    fb = torch.full((3, c), -1.0, dtype=torch.float32, device="cuda")
    rc = apt._lib.lib().apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(sc.d_sph.data_ptr()), ctypes.c_void_p(sc.d_mat.data_ptr()),
                                                   ctypes.c_uint64(b), ctypes.c_uint64(c), ctypes.c_void_p(fb.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    apt.render.check_device_status()
    assert_bits_equal(fb.cpu().numpy(), sc.frame_ref(p, "plain")[0][:, b:b + c])


# ---- buffer mode ----------------------------------------------------------------------------------------------------------------------
def _hand_rays(sc):
    """1024 rays for sphere 6 of gen_spheres (the ball): 256 at normal incidence, 256 grazing at 0.999 of the radius, 256 from inside, and
    256 whose lanes alternate between a DIFF wall, a SPEC wall, a REFR wall and the GLOSS ball (the codes: _four_codes)."""
    planes = sc.sph[:10 * sc.ns].reshape(10, sc.ns).astype(np.float64)
    c, r = planes[1:4, 6], float(np.sqrt(planes[0, 6]))
    rng = np.random.default_rng(4)
    unit = lambda v: v / np.linalg.norm(v)
    out = []
    for _ in range(4):                                                     # normal incidence, 64 lanes each
        a = unit(rng.normal(size=3) + np.array([0.3, 1.0, 0.6]))          # from above and in front: inside the room
        out += [np.concatenate([c + 1.6 * r * a, -a])] * 64
    for _ in range(4):                                                     # grazing: impact parameter 0.999 r
        a = unit(rng.normal(size=3) + np.array([0.3, 1.0, 0.6]))
        side = unit(np.cross(a, rng.normal(size=3)))
        o = c + 1.6 * r * a
        sin_a = 0.999 * r / (1.6 * r)
        out += [np.concatenate([o, -np.sqrt(1.0 - sin_a * sin_a) * a + sin_a * side])] * 64
    for _ in range(256):                                                   # from inside the ball
        out.append(np.concatenate([c + 0.5 * r * rng.random() * unit(rng.normal(size=3)), unit(rng.normal(size=3))]))
    eye = np.array([50.0, 45.0, 110.0])
    targets = [np.array([1.0, 40.0, 80.0]), np.array([99.0, 40.0, 80.0]), np.array([50.0, 40.0, 0.5]), c]   # left, right, back wall, the ball
    for i in range(256):
        t = targets[i % 4] + (rng.normal(size=3) if i % 4 < 3 else 0.3 * r * unit(rng.normal(size=3)))
        out.append(np.concatenate([eye, unit(t - eye)]))
    return np.array(out, dtype=np.float64).T.astype(np.float32)


def _four_codes(apt, ns):
    """gen_spheres' table (ns 8) or the demo scene's (ns 9) with the left wall DIFF, the right wall SPEC, the back wall REFR and the
    ball GLOSS; sphere 7 is smallpt's lamp, the ball a second light."""
    gd = apt.gen_data
    if ns == 8:
        sph, mat = gd.gen_spheres(), np.array([1, 0, 2, 1, 1, 1, 0, 1], dtype=np.int32)
    else:
        sph, mat = gd.gen_spheres_materials()
        mat = np.array(mat, dtype=np.int32)
        mat[1], mat[2] = mr.SPEC, mr.REFR
    mat[6] = gd.gloss(0.4)
    sph = gd.with_lamp(sph, ns, 7)
    sph[:10 * ns].reshape(10, ns)[4:7, 6] = [1.0, 2.0, 3.0]
    return Scene(apt, sph, mat, ns, [7, 6], 7)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ns", [8, 9], ids=["8", "tiles9"])
def test_hand_made_rays_in_buffer_mode(apt, ns, mode):
    import torch
    sc = _four_codes(apt, ns)
    rays = _hand_rays(sc)
    n = rays.shape[1]
    paths = np.arange(n, dtype=np.uint64)
    geo = sc.sph[:10 * ns].reshape(10, ns)
    _, first = mr._intersect(list(rays[:3]), list(rays[3:]), (geo[1], geo[2], geo[3], geo[0]), np.float32(1e-4), np.full(n, -1))
    assert (first[:768] == 6).all()                                        # the three kinds aimed at the ball hit it first
    wave = first[768:832]
    assert sorted(set(wave.tolist())) == [0, 1, 2, 6] and (wave[3::4] == 6).all() and (wave[0::4] == 0).all()   # one wave, four codes
    p = sc.params(16, 16, 1, 6, mode=mode, rr=True, seed=9)
    assert p.num_paths == n
    kw = dict(light=7, nee=True) if mode == "nee" else (dict(table=sc.table) if mode == "table" else {})
    want, bad, _ = mr.trace(rays, sc.sph, sc.mat, ns, 6, 1e-4, 9, paths, rr_start=2, **kw)
    assert not bad.any()
    # some grazing lanes draw a direction below the horizon and end there: their colour is what the ball itself emits
    f32 = np.float32
    tmin, _ = mr._intersect(list(rays[:3]), list(rays[3:]), (geo[1], geo[2], geo[3], geo[0]), f32(1e-4), np.full(n, -1))
    nrm = [(rays[i] + rays[3 + i] * tmin) - geo[1 + i][6] for i in range(3)]
    ln = np.sqrt(mr.dot(*nrm, *nrm))
    u1, u2 = mr.uniforms(mr.mat_key(9, paths), 0)
    with np.errstate(all="ignore"):
        _, _, up = mr.gloss_sample(list(rays[3:]), [x / ln for x in nrm], np.full(n, (int(sc.mat[6]) >> 8) * 2.0 ** -16, f32), u1, u2)
    ended = ~up[256:512]
    assert 0 < ended.sum() < 256
    assert (want[:, 256:512][:, ended] == geo[4:7, 6][:, None]).all()
    d_rays = dev(rays.ravel())
    got = apt.render.render_paths(p, d_rays, sc.d_sph, materials=sc.d_mat, lights=sc.d_table if mode == "table" else None)
    torch.cuda.synchronize()
    apt.render.check_device_status()
    assert_bits_equal(got.cpu().numpy(), want)
    # a path range in band-relative buffers
    b, c = 300, 600
    pb = sc.params(16, 16, 1, 6, mode=mode, rr=True, seed=9, flags=apt.APT_FLAG_BAND_BUFFERS, path_begin=b, path_count=c)
    band = torch.full((3 * c,), -1.0, dtype=torch.float32, device="cuda")
    apt.render.render_do_ex(pb, None, dev(rays[:, b:b + c].ravel()), sc.d_sph, band, materials=sc.d_mat,
                            lights=sc.d_table if mode == "table" else None)
    torch.cuda.synchronize()
    apt.render.check_device_status()
    assert_bits_equal(band.cpu().numpy().reshape(3, c), want[:, b:b + c])


# ---- the flag -------------------------------------------------------------------------------------------------------------------------
def _bad_material(apt):
    with pytest.raises(apt.AptError) as e:
        apt.render.check_device_status()                                   # reads and clears the word
    assert "bad-material" in str(e.value)


@pytest.mark.parametrize("name", ["gloss8", "demo9"])
def test_gloss_words_need_the_flag_and_malformed_ones_are_bad(apt, name):
    sc = _scene(apt, name)
    apt.render.check_device_status()                                       # nothing pending
    for s_ in (1, 8):
        sc.frame(sc.params(16, 16, s_, 3, seed=1, gloss=0), "plain", check=False)      # well-formed words, no flag: as before the flag existed
        _bad_material(apt)
    for word in (3, mr.word(700) | (1 << 24), 4 | (700 << 8)):             # q == 0, bit 24, a low byte of 4
        mat = sc.mat.copy()
        mat[2] = word                                                      # the back wall: every frame hits it
        bad = Scene(apt, sc.sph, mat, sc.ns)                               # launched with the flags that sc's own words earn
        bad.frame(sc.params(16, 16, 8, 3, seed=1), "plain", check=False)
        _bad_material(apt)
        bad.frame(sc.params(16, 16, 8, 3, seed=1, gloss=0), "plain", check=False)
        _bad_material(apt)
    sc.frame(sc.params(16, 16, 8, 3, seed=1), "plain")                     # and the table as it is renders clean


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_the_flag_changes_nothing_without_gloss_words(apt, name, grid, mode):
    sc = scene(apt, {"gloss8": "room8", "demo9": "demo9x2", "big": "big1030x2"}[name])
    assert sc.mat_flags == 0
    for s_, depth in ((3, 5), (8, 3)):
        off = sc.frame(sc.params(W, H, s_, depth, mode=mode, rr=True, seed=5, grid=grid, gloss=0), mode)
        on = sc.frame(sc.params(W, H, s_, depth, mode=mode, rr=True, seed=5, grid=grid, gloss=apt.APT_FLAG_GLOSS), mode)
        same(on, off)
        assert off[0].max() > 0


# ---- physics --------------------------------------------------------------------------------------------------------------------------
LIGHT, TABLE_LIGHTS = 0, [0, 2]          # walls, as tests/test_gloss_cpu.py


class Physics:
    def __init__(self, apt):
        self.apt = apt
        self.rays = gp.copies(gp.rays())
        self.d_rays = dev(self.rays.ravel())
        self.paths = np.arange(8 * gp.COPIES, dtype=np.uint64)
        self.fixture, _ = gp.load_fixture()
        self.scenes, self.want, self.got = {}, {}, {}

    def scene(self, name, grid):
        if (name, grid) not in self.scenes:
            s = getattr(gp, name)()
            self.scenes[name, grid] = Scene(self.apt, s.table, s.materials, s.ns, TABLE_LIGHTS, LIGHT, grid=grid)
        return self.scenes[name, grid]

    def restated(self, name, mode, rr):
        if (name, mode, rr) not in self.want:
            sc = self.scene(name, False)
            kw = dict(light=LIGHT, nee=True) if mode == "nee" else (dict(table=sc.table) if mode == "table" else {})
            L, bad, _ = mr.trace(self.rays, sc.sph, sc.mat, sc.ns, gp.DEPTH, 1e-4, 1, self.paths, rr_start=1 if rr else 0, **kw)
            assert not bad.any()
            self.want[name, mode, rr] = L
        return self.want[name, mode, rr]

    def launch(self, name, grid, mode, rr):
        import torch
        if (name, grid, mode, rr) not in self.got:
            sc = self.scene(name, grid)
            p = sc.params(128, 128, 2, gp.DEPTH, mode=mode, rr=rr, seed=1, grid=grid)
            if rr:
                p.rr_start = 1                                             # roulette on the gloss bounce's own throughput
            assert p.num_paths == 8 * gp.COPIES and p.flags & self.apt.APT_FLAG_GLOSS
            colors = self.apt.render.render_paths(p, self.d_rays, sc.d_sph, materials=sc.d_mat, lights=sc.d_table if mode == "table" else None)
            torch.cuda.synchronize()
            self.apt.render.check_device_status()
            self.got[name, grid, mode, rr] = colors.cpu().numpy()
        return self.got[name, grid, mode, rr]


@pytest.fixture(scope="module")
def physics(apt):
    return Physics(apt)


@pytest.mark.parametrize("rr", [False, True], ids=["", "rr"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", [("gloss8", False), ("gloss9", False), ("gloss9", True)], ids=["gloss8", "gloss9-tiles", "gloss9-grid"])
def test_physics_and_restatement(physics, name, grid, mode, rr):
    got = physics.launch(name, grid, mode, rr)
    want, _ = physics.fixture[name]
    c, _ = gp.compare(got, want)
    print("%s%s %-5s%s  max |z| %.2f at %s over %d components, all-equal error %.2e at %s" % (
        name, " grid" if grid else "", mode, " rr" if rr else "", c["zmax"], c["z_at"], c["differing"], c["exact"], c["exact_at"]))
    assert c["finite"]
    assert c["zmax"] <= ph.Z_CAP and c["exact"] <= ph.EXACT_TOL
    assert c["differing"] >= 8
    assert_bits_equal(got, physics.restated(name, mode, rr))
    if grid:
        assert_bits_equal(got, physics.launch(name, False, mode, rr))
