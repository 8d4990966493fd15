"""GPU: the environment (include/render_mi355x.h "environment": a sky and a sampled sun for the material renderer) through the C-ABI.

  frames    bit for bit against the NumPy restatement tests/materials_ref.py with the status word clean and the trace counter equal to the
            restatement's count of segments (the lights' and the sun's shadow segments included): the three scene forms -- the open
            8-sphere scene (SGPRs), 40 open spheres (LDS tiles), 220 open spheres behind the grid with grid image == tile image -- x
            {plain, APT_FLAG_NEE, a light table} x {sun sampled, not}, each over samples 1 / 4 / 8 / 9 (both groups and the n % 8
            tail), depth 1 / 2 / 5, no camera / a thin-lens camera, a gloss table / a gloss-free one; roulette once per form; one
            mid-image pixel range with fb_u8 NULL.
  black     an environment without light on the closed-room scenes renders the image of the launch without an environment, bit for
            bit, in all three forms with no camera and a gloss-free table: the environment kernels are always the general-camera,
            gloss instantiations, and this is what ties them to the kernels they stand in for.
  physics   the rays of tests/env_physics.py (float64 expectations from geometry alone) through render_paths in all three forms:
            the expectations hold, and the same buffers equal the restatement bit for bit.
  grid      a grid that is not the scene's still writes nothing and reports APT_DEV_GRID_MISMATCH.

On the parent every test here fails: the entries do not exist."""
import ctypes

import numpy as np
import pytest

import env_physics as ep
import materials_ref as mr
from gpu_harness import Scene, apt, assert_bits_equal, dev, lens, same, scene, sky_and_sun  # noqa: F401

pytestmark = pytest.mark.gpu
MODES = ["plain", "nee", "table"]
W, H = 64, 32
# (samples, depth, camera, gloss table): every sample count and depth, both cameras and both tables meet every form, mode and sun rule
LAUNCHES = [(1, 5, False, True), (4, 2, True, False), (8, 5, True, True), (9, 1, False, False)]


def _scene(apt, name):
    """The catalogue's open scenes: open8 (SGPRs), open40 (one LDS tile), open220 (its grid; four tiles without it)."""
    sc = scene(apt, name)
    assert sc.mat_flags == apt.APT_FLAG_GLOSS
    return sc


FORMS = [("open8", False), ("open40", False), ("open220", True)]
FORM_IDS = ["8", "tiles40", "grid220"]


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [True, False], ids=["sun-sampled", "sun-plain"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_frames_equal_the_restatement(apt, name, grid, mode, sample):
    sc = _scene(apt, name)
    env = sky_and_sun(apt, sample)
    assert bool(env.flags & apt.APT_ENV_SAMPLE_SUN) == sample
    for s_, depth, with_lens, gloss in LAUNCHES:
        cam = lens(apt, W, H) if with_lens else None
        p = sc.params(W, H, s_, depth, mode=mode, seed=10 + s_, grid=grid, gloss=gloss)
        got = sc.frame(p, mode, cam, env, gloss, count=True)
        same(got, sc.frame_ref(p, mode, cam, env, gloss))
        assert got[0].max() > 0
        if grid:                                                             # the grid form is the tile form
            same(got, sc.frame(sc.params(W, H, s_, depth, mode=mode, seed=10 + s_, gloss=gloss), mode, cam, env, gloss, count=True))


@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_frames_with_roulette(apt, name, grid):
    sc = _scene(apt, name)
    env = sky_and_sun(apt, True)
    for mode, (s_, depth) in zip(MODES, [(8, 5), (4, 5), (9, 5)]):
        p = sc.params(W, H, s_, depth, mode=mode, rr=True, seed=21, grid=grid)
        same(sc.frame(p, mode, env=env, count=True), sc.frame_ref(p, mode, env=env))


def test_the_sun_sample_changes_the_image_by_noise_only_and_depth_one_by_nothing(apt):
    sc = _scene(apt, "open8")
    on, off = sky_and_sun(apt, True), sky_and_sun(apt, False)
    p = sc.params(W, H, 8, 1, seed=5)
    assert_bits_equal(sc.frame(p, env=on)[0], sc.frame(p, env=off)[0])
    p = sc.params(W, H, 9, 3, seed=5)
    a, b = sc.frame(p, env=on, count=True), sc.frame(p, env=off, count=True)
    assert not np.array_equal(a[0], b[0]) and a[2] > b[2]                   # another estimate, and its shadow segments are counted
    assert abs(a[0].mean() - b[0].mean()) < 0.02 * b[0].mean()


@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_a_pixel_range_without_the_byte_frame(apt, name, grid):
    """Pixels [517, 517 + 700) of the frame through the C entries themselves with fb_u8 NULL."""
    import torch
    sc = _scene(apt, name)
    env = sky_and_sun(apt, True)
    L = apt._lib.lib()
    b, c = 517, 700
    for mode in ("plain", "table"):
        p = sc.params(W, H, 8, 3, mode=mode, seed=31, grid=grid)
        fb = torch.full((3, c), -1.0, dtype=torch.float32, device="cuda")
        args = (ctypes.byref(p), None, ctypes.c_void_p(sc.d_sph.data_ptr()), ctypes.c_void_p(sc.d_mat.data_ptr()))
        tail = (ctypes.c_uint64(b), ctypes.c_uint64(c), ctypes.c_void_p(fb.data_ptr()), None)
        apt.render.set_environment(env)
        try:
            rc = L.apt_render_frame_lights(*args, ctypes.c_void_p(sc.d_table.data_ptr()), *tail) if mode == "table" else L.apt_render_frame_materials(*args, *tail)
            torch.cuda.synchronize()
        finally:
            apt.render.set_environment(None)
        assert rc == 0
        apt.render.check_device_status()
        assert_bits_equal(fb.cpu().numpy(), sc.frame_ref(p, mode, env=env)[0][:, b:b + c])


def test_a_context_of_its_own_carries_the_environment(apt):
    """Context.set_environment: that context's launches gather the environment, the default context's do not."""
    import torch
    sc = _scene(apt, "open8")
    env = sky_and_sun(apt, True)
    p = sc.params(W, H, 4, 3, seed=8)
    ctx = apt.render.Context()
    try:
        ctx.set_environment(env)
        fb, u8 = ctx.render_frame(p, sc.d_sph, materials=sc.d_mat)
        dark, _ = apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat)
        torch.cuda.synchronize()
        ctx.check()
        want = sc.frame_ref(p, env=env)
        assert_bits_equal(fb.cpu().numpy(), want[0])
        assert np.array_equal(u8.cpu().numpy(), want[1])
        assert_bits_equal(dark.cpu().numpy(), sc.frame_ref(p)[0])
        with pytest.raises(apt.AptError, match="environment"):
            ctx.render_frame(p, sc.d_sph)                                    # its mirror frame entry refuses
    finally:
        ctx.close()


def test_gloss_words_need_the_flag_with_an_environment_too(apt):
    """The environment kernels are the gloss instantiations, but APT_FLAG_GLOSS is still the caller's to give: without it a gloss word is
    the bad code it is without an environment."""
    import torch
    sc = _scene(apt, "open8")
    env = sky_and_sun(apt, True)
    apt.render.check_device_status()                                         # nothing pending
    for s_ in (1, 8):
        p = sc.params(W, H, s_, 3, seed=1)
        p.flags &= ~apt.APT_FLAG_GLOSS
        apt.render.set_environment(env)
        try:
            apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat)
            torch.cuda.synchronize()
        finally:
            apt.render.set_environment(None)
        with pytest.raises(apt.AptError, match="bad-material"):
            apt.render.check_device_status()                                 # reads and clears the word
    p = sc.params(W, H, 8, 3, seed=1)
    same(sc.frame(p, env=env, count=True), sc.frame_ref(p, env=env))          # and with the flag the table renders clean


# ---- a black environment is no environment ----------------------------------------------------------------------------------------------
_closed_scenes = {}


def _closed(apt, name):
    if name not in _closed_scenes:
        gd = apt.gen_data
        if name != "room300":
            sc = scene(apt, "room8" if name == "room8" else "demo9x2")
        else:
            ns = 300                                                         # gen_scene's closed room: five tiles, or the grid
            sph, mat = gd.gen_scene_materials(ns, seed=5)
            sph = gd.with_lamps(sph, ns, [50], radius=[1.2], emission=[(60.0, 30.0, 15.0)])
            sc = Scene(apt, sph, mat, ns, [ns - 1, 50], ns - 1, grid=True)
        assert sc.mat_flags == 0                                           # gloss-free
        _closed_scenes[name] = sc
    return _closed_scenes[name]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", [("room8", False), ("demo9", False), ("room300", True)], ids=["8", "tiles9", "grid300"])
def test_a_black_environment_renders_the_image_without_one(apt, name, grid, mode):
    sc = _closed(apt, name)
    black = apt.gen_data.environment()
    assert black.sun_omc == 0 and not any(black.horizon) and not any(black.zenith)
    for s_, depth, rr in ((1, 5, False), (8, 5, True), (9, 3, False)):
        p = sc.params(W, H, s_, depth, mode=mode, rr=rr, seed=40 + s_, grid=grid)
        with_env, without = sc.frame(p, mode, env=black, count=True), sc.frame(p, mode, count=True)
        same(with_env, without)
        assert without[0].max() > 0


# ---- physics --------------------------------------------------------------------------------------------------------------------------
PHYS_FORMS = [(8, False), (9, False), (9, True)]
PHYS_IDS = ["8", "tiles9", "grid9"]
PHYS_CASES = [ep.uniform_sky(1), ep.uniform_sky(2), ep.uniform_sky(5), ep.gradient_sky(), ep.sun_only(False), ep.sun_only(True), ep.sun_only(True, 5),
              ep.occluder(), ep.mirror_ball(False), ep.mirror_ball(True)]


class Physics:
    def __init__(self, apt):
        self.apt, self.scenes, self.want, self.got = apt, {}, {}, {}

    def scene(self, case, ns, grid):
        key = (case.name, ns, grid)
        if key not in self.scenes:
            sph = case.table(ns)
            lights = case.lights if case.lights is not None else [0]       # a table needs an entry; only sun_and_lamp renders with it
            self.scenes[key] = (Scene(self.apt, sph, case.materials(ns), ns, lights, case.light, grid=grid), dev(case.rays().ravel()))
        return self.scenes[key]

    def env(self, case):
        e = case.env
        rec = self.apt._lib.ApEnvironment()
        rec.struct_size = ctypes.sizeof(rec)
        d3 = ctypes.c_double * 3
        self.apt._lib.check(self.apt._lib.lib().apt_environment_build_host(d3(*e["horizon"]), d3(*e["zenith"]), d3(*e["sun_dir"]), d3(*e["sun_radiance"]),
                                                                           ctypes.c_double(e["sun_omc"]), ctypes.c_uint32(e.get("flags", 0)),
                                                                           ctypes.byref(rec)), "apt_environment_build_host")
        return rec

    def restated(self, case, ns, mode):
        key = (case.name, ns, mode)
        if key not in self.want:
            sc, _ = self.scene(case, ns, False)
            kw = dict(light=case.light, nee=True) if mode == "nee" else (dict(table=sc.table) if mode == "table" else {})
            L, bad, _ = mr.trace(case.rays(), sc.sph, sc.plain, ns, case.depth, 1e-4, ep.SEED, case.paths(), mr.Env.from_ctypes(self.env(case)),
                                 gloss=False, **kw)
            assert not bad.any()
            self.want[key] = L
        return self.want[key]

    def launch(self, case, ns, grid, mode):
        import torch
        key = (case.name, ns, grid, mode)
        if key not in self.got:
            sc, d_rays = self.scene(case, ns, grid)
            w, h, s_ = case.frame_shape()
            p = sc.params(w, h, s_, case.depth, mode=mode, seed=ep.SEED, grid=grid, gloss=False)
            assert p.num_paths == case.nrays * ep.COPIES
            self.apt.render.set_environment(self.env(case))
            try:
                colors = self.apt.render.render_paths(p, d_rays, sc.d_sph, materials=sc.d_plain, lights=sc.d_table if mode == "table" else None)
                torch.cuda.synchronize()
            finally:
                self.apt.render.set_environment(None)
            self.apt.render.check_device_status()
            self.got[key] = colors.cpu().numpy()
        return self.got[key]


@pytest.fixture(scope="module")
def physics(apt):
    return Physics(apt)


def _check(case, L, label):
    c = ep.compare(L, case.want, case.exact)
    print("%-22s %-12s max |z| %.2f over %d differing components, all-equal error %.2e" % (case.name, label, c["zmax"], c["differing"], c["exact"]))
    assert ep.passes(c, case.exact), c


@pytest.mark.parametrize("case", PHYS_CASES, ids=[c.name for c in PHYS_CASES])
@pytest.mark.parametrize("ns,grid", PHYS_FORMS, ids=PHYS_IDS)
def test_physics_and_restatement(physics, ns, grid, case):
    got = physics.launch(case, ns, grid, "plain")
    _check(case, got, "grid" if grid else str(ns))
    assert_bits_equal(got, physics.restated(case, ns, "plain"))


@pytest.mark.parametrize("ns,grid", PHYS_FORMS, ids=PHYS_IDS)
def test_physics_a_glass_ball_between_the_point_and_the_sun(physics, ns, grid):
    on, off = ep.glass_ball(True), ep.glass_ball(False)
    Lon, Loff = physics.launch(on, ns, grid, "plain"), physics.launch(off, ns, grid, "plain")
    m1, s1, same1 = ep.summarise(Lon)
    m0, s0, same0 = ep.summarise(Loff)
    assert not same1.any() and not same0.any() and (m0 > 0.01).all()
    z = np.abs(m1 - m0) / np.sqrt((s1 * s1 + s0 * s0) / ep.COPIES)
    assert z.max() <= ep.Z_CAP
    assert_bits_equal(Lon, physics.restated(on, ns, "plain"))
    assert_bits_equal(Loff, physics.restated(off, ns, "plain"))


@pytest.mark.parametrize("sample", [True, False], ids=["sun-sampled", "sun-plain"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ns,grid", PHYS_FORMS, ids=PHYS_IDS)
def test_physics_the_sun_next_to_a_sphere_lamp(physics, ns, grid, mode, sample):
    case = ep.sun_and_lamp(sample)
    case.name += "_on" if sample else "_off"
    got = physics.launch(case, ns, grid, mode)
    _check(case, got, mode)
    assert_bits_equal(got, physics.restated(case, ns, mode))


# ---- the grid's promise ------------------------------------------------------------------------------------------------------------------
def test_a_grid_that_is_not_the_scenes_writes_nothing(apt):
    import torch
    sc = _scene(apt, "open220")
    other = apt.gen_data.build_grid(apt.gen_data.gen_scene_open(100, seed=9)[0], 100)
    d_other = torch.from_numpy(other.view(np.int32)).cuda()
    env = sky_and_sun(apt, True)
    apt.render.check_device_status()                                         # nothing pending
    for s_ in (1, 8):
        p = sc.params(W, H, s_, 3, seed=2, flags=apt.APT_FLAG_GRID_SLOTS)
        p.accel = d_other.data_ptr()
        fb = torch.full((3, W * H), -2.0, dtype=torch.float32, device="cuda")
        apt.render.set_environment(env)
        try:
            apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat, fb=fb)
            torch.cuda.synchronize()
        finally:
            apt.render.set_environment(None)
        assert (fb.cpu().numpy() == -2.0).all()
        with pytest.raises(apt.AptError, match="grid-mismatch"):
            apt.render.check_device_status()                                 # reads and clears the word
    rays = dev(np.zeros(6 * W * H * 4, dtype=np.float32))
    colors = torch.full((3 * W * H * 4,), -2.0, dtype=torch.float32, device="cuda")
    p = sc.params(W, H, 1, 3, seed=2, flags=apt.APT_FLAG_GRID_SLOTS)
    p.accel = d_other.data_ptr()
    apt.render.set_environment(env)
    try:
        apt.render.render_do_ex(p, None, rays, sc.d_sph, colors, materials=sc.d_mat)
        torch.cuda.synchronize()
    finally:
        apt.render.set_environment(None)
    assert (colors.cpu().numpy() == -2.0).all()
    with pytest.raises(apt.AptError, match="grid-mismatch"):
        apt.render.check_device_status()
