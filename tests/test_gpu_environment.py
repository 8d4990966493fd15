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

import camera_ref as cr
import env_physics as ep
import materials_ref as mr

pytestmark = pytest.mark.gpu
MODES = ["plain", "nee", "table"]
W, H = 64, 32
# (samples, depth, camera, gloss table): every sample count and depth, both cameras and both tables meet every form, mode and sun rule
LAUNCHES = [(1, 5, False, True), (4, 2, True, False), (8, 5, True, True), (9, 1, False, False)]


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def _dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


class Scene:
    """A scene on the device: the sphere table, its material words with and without gloss words, a two-light table, the light of
    APT_FLAG_NEE; grid=True builds a grid."""

    def __init__(self, apt, sph, mat, ns, lights, light, grid=False):
        import torch
        self.apt, self.sph, self.ns, self.light = apt, np.asarray(sph, dtype=np.float32), int(ns), light
        self.mat = {True: np.asarray(mat, dtype=np.int32)}
        plain = self.mat[True].copy()
        plain[(plain & 0xFF) == 3] = mr.SPEC                                # the gloss-free table: those spheres are mirrors
        self.mat[False] = plain
        self.d_sph = _dev(self.sph)
        self.d_mat = {k: _dev(v) for k, v in self.mat.items()}
        self.table = apt.gen_data.build_lights(self.sph, ns, lights)
        self.d_table = _dev(self.table.view(np.int32))
        self.flags = {k: apt.gen_data.materials_flags(v) for k, v in self.mat.items()}
        assert self.flags[False] == 0
        self.grid, self.grid_flags = None, 0
        if grid:
            hgrid = apt.gen_data.build_grid(self.sph, self.ns)
            self.grid = torch.from_numpy(hgrid.view(np.int32)).cuda()
            self.grid_flags = apt.gen_data.grid_flags(hgrid, self.ns)
            assert self.grid_flags == apt.APT_FLAG_GRID_SLOTS
        self.ref = {}

    def params(self, w, h, s_, depth, mode="plain", rr=False, seed=3, grid=False, gloss=True, **kw):
        apt = self.apt
        use_grid = grid and self.grid is not None
        flags = kw.pop("flags", 0) | (apt.APT_FLAG_NEE if mode == "nee" else 0) | (apt.APT_FLAG_RR if rr else 0)
        flags |= (self.grid_flags if use_grid else 0) | self.flags[gloss]
        return apt.make_params(w, h, s_, depth=depth, num_spheres=self.ns, light_index=self.light, seed=seed, flags=flags,
                               rr_start=2 if rr else 0, accel=self.grid.data_ptr() if use_grid else 0, **kw)

    def frame(self, p, mode, env, cam=None, gloss=True, count=True):
        """One launch through the default context -> (fb, u8, segments traced); the status word is clean after it."""
        import torch
        apt = self.apt
        apt.render.set_camera(cam)
        apt.render.set_environment(env)
        try:
            with apt.render.TraceCounter() as tc:
                fb, u8 = apt.render.render_frame(p, self.d_sph, materials=self.d_mat[gloss], lights=self.d_table if mode == "table" else None)
                torch.cuda.synchronize()
            traced = tc.value
        finally:
            apt.render.set_camera(None)
            apt.render.set_environment(None)
        apt.render.check_device_status()
        return fb.cpu().numpy(), u8.cpu().numpy(), traced

    def frame_ref(self, p, mode, env, gloss=True, rays=None):
        """materials_ref's frame for the launch `p` and the record `env` (the grid changes no image: it is not part of the key)."""
        key = (p.width, p.height, p.samples, p.depth, p.seed, mode, p.flags & (2 | 32 | 64), p.rr_start, rays is not None, gloss,
               None if env is None else bytes(env))
        if key not in self.ref:
            from oracle import oracle
            fb, u8, bad, seg = mr.render_frame(oracle.Params.from_buffer_copy(bytes(p)), self.sph, self.mat[gloss],
                                               env=None if env is None else mr.Env.from_ctypes(env),
                                               table=self.table if mode == "table" else None, rays=rays)
            assert not bad.any()
            self.ref[key] = (fb, u8, seg)
        return self.ref[key]


def _same(got, want):
    _bits_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert len(got) < 3 or got[2] == want[2], (got[2], want[2])              # the trace counter: every segment, shadow segments included


_scenes = {}


def _glossy(apt, mat, every):
    """Every `every`-th mirror of a generated table becomes a rough-metal sphere of its own roughness."""
    mat = np.array(mat, dtype=np.int32)
    for i in np.nonzero(mat == mr.SPEC)[0][::every]:
        mat[i] = apt.gen_data.gloss((600 + (int(i) * 977) % 64000) / 65536.0)
    return mat


def _scene(apt, name):
    """open8: gen_spheres_open with two of its DIFF balls as lamps; open40: gen_scene_open(40) (one LDS tile), open220: gen_scene_open(220)
    with a grid (four tiles without it), both with two small spheres as lamps and some mirrors as rough metal."""
    if name not in _scenes:
        gd = apt.gen_data
        if name == "open8":
            sph, mat = gd.gen_spheres_open()
            sph = gd.with_lamps(sph, 8, [5, 4], radius=8.0, emission=[(30.0, 20.0, 10.0), 12.0])
            _scenes[name] = Scene(apt, sph, mat, 8, [5, 4], 5)
        else:
            ns = 40 if name == "open40" else 220
            sph, mat = gd.gen_scene_open(ns, seed=2)
            a, b = (7, 19) if ns == 40 else (11, 97)
            sph = gd.with_lamps(sph, ns, [a, b], radius=[1.5, 2.0], emission=[(40.0, 30.0, 20.0), 25.0])
            _scenes[name] = Scene(apt, sph, _glossy(apt, mat, 2), ns, [a, b], a, grid=ns > 64)
        assert _scenes[name].flags[True] == apt.APT_FLAG_GLOSS
    return _scenes[name]


FORMS = [("open8", False), ("open40", False), ("open220", True)]
FORM_IDS = ["8", "tiles40", "grid220"]


def _env(apt, sample):
    return apt.gen_data.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(30.0, 28.0, 24.0),
                                    sun_angle_deg=8.0, sample_sun=sample)


def _lens(apt):
    return apt.gen_data.camera(width=W, height=H, aperture=1.5, eye=(50.0, 45.0, 210.0), target=(50.0, 10.0, 60.0), up=(0.05, 1.0, 0.0),
                               vfov_deg=42.0, offset=0.0)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample", [True, False], ids=["sun-sampled", "sun-plain"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_frames_equal_the_restatement(apt, name, grid, mode, sample):
    sc = _scene(apt, name)
    env = _env(apt, sample)
    assert bool(env.flags & apt.APT_ENV_SAMPLE_SUN) == sample
    for s_, depth, lens, gloss in LAUNCHES:
        cam = _lens(apt) if lens else None
        rays = cr.rays(cr.from_ctypes(cam), W, H, s_, seed=10 + s_) if lens else None
        p = sc.params(W, H, s_, depth, mode=mode, seed=10 + s_, grid=grid, gloss=gloss)
        got = sc.frame(p, mode, env, cam, gloss)
        _same(got, sc.frame_ref(p, mode, env, gloss, rays))
        assert got[0].max() > 0
        if grid:                                                             # the grid form is the tile form
            _same(got, sc.frame(sc.params(W, H, s_, depth, mode=mode, seed=10 + s_, gloss=gloss), mode, env, cam, gloss))


@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_frames_with_roulette(apt, name, grid):
    sc = _scene(apt, name)
    env = _env(apt, True)
    for mode, (s_, depth) in zip(MODES, [(8, 5), (4, 5), (9, 5)]):
        p = sc.params(W, H, s_, depth, mode=mode, rr=True, seed=21, grid=grid)
        _same(sc.frame(p, mode, env), sc.frame_ref(p, mode, env))


def test_the_sun_sample_changes_the_image_by_noise_only_and_depth_one_by_nothing(apt):
    sc = _scene(apt, "open8")
    on, off = _env(apt, True), _env(apt, False)
    p = sc.params(W, H, 8, 1, seed=5)
    _bits_equal(sc.frame(p, "plain", on)[0], sc.frame(p, "plain", off)[0])
    p = sc.params(W, H, 9, 3, seed=5)
    a, b = sc.frame(p, "plain", on), sc.frame(p, "plain", off)
    assert not np.array_equal(a[0], b[0]) and a[2] > b[2]                   # another estimate, and its shadow segments are counted
    assert abs(a[0].mean() - b[0].mean()) < 0.02 * b[0].mean()


@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_a_pixel_range_without_the_byte_frame(apt, name, grid):
    """Pixels [517, 517 + 700) of the frame through the C entries themselves with fb_u8 NULL."""
    import torch
    sc = _scene(apt, name)
    env = _env(apt, True)
    L = apt._lib.lib()
    b, c = 517, 700
    for mode in ("plain", "table"):
        p = sc.params(W, H, 8, 3, mode=mode, seed=31, grid=grid)
        fb = torch.full((3, c), -1.0, dtype=torch.float32, device="cuda")
        args = (ctypes.byref(p), None, ctypes.c_void_p(sc.d_sph.data_ptr()), ctypes.c_void_p(sc.d_mat[True].data_ptr()))
        tail = (ctypes.c_uint64(b), ctypes.c_uint64(c), ctypes.c_void_p(fb.data_ptr()), None)
        apt.render.set_environment(env)
        try:
            rc = L.apt_render_frame_lights(*args, ctypes.c_void_p(sc.d_table.data_ptr()), *tail) if mode == "table" else L.apt_render_frame_materials(*args, *tail)
            torch.cuda.synchronize()
        finally:
            apt.render.set_environment(None)
        assert rc == 0
        apt.render.check_device_status()
        _bits_equal(fb.cpu().numpy(), sc.frame_ref(p, mode, env)[0][:, b:b + c])


def test_a_context_of_its_own_carries_the_environment(apt):
    """Context.set_environment: that context's launches gather the environment, the default context's do not."""
    import torch
    sc = _scene(apt, "open8")
    env = _env(apt, True)
    p = sc.params(W, H, 4, 3, seed=8)
    ctx = apt.render.Context()
    try:
        ctx.set_environment(env)
        fb, u8 = ctx.render_frame(p, sc.d_sph, materials=sc.d_mat[True])
        dark, _ = apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat[True])
        torch.cuda.synchronize()
        ctx.check()
        want = sc.frame_ref(p, "plain", env)
        _bits_equal(fb.cpu().numpy(), want[0])
        assert np.array_equal(u8.cpu().numpy(), want[1])
        _bits_equal(dark.cpu().numpy(), sc.frame_ref(p, "plain", None)[0])
        with pytest.raises(apt.AptError, match="environment"):
            ctx.render_frame(p, sc.d_sph)                                    # its mirror frame entry refuses
    finally:
        ctx.close()


def test_gloss_words_need_the_flag_with_an_environment_too(apt):
    """The environment kernels are the gloss instantiations, but APT_FLAG_GLOSS is still the caller's to give: without it a gloss word is
    the bad code it is without an environment."""
    import torch
    sc = _scene(apt, "open8")
    env = _env(apt, True)
    apt.render.check_device_status()                                         # nothing pending
    for s_ in (1, 8):
        p = sc.params(W, H, s_, 3, seed=1)
        p.flags &= ~apt.APT_FLAG_GLOSS
        apt.render.set_environment(env)
        try:
            apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat[True])
            torch.cuda.synchronize()
        finally:
            apt.render.set_environment(None)
        with pytest.raises(apt.AptError, match="bad-material"):
            apt.render.check_device_status()                                 # reads and clears the word
    p = sc.params(W, H, 8, 3, seed=1)
    _same(sc.frame(p, "plain", env), sc.frame_ref(p, "plain", env))          # and with the flag the table renders clean


# ---- a black environment is no environment ----------------------------------------------------------------------------------------------
def _closed(apt, name):
    import lights_ref as lr
    if ("closed", name) not in _scenes:
        gd = apt.gen_data
        if name == "room8":
            sph, mat, ns = lr.two_lamps(gd)
            sc = Scene(apt, sph, mat, ns, [7, 6], 7)
        elif name == "demo9":
            sc = Scene(apt, *lr.demo_two_lights(gd), [7, 6], 7)
        else:
            ns = 300                                                         # gen_scene's closed room: five tiles, or the grid
            sph, mat = gd.gen_scene_materials(ns, seed=5)
            sph = gd.with_lamps(sph, ns, [50], radius=[1.2], emission=[(60.0, 30.0, 15.0)])
            sc = Scene(apt, sph, mat, ns, [ns - 1, 50], ns - 1, grid=True)
        assert sc.flags[True] == 0                                           # gloss-free
        _scenes["closed", name] = sc
    return _scenes["closed", name]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", [("room8", False), ("demo9", False), ("room300", True)], ids=["8", "tiles9", "grid300"])
def test_a_black_environment_renders_the_image_without_one(apt, name, grid, mode):
    sc = _closed(apt, name)
    black = apt.gen_data.environment()
    assert black.sun_omc == 0 and not any(black.horizon) and not any(black.zenith)
    for s_, depth, rr in ((1, 5, False), (8, 5, True), (9, 3, False)):
        p = sc.params(W, H, s_, depth, mode=mode, rr=rr, seed=40 + s_, grid=grid)
        with_env, without = sc.frame(p, mode, black), sc.frame(p, mode, None)
        _same(with_env, without)
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
            self.scenes[key] = (Scene(self.apt, sph, case.materials(ns), ns, lights, case.light, grid=grid), _dev(case.rays().ravel()))
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
            L, bad, _ = mr.trace(case.rays(), sc.sph, sc.mat[False], ns, case.depth, 1e-4, ep.SEED, case.paths(), mr.Env.from_ctypes(self.env(case)),
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
                colors = self.apt.render.render_paths(p, d_rays, sc.d_sph, materials=sc.d_mat[False], lights=sc.d_table if mode == "table" else None)
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
    _bits_equal(got, physics.restated(case, ns, "plain"))


@pytest.mark.parametrize("ns,grid", PHYS_FORMS, ids=PHYS_IDS)
def test_physics_a_glass_ball_between_the_point_and_the_sun(physics, ns, grid):
    on, off = ep.glass_ball(True), ep.glass_ball(False)
    Lon, Loff = physics.launch(on, ns, grid, "plain"), physics.launch(off, ns, grid, "plain")
    m1, s1, same1 = ep.summarise(Lon)
    m0, s0, same0 = ep.summarise(Loff)
    assert not same1.any() and not same0.any() and (m0 > 0.01).all()
    z = np.abs(m1 - m0) / np.sqrt((s1 * s1 + s0 * s0) / ep.COPIES)
    assert z.max() <= ep.Z_CAP
    _bits_equal(Lon, physics.restated(on, ns, "plain"))
    _bits_equal(Loff, physics.restated(off, ns, "plain"))


@pytest.mark.parametrize("sample", [True, False], ids=["sun-sampled", "sun-plain"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ns,grid", PHYS_FORMS, ids=PHYS_IDS)
def test_physics_the_sun_next_to_a_sphere_lamp(physics, ns, grid, mode, sample):
    case = ep.sun_and_lamp(sample)
    case.name += "_on" if sample else "_off"
    got = physics.launch(case, ns, grid, mode)
    _check(case, got, mode)
    _bits_equal(got, physics.restated(case, ns, mode))


# ---- the grid's promise ------------------------------------------------------------------------------------------------------------------
def test_a_grid_that_is_not_the_scenes_writes_nothing(apt):
    import torch
    sc = _scene(apt, "open220")
    other = apt.gen_data.build_grid(apt.gen_data.gen_scene_open(100, seed=9)[0], 100)
    d_other = torch.from_numpy(other.view(np.int32)).cuda()
    env = _env(apt, True)
    apt.render.check_device_status()                                         # nothing pending
    for s_ in (1, 8):
        p = sc.params(W, H, s_, 3, seed=2, flags=apt.APT_FLAG_GRID_SLOTS)
        p.accel = d_other.data_ptr()
        fb = torch.full((3, W * H), -2.0, dtype=torch.float32, device="cuda")
        apt.render.set_environment(env)
        try:
            apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat[True], fb=fb)
            torch.cuda.synchronize()
        finally:
            apt.render.set_environment(None)
        assert (fb.cpu().numpy() == -2.0).all()
        with pytest.raises(apt.AptError, match="grid-mismatch"):
            apt.render.check_device_status()                                 # reads and clears the word
    rays = _dev(np.zeros(6 * W * H * 4, dtype=np.float32))
    colors = torch.full((3 * W * H * 4,), -2.0, dtype=torch.float32, device="cuda")
    p = sc.params(W, H, 1, 3, seed=2, flags=apt.APT_FLAG_GRID_SLOTS)
    p.accel = d_other.data_ptr()
    apt.render.set_environment(env)
    try:
        apt.render.render_do_ex(p, None, rays, sc.d_sph, colors, materials=sc.d_mat[True])
        torch.cuda.synchronize()
    finally:
        apt.render.set_environment(None)
    assert (colors.cpu().numpy() == -2.0).all()
    with pytest.raises(apt.AptError, match="grid-mismatch"):
        apt.render.check_device_status()
