"""What the material renderer's GPU test files share (tests/test_gpu_materials*.py, _nee, _lights, _gloss, _camera, _environment, _film,
_features, _glass_physics, _deep_plans, _material_matrix, _mis, _film_list, _degenerate_scenes): the `apt` fixture, the comparisons, one
Scene and the scenes that more than one file renders; and, for the CPU tests that restate them (test_mis_cpu, test_degenerate_scenes_cpu,
test_restatement_frozen, the CPU halves of the matrices), the device-free `host` fixture.  A plain module beside materials_ref.py,
imported the same way: `from gpu_harness import apt  # noqa: F401` brings the fixture.  tests/mat_rows.py holds what the row matrices share.

A Scene's host half -- the tables the restatements read -- needs no device: the tensors are made on first use."""
import contextlib
import functools

import numpy as np
import pytest

import camera_ref as cr
import lights_ref as lr
import materials_ref as mr

F = np.float32


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def load_host():
    """The package without a device: scenes, cameras, environments and light tables are host data."""
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data
    pkg.gen_data = gen_data
    return pkg


@pytest.fixture(scope="module")
def host():
    return load_host()


def dev(a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def bits_equal(a, b):
    """-> bool: for a condition that a test asserts itself."""
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def assert_bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def same(got, want):
    """(fb, u8[, traced]) twice: fb bit for bit, u8 equal and, where both carry it, the trace counter: every segment, shadow segments included."""
    assert_bits_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])
    assert len(got) < 3 or len(want) < 3 or got[2] == want[2], (got[2], want[2])


def oracle_params(p):
    from oracle import oracle
    return oracle.Params.from_buffer_copy(bytes(p.copy(accel=0, flags=p.flags & ~16)))   # the restatements know no grid


class Scene:
    """A scene: the sphere table, its material words (`mat`; `plain`: the same with every gloss word a mirror), the light table of
    `lights` (None: every emitter), the light of APT_FLAG_NEE; grid=True builds a grid FROM THIS TABLE (builder: "host" or "device").
    Launches go through the default context and leave it without camera or environment."""

    def __init__(self, apt, sph, mat, ns, lights=None, light=-1, grid=False, builder="host"):
        self.apt, self.sph, self.mat, self.ns = apt, np.asarray(sph, dtype=F), np.asarray(mat, dtype=np.int32), int(ns)
        self.lights, self.light, self.ref = lights, light, {}
        self.plain = self.mat.copy()
        self.plain[(self.plain & 0xFF) == 3] = mr.SPEC
        self.mat_flags = apt.gen_data.materials_flags(self.mat)
        assert apt.gen_data.materials_flags(self.plain) == 0
        self.hgrid, self.grid_flags = None, 0
        if grid:
            if builder == "host":
                self.hgrid = apt.gen_data.build_grid(self.sph, self.ns)
            else:
                import torch
                self.grid = apt.gen_data.build_grid_device(self.d_sph, self.ns)
                torch.cuda.synchronize()
                self.hgrid = self.grid.cpu().numpy().view(np.uint32)
            self.grid_flags = apt.gen_data.grid_flags(self.hgrid, self.ns)
            assert self.grid_flags == apt.APT_FLAG_GRID_SLOTS

    # ---- the host half, continued, and the device half: each made once, when first asked for
    @functools.cached_property
    def table(self):
        return self.apt.gen_data.build_lights(self.sph, self.ns, self.lights)

    @functools.cached_property
    def grid(self):
        import torch
        return None if self.hgrid is None else torch.from_numpy(self.hgrid.view(np.int32)).cuda()

    d_sph = functools.cached_property(lambda self: dev(self.sph))
    d_mat = functools.cached_property(lambda self: dev(self.mat))
    d_plain = functools.cached_property(lambda self: dev(self.plain))
    d_table = functools.cached_property(lambda self: dev(self.table.view(np.int32)))

    def params(self, w, h, s_, depth, mode="plain", rr=False, seed=3, grid=False, gloss=None, **kw):
        """gloss: None / True = the flags the words earn, False / 0 = none, or the flag itself; grid=True needs a Scene built with one."""
        apt = self.apt
        assert not grid or self.hgrid is not None
        flags = kw.pop("flags", 0) | (apt.APT_FLAG_NEE if mode == "nee" else 0) | (apt.APT_FLAG_RR if rr else 0)
        flags |= (self.grid_flags if grid else 0) | (self.mat_flags if gloss is None or gloss is True else int(gloss))
        return apt.make_params(w, h, s_, depth=depth, num_spheres=self.ns, light_index=self.light, seed=seed, flags=flags,
                               rr_start=2 if rr else 0, accel=self.grid.data_ptr() if grid else 0, **kw)

    @contextlib.contextmanager
    def view(self, cam=None, env=None):
        """The default context with `cam` and `env` set; both unset again on the way out."""
        render = self.apt.render
        render.set_camera(cam)
        render.set_environment(env)
        try:
            yield
        finally:
            render.set_camera(None)
            render.set_environment(None)

    def _launch(self, cam, env, check, count, fn):
        import torch
        render = self.apt.render
        with self.view(cam, env), (render.TraceCounter() if count else contextlib.nullcontext()) as tc:
            out = fn()
            torch.cuda.synchronize()
        if check:
            render.check_device_status()                      # the status word is clean after the launch
        return out, (tc.value if count else None)

    def frame(self, p, mode="plain", cam=None, env=None, gloss=True, check=True, count=False, **kw):
        """One frame launch -> (fb, u8) or, with count, (fb, u8, segments traced).  mode "table": the light-table entry; otherwise the
        *_materials entry, which reads APT_FLAG_NEE from p.  gloss=False: the gloss-free words."""
        (fb, u8), traced = self._launch(cam, env, check, count, lambda: self.apt.render.render_frame(
            p, self.d_sph, materials=self.d_mat if gloss else self.d_plain, lights=self.d_table if mode == "table" else None, **kw))
        return (fb.cpu().numpy(), u8.cpu().numpy()) + ((traced,) if count else ())

    def paths(self, p, rays, mode="plain", check=True):
        """Buffer mode on host rays [6][n] -> colours [3][n], NaN where nothing was written."""
        import torch
        n = rays.shape[1]
        colors = torch.full((3 * n,), float("nan"), dtype=torch.float32, device="cuda")
        self._launch(None, None, check, False, lambda: self.apt.render.render_do_ex(
            p, None, dev(rays.ravel()), self.d_sph, colors, materials=self.d_mat, lights=self.d_table if mode == "table" else None))
        return colors.cpu().numpy().reshape(3, n)

    def film_passes(self, p, mode, env, cam, upto, film=None, checkpoints=()):
        """Passes 0 .. upto - 1 of `p` -> ({k: the film after k passes, for k in checkpoints}, [segments traced per pass])."""
        import torch
        if film is None:
            film = torch.full((3, p.width * p.height), -5.0, dtype=torch.float32, device="cuda")
        snaps, traced = {}, []
        for k in range(upto):
            _, seg = self._launch(cam, env, k == upto - 1, True, lambda: self.apt.render.render_frame_film(
                p, self.d_sph, self.d_mat, film=film, pass_index=k, lights=self.d_table if mode == "table" else None))
            traced.append(seg)
            if k + 1 in checkpoints:
                snaps[k + 1] = film.cpu().numpy().copy()
        return snaps, traced

    def features(self, p, cam=None, **kw):
        """The first-hit feature planes of the launch `p` -> host [8][count]."""
        out, _ = self._launch(cam, None, True, False, lambda: self.apt.render.render_frame_features(p, self.d_sph, **kw))
        return out.cpu().numpy()

    def frame_ref(self, p, mode="plain", cam=None, env=None, gloss=True):
        """materials_ref's whole frame for the launch `p` (APT_FLAG_MIS read from its flags, like the others) -> (fb, u8, segments),
        computed once.  The key holds every input of the restatement but the scene: p without its grid (which changes no image), table or
        not, the words, the camera and the environment."""
        key = (bytes(oracle_params(p)), mode == "table", bool(gloss), None if cam is None else bytes(cam), None if env is None else bytes(env))
        if key not in self.ref:
            rays = None if cam is None else cr.rays(cr.from_ctypes(cam), p.width, p.height, p.samples, seed=p.seed)
            fb, u8, bad, seg = mr.render_frame(oracle_params(p), self.sph, self.mat if gloss else self.plain,
                                               env=None if env is None else mr.Env.from_ctypes(env),
                                               table=self.table if mode == "table" else None, rays=rays)
            assert not bad.any()
            self.ref[key] = (fb, u8, seg)
        return self.ref[key]


# ---- the scenes, the cameras and the environment that more than one file renders ---------------------------------------------------------
def _glossy(apt, mat, every):
    """Every `every`-th mirror of a generated table becomes a rough-metal sphere of its own roughness."""
    mat = np.array(mat, dtype=np.int32)
    for i in np.nonzero(mat == mr.SPEC)[0][::every]:
        mat[i] = apt.gen_data.gloss((600 + (int(i) * 977) % 64000) / 65536.0)
    return mat


def _build(apt, name):
    gd = apt.gen_data
    if name in ("two8", "room8"):                          # 8 spheres (SGPR form), spheres 6 and 7 lamps: every emitter / listed 7, 6
        sph, mat, ns = lr.two_lamps(gd)
        return Scene(apt, sph, mat, ns, None if name == "two8" else [7, 6], 7)
    if name == "demo9x2":                                  # the demo scene with the glass ball (tiles), the mirror ball a second light
        return Scene(apt, *lr.demo_two_lights(gd), [7, 6], 7)
    if name == "big1030x2":                                # 1030 spheres by tiles and through a grid, the stock light and one lamp listed
        sph, mat, ns, idx = lr.sixteen_lamps(gd)
        return Scene(apt, sph, mat, ns, [ns - 1, idx[5]], ns - 1, grid=True)
    if name == "open8":                                    # gen_spheres_open with two of its DIFF balls as lamps
        sph, mat = gd.gen_spheres_open()
        sph = gd.with_lamps(sph, 8, [5, 4], radius=8.0, emission=[(30.0, 20.0, 10.0), 12.0])
        return Scene(apt, sph, mat, 8, [5, 4], 5)
    if name in ("open40", "open220"):                      # gen_scene_open: one LDS tile / a grid; two lamps, every second mirror rough metal
        ns = int(name[4:])
        sph, mat = gd.gen_scene_open(ns, seed=2)
        a, b = (7, 19) if ns == 40 else (11, 97)
        sph = gd.with_lamps(sph, ns, [a, b], radius=[1.5, 2.0], emission=[(40.0, 30.0, 20.0), 25.0])
        return Scene(apt, sph, _glossy(apt, mat, 2), ns, [a, b], a, grid=ns > 64)
    if name == "big1030g":                                 # big1030x2 with every second mirror rough metal (Scene.plain: gloss-free again)
        sph, mat, ns, idx = lr.sixteen_lamps(gd)
        return Scene(apt, sph, _glossy(apt, mat, 2), ns, [ns - 1, idx[5]], ns - 1, grid=True)
    base, kind = name.split("-")                           # "<diff8|demo9|big1030>-<stock|lamp>": the closed rooms, their light listed alone
    assert kind in ("stock", "lamp")
    if base in ("gloss8", "gloss9"):                       # closed rooms for every kernel of materials.hip: the ball (sphere 6) rough metal and a
        if base == "gloss8":                               # weak second light, the light (sphere 7) the stock one or smallpt's lamp; two listed
            sph, mat = gd.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
            mat[6] = gd.gloss(0.3)
        else:                                              # the demo scene with its glass ball; with a grid of its own (form 2 at 9 spheres)
            sph, mat = gd.gen_spheres_materials(gloss=0.25)
        ns = int(np.asarray(mat).size)
        sph = np.array(sph, dtype=F)
        sph[:10 * ns].reshape(10, ns)[4:7, 6] = [3.0, 6.0, 9.0]
        if kind == "lamp":
            sph = gd.with_lamp(sph, ns, 7)
        return Scene(apt, sph, mat, ns, [7, 6], 7, grid=ns != 8)
    if base == "diff8":                                    # 8-sphere form: DIFF walls and light, the mirror SPEC
        sph, mat, light = gd.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 7
    elif base == "demo9":                                  # tile form: gen_spheres + the glass ball
        sph, mat = gd.gen_spheres_materials()
        light = 7
    else:                                                  # > one 1024-sphere tile, and its grid; small spheres of every code
        assert base == "big1030"
        sph, mat = gd.gen_scene_materials(1030, seed=5)
        light = 1029
    ns = int(np.asarray(mat).size)
    if kind == "lamp":                                     # smallpt's small lamp in the light's place
        sph = gd.with_lamp(sph, ns, light)
    return Scene(apt, sph, mat, ns, [light], light, grid=base == "big1030")


_scenes = {}


def scene(apt, name):
    if name not in _scenes:
        _scenes[name] = _build(apt, name)
    return _scenes[name]


def pinhole(apt, w, h, aperture=0.0):
    return apt.gen_data.camera(width=w, height=h, aperture=aperture, eye=(50.0, 45.0, 210.0), target=(50.0, 10.0, 60.0), up=(0.05, 1.0, 0.0),
                               vfov_deg=42.0, offset=0.0)


def lens(apt, w, h):
    return pinhole(apt, w, h, aperture=1.5)


def inside_pinhole(apt, w, h, aperture=0.0):
    """A look-at camera whose eye is INSIDE the closed rooms (x in [1, 99], y in [0, 81.6], z in [0, 170]); pinhole / lens put theirs
    at z = 210, behind the front wall, from where a closed room renders black.  It sees the open scenes' balls as well."""
    return apt.gen_data.camera(width=w, height=h, aperture=aperture, eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05),
                               vfov_deg=55.0, offset=0.0)


def inside_lens(apt, w, h):
    return inside_pinhole(apt, w, h, aperture=2.5)


def sky_and_sun(apt, sample=True):
    return apt.gen_data.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(30.0, 28.0, 24.0),
                                    sun_angle_deg=8.0, sample_sun=sample)
