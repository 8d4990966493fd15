"""CPU-only: the environment (include/render_mi355x.h "environment") -- the record's host entries through ctypes with every refusal and
the context state, the restatement tests/materials_ref.py with a black environment against itself without one bit for bit, and
the restatement against physics written in float64 from geometry alone (tests/env_physics.py, which imports no restatement): a uniform
and a graded sky, the sun sampled and not, an occluder, a mirror ball, a glass ball, the sun next to a sphere lamp.

Without the feature nothing here passes: the entries, gen_data.environment and the scene generators do not exist."""
import ctypes

import numpy as np
import pytest

import env_physics as ep
import lights_ref as lr
import materials_ref as mr

F, U = np.float32, np.uint64


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data, render
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


# ---- host entries -------------------------------------------------------------------------------------------------------------------
def test_record_layout_and_symbols(apt):
    from ascendpathtracing_amd._lib import ApEnvironment
    assert ctypes.sizeof(ApEnvironment) == 60 and ApEnvironment.horizon.offset == 8 and ApEnvironment.sun_omc.offset == 56
    assert ctypes.sizeof(apt.RenderParams) == 80 and apt._lib.lib().apt_abi_version() == 3          # additive: no new field, same ABI version
    for name in ("apt_environment_build_host", "apt_environment_check_host", "apt_context_set_environment", "apt_set_environment"):
        assert name in apt._lib.ABI_SYMBOLS
    header = open(mr.ROOT + "/include/render_mi355x.h").read()
    assert "APT_ENV_SUN_SALT 0x%016Xull" % int(mr.SUN_SALT) in header and "#define APT_ABI_VERSION 3 " in header


def test_build_then_check_round_trip(apt):
    L = apt._lib.lib()
    e = apt.gen_data.environment(horizon=(0.25, 0.5, 0.75), zenith=(1.0, 2.0, 3.0), sun_dir=(3.0, 4.0, 12.0), sun_radiance=(100.0, 90.0, 80.0),
                                 sun_angle_deg=5.0, sample_sun=True)
    assert L.apt_environment_check_host(ctypes.byref(e)) == 0 and L.apt_last_error() == b""
    assert e.struct_size == 60 and e.flags == apt.APT_ENV_SAMPLE_SUN
    assert list(e.horizon) == [0.25, 0.5, 0.75] and list(e.zenith) == [1.0, 2.0, 3.0] and list(e.sun_radiance) == [100.0, 90.0, 80.0]
    # normalised in float64, one operation at a time (np.linalg.norm's fma chain), each field rounded once
    n = np.sqrt(np.float64(144.0) + (np.float64(16.0) + np.float64(9.0)))
    assert n == 13.0 and list(e.sun_dir) == [float(F(3.0 / 13.0)), float(F(4.0 / 13.0)), float(F(12.0 / 13.0))]
    half = np.sin(np.radians(np.float64(5.0)) * 0.5)
    assert e.sun_omc == float(F(2.0 * half * half)) and abs(e.sun_omc - (1.0 - np.cos(np.radians(5.0)))) < 1e-9
    # no sun: the flag is dropped, the direction is kept as it is
    none = apt.gen_data.environment(horizon=0.5, sun_dir=(0.0, 0.0, 0.0))
    assert none.sun_omc == 0.0 and none.flags == 0 and list(none.zenith) == [0.5] * 3 and L.apt_environment_check_host(ctypes.byref(none)) == 0
    # an awkward direction still lands within the check's 2^-20
    for d in ((1e-8, 3e-8, -2e-8), (1e25, -1.0, 3.0), (0.1, 0.7, -0.3)):
        rec = apt.gen_data.environment(sun_dir=d, sun_radiance=1.0, sun_angle_deg=1.0)
        v = np.array(list(rec.sun_dir), dtype=np.float64)
        assert abs(v @ v - 1.0) < 2.0 ** -22 and L.apt_environment_check_host(ctypes.byref(rec)) == 0
    with pytest.raises(apt.AptError):
        apt.gen_data.environment(sun_angle_deg=91.0)
    with pytest.raises(apt.AptError, match="non-zero"):
        apt.gen_data.environment(sun_dir=(0, 0, 0), sun_radiance=1.0, sun_angle_deg=1.0)
    with pytest.raises(apt.AptError, match="radiance"):
        apt.gen_data.environment(horizon=(-1.0, 0, 0))


def _refusals(apt):
    """(what, record, status) for every refusal of the header's list."""
    good = apt.gen_data.environment(horizon=(0.25, 0.5, 0.75), zenith=1.0, sun_dir=(0, 1, 0), sun_radiance=4.0, sun_angle_deg=10.0)
    nan, inf = float("nan"), float("inf")
    out = [("struct_size", good.copy(struct_size=56), 2), ("struct_size 0", good.copy(struct_size=0), 2), ("flags", good.copy(flags=2), 1),
           ("flags high", good.copy(flags=0x80000001), 1)]
    for field in ("horizon", "zenith", "sun_radiance"):
        for v in (nan, inf, -1.0, -1e-30):
            for k in range(3):
                t = [0.5, 0.5, 0.5]
                t[k] = v
                out.append(("%s[%d]=%r" % (field, k, v), good.copy(**{field: t}), 1))
    for v in (nan, -1e-6, 1.0000001, inf, -inf, 2.0):
        out.append(("sun_omc=%r" % v, good.copy(sun_omc=v), 1))
    for d in ((0.0, 1.001, 0.0), (0.0, 0.999, 0.0), (0.0, 0.0, 0.0), (nan, 1.0, 0.0), (0.0, inf, 0.0), (0.6, 0.6, 0.6),
              (0.0, float(F(1.0 + 2.0 ** -20)), 0.0)):                       # squared length 1 + 2^-19: just outside
        out.append(("sun_dir=%r" % (d,), good.copy(sun_dir=d), 1))
    return good, out


def test_every_refusal_keeps_the_previous_record(apt):
    L = apt._lib.lib()
    good, bad = _refusals(apt)
    ctx = ctypes.c_void_p(L.apt_context_create())
    one, u64 = ctypes.c_void_p(16), ctypes.c_uint64
    p = apt.make_params(16, 16, 1)
    refused = lambda: L.apt_context_render_frame(ctx, ctypes.byref(p), None, one, u64(0), u64(10), one, None) == 1 and b"environment" in L.apt_last_error()
    try:
        assert L.apt_environment_check_host(None) == 1 and L.apt_context_set_environment(None, ctypes.byref(good)) == 1
        assert L.apt_environment_check_host(ctypes.byref(good)) == 0
        assert not refused()                                                 # no environment yet: the mirror entry gets further
        assert L.apt_context_set_environment(ctx, ctypes.byref(good)) == 0 and refused()
        for what, rec, status in bad:
            assert L.apt_environment_check_host(ctypes.byref(rec)) == status and L.apt_last_error() != b"" and L.apt_last_status() == status, what
            assert L.apt_context_set_environment(ctx, ctypes.byref(rec)) == status, what
            assert refused(), what                                           # the previous record is still in place
        # a direction of any length is fine while there is no sun, and the rim of the length rule is inside
        assert L.apt_environment_check_host(ctypes.byref(good.copy(sun_omc=0.0, sun_dir=(0.0, 7.0, 0.0), flags=0))) == 0
        assert L.apt_environment_check_host(ctypes.byref(good.copy(sun_dir=(0.0, float(F(1.0 + 2.0 ** -22)), 0.0)))) == 0
        assert L.apt_environment_check_host(ctypes.byref(good.copy(sun_omc=1.0))) == 0
        # the builder refuses what the check refuses, and writes nothing
        d3 = ctypes.c_double * 3
        out = good.copy(horizon=(9.0, 9.0, 9.0))
        build = lambda hz=(0, 0, 0), zn=(0, 0, 0), sd=(0, 1, 0), sr=(1, 1, 1), omc=0.5, fl=0, o=out: L.apt_environment_build_host(
            d3(*hz), d3(*zn), d3(*sd), d3(*sr), ctypes.c_double(omc), ctypes.c_uint32(fl), ctypes.byref(o))
        for kw in (dict(hz=(-1, 0, 0)), dict(zn=(0, float("inf"), 0)), dict(sr=(0, 0, float("nan"))), dict(omc=1.5), dict(omc=-0.1), dict(omc=float("nan")),
                   dict(fl=4), dict(sd=(0, 0, 0)), dict(sd=(float("nan"), 1, 0))):
            assert build(**kw) == 1 and L.apt_last_error() != b"", kw
            assert list(out.horizon) == [9.0, 9.0, 9.0]
        assert build(o=good.copy(struct_size=64)) == 2
        assert L.apt_environment_build_host(None, d3(), d3(), d3(), ctypes.c_double(0), ctypes.c_uint32(0), ctypes.byref(out)) == 1
        assert build() == 0 and list(out.horizon) == [0.0, 0.0, 0.0]
        # NULL removes it
        assert L.apt_context_set_environment(ctx, None) == 0 and not refused()
    finally:
        L.apt_context_destroy(ctx)


def test_mirror_frame_entries_refuse_with_an_environment_set_and_need_no_gpu(apt):
    L = apt._lib.lib()
    one, u64 = ctypes.c_void_p(16), ctypes.c_uint64          # never dereferenced: the refusal comes first
    env = apt.gen_data.environment(horizon=1.0)
    p = apt.make_params(16, 16, 1)
    ctx, other = apt.render.Context(), apt.render.Context()
    frame = lambda q, c=10: L.render_frame(q, None, one, u64(0), u64(c), one, None)
    cframe = lambda h, q, c=10: L.apt_context_render_frame(h, q, None, one, u64(0), u64(c), one, None)
    frame_mt = lambda q: L.apt_render_frame_mt(q, None, one, u64(1), u64(0), one, u64(0), u64(10), one, None)
    ids = (ctypes.c_int * 1)(0)
    sph = apt.gen_data.gen_spheres()
    handle = ctypes.c_void_p()
    multi = lambda q: L.apt_multi_create(ids, ctypes.c_uint32(1), ctypes.c_uint32(1), q, ctypes.c_void_p(sph.ctypes.data), ctypes.byref(handle))
    is_env = lambda: b"environment" in L.apt_last_error() and L.apt_last_status() == 1
    try:
        ctx.set_environment(env)
        assert cframe(ctx._h, ctypes.byref(p)) == 1 and is_env()
        assert cframe(other._h, ctypes.byref(p), c=0) == 0                  # another context has none
        apt.render.set_environment(env)
        for call in (frame, frame_mt, multi):
            assert call(ctypes.byref(p)) == 1 and is_env(), call           # the camera's status, APT_ERR_ARG
        # their own refusals come first, as with a camera
        bad = apt.default_params(); bad.struct_size = 8
        assert frame(ctypes.byref(bad)) == 2 and frame(None) == 1 and b"params is null" in L.apt_last_error()
        assert frame(ctypes.byref(p), c=10 ** 9) == 1 and b"pixel range" in L.apt_last_error()
        assert frame(ctypes.byref(p), c=0) == 0
        # the material entries' own checks are what they were, and an empty range is still a no-op
        e = apt.make_params(16, 16, 1, path_begin=1024)
        assert L.render_do_ex(ctypes.byref(e), None, one, one, one) == 0
        assert L.apt_render_paths_materials(ctypes.byref(e), None, one, one, one, one) == 0
        assert L.apt_render_frame_materials(ctypes.byref(p), None, one, None, u64(0), u64(10), one, None) == 1 and b"materials" in L.apt_last_error()
        apt.render.set_environment(None)
        ctx.set_environment(None)
        assert cframe(ctx._h, ctypes.byref(p), c=10 ** 9) == 1 and b"pixel range" in L.apt_last_error()
        rc = multi(ctypes.byref(p))
        assert not is_env() and rc in (0, apt._lib.APT_ERR_DEVICE)
        if rc == 0:
            L.apt_multi_destroy(handle)
    finally:
        apt.render.set_environment(None)
        ctx.close()
        other.close()


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------
def test_open_scenes_and_their_grids(apt):
    g = apt.gen_data
    sph, mat = g.gen_spheres_open()
    assert sph.shape == (128,) and mat.shape == (8,) and g.materials_flags(mat) == apt.APT_FLAG_GLOSS
    planes = sph[:80].reshape(10, 8)
    assert (planes[4:7] == 0).all()                                         # no emitter
    codes = {int(m) & 0xFF for m in mat}
    assert codes == {apt.MAT_SPEC, apt.MAT_DIFF, apt.MAT_REFR, apt.MAT_GLOSS}
    assert planes[0, 0] == F(1e10) and planes[2, 0] == F(-1e5)             # the ground, top at y = 0
    r = np.sqrt(planes[0, 1:].astype(np.float64))
    assert np.allclose(planes[2, 1:], r)                                    # the balls stand on it
    for ns in (40, 250):
        sph, mat = g.gen_scene_open(ns, seed=3)
        assert sph.size == (10 * ns + 127) // 128 * 128 and mat.shape == (ns,) and set(mat.tolist()) <= {0, 1, 2}
        planes = sph[:10 * ns].reshape(10, ns)
        assert planes[0, 0] == F(1e10) and (planes[0, 1:] <= 4.0).all() and (planes[4:7] == 0).all()
        src = g.gen_scene(ns + 6, seed=3)[:10 * (ns + 6)].reshape(10, ns + 6)
        assert np.array_equal(planes[:, 1:], src[:, 6:ns + 5])
        grid = g.build_grid(sph, ns)                                        # apt_build_grid_host accepts it
        assert g.grid_flags(grid, ns) == apt.APT_FLAG_GRID_SLOTS
    with pytest.raises(apt.AptError):
        g.gen_scene_open(1)


# ---- a black environment is no environment -------------------------------------------------------------------------------------------
BLACK = mr.Env()


def _frame_rays(oracle, w, h, s, seed):
    return oracle.gen_rays_counter(oracle.make_params(w, h, s, depth=5, seed=seed))


@pytest.mark.parametrize("rr", [0, 2], ids=["", "rr"])
def test_black_environment_equals_no_environment(apt, oracle, rr):
    """env=the black Env() against env=None (whose bytes tests/test_restatement_frozen.py records) in every mode: plain, APT_FLAG_NEE,
    a light table, a gloss ball in all three."""
    g = apt.gen_data
    rays = _frame_rays(oracle, 24, 16, 2, 7)
    n = rays.shape[1]
    paths = np.arange(n, dtype=U)
    # plain: the demo scene (9 spheres, glass ball) and the 8-sphere DIFF room
    for sph, mat, ns in ((*g.gen_spheres_materials(), 9), (g.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 8)):
        want, bad, seg = mr.trace(rays, sph, mat, ns, 5, 1e-4, 7, paths, None, rr, gloss=False)
        got, gbad, gseg = mr.trace(rays, sph, mat, ns, 5, 1e-4, 7, paths, BLACK, rr, gloss=False)
        _bits_equal(got, want)
        assert np.array_equal(gbad, bad) and gseg == seg and want.max() > 0
    # APT_FLAG_NEE: the demo scene with smallpt's lamp
    sph, mat = g.gen_spheres_materials()
    sph = g.with_lamp(sph, 9, 7)
    want, bad, seg = mr.trace(rays, sph, mat, 9, 5, 1e-4, 7, paths, None, rr, light=7, nee=True, gloss=False)
    got, gbad, gseg = mr.trace(rays, sph, mat, 9, 5, 1e-4, 7, paths, BLACK, rr, light=7, nee=True, gloss=False)
    _bits_equal(got, want)
    assert gseg == seg and not bad.any() and not gbad.any()
    # a light table: two lights of the demo scene, and the 8-sphere room with two lamps
    for sph, mat, ns in (lr.demo_two_lights(g), lr.two_lamps(g)):
        table = lr.build_table(sph, ns, [7, 6])
        want, bad, seg = mr.trace(rays, sph, mat, ns, 5, 1e-4, 7, paths, None, rr, table=table, gloss=False)
        got, gbad, gseg = mr.trace(rays, sph, mat, ns, 5, 1e-4, 7, paths, BLACK, rr, table=table, gloss=False)
        _bits_equal(got, want)
        assert gseg == seg and not gbad.any()
    # the rough-metal material: the room with a gloss ball, all three light modes
    sph, mat, ns = lr.two_lamps(g)
    mat = mat.copy()
    mat[6] = g.gloss(0.3)
    table = lr.build_table(sph, ns, [7, 6])
    for kw in ({}, dict(light=7, nee=True), dict(table=table)):
        want, bad, seg = mr.trace(rays, sph, mat, ns, 5, 1e-4, 7, paths, None, rr, **kw)
        got, gbad, gseg = mr.trace(rays, sph, mat, ns, 5, 1e-4, 7, paths, BLACK, rr, **kw)
        _bits_equal(got, want)
        assert gseg == seg and not gbad.any() and want.max() > 0
    # and an environment that is not black changes an open scene, so the comparison above is not vacuous
    sph, mat = g.gen_spheres_open()
    lit, _, _ = mr.trace(rays, sph, mat, 8, 5, 1e-4, 7, paths, mr.Env(horizon=(1, 1, 1), zenith=(1, 1, 1)), rr)
    dark, _, _ = mr.trace(rays, sph, mat, 8, 5, 1e-4, 7, paths, BLACK, rr)
    assert dark.max() == 0 and (lit > 0).mean() > 0.9


def test_the_restatement_has_no_float64_intermediates(apt):
    """f32() guards every step of the restatement; a float64 constant slipped into the environment's own steps must trip it."""
    env = mr.Env(horizon=(0.25, 0.5, 0.75), zenith=(1, 2, 3), sun_dir=(0, 1, 0), sun_radiance=(4, 4, 4), sun_omc=0.0625, flags=1)
    rays = ep.sun_only(True).rays()[:, :256]
    L, _, _ = mr.trace(rays, ep.sun_only(True).table(8), ep.sun_only(True).materials(8), 8, 3, 1e-4, 1, np.arange(256, dtype=U), env)
    assert L.dtype == F
    wide = mr.Env(horizon=(0.25, 0.5, 0.75), zenith=(1, 2, 3))
    wide.horizon = [np.float64(x) for x in wide.horizon]
    with pytest.raises(AssertionError):
        mr.sky(wide, rays[4])
    wide = mr.Env(sun_dir=(0, 1, 0), sun_radiance=(4, 4, 4), sun_omc=0.0625, flags=1)
    wide.sun_omc = np.float64(0.0625)
    with pytest.raises(AssertionError):
        mr.sun_sample(wide, [rays[3], rays[4], rays[5]], mr.splitmix64(np.arange(256, dtype=U)), 0)


# ---- physics --------------------------------------------------------------------------------------------------------------------------
def _env_of(case):
    e = case.env
    return mr.Env(e["horizon"], e["zenith"], e["sun_dir"], e["sun_radiance"], e["sun_omc"], e.get("flags", 0))


def _render(case, ns=8, mode="plain", real_only=False):
    """materials_ref on the case's rays; real_only: the scene without its parked spheres."""
    n = len(case.rows) if real_only else ns
    sph, mat = case.table(n), case.materials(n)
    kw = {}
    if mode == "nee":
        kw = dict(light=case.light, nee=True)
    elif mode == "table":
        kw = dict(table=lr.build_table(sph, n, case.lights))
    L, bad, _ = mr.trace(case.rays(), sph, mat, n, case.depth, 1e-4, ep.SEED, case.paths(), _env_of(case), gloss=False, **kw)
    assert not bad.any()
    return L


def _check(case, L, label=""):
    c = ep.compare(L, case.want, case.exact)
    print("%-22s %-6s max |z| %.2f over %d differing components, all-equal error %.2e" % (case.name, label, c["zmax"], c["differing"], c["exact"]))
    assert ep.passes(c, case.exact), c
    return c


CASES = [ep.uniform_sky(1), ep.uniform_sky(2), ep.uniform_sky(5), ep.gradient_sky(), ep.sun_only(False), ep.sun_only(True), ep.sun_only(True, 5),
         ep.occluder(), ep.mirror_ball(False), ep.mirror_ball(True)]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_physics(case):
    L = _render(case)
    _check(case, L)
    _bits_equal(L, _render(case, real_only=True))                           # no path meets a parked sphere
    _bits_equal(L, _render(case, ns=9))


def test_physics_a_glass_ball_between_the_point_and_the_sun():
    """APT_ENV_SAMPLE_SUN on and off estimate the same light through the glass: `sampled_sun` is cleared at the hits in between."""
    on, off = ep.glass_ball(True), ep.glass_ball(False)
    Lon, Loff = _render(on), _render(off)
    _bits_equal(Lon, _render(on, real_only=True))
    m1, s1, same1 = ep.summarise(Lon)
    m0, s0, same0 = ep.summarise(Loff)
    assert not same1.any() and not same0.any() and (m0 > 0.01).all()       # light does arrive through the ball
    z = np.abs(m1 - m0) / np.sqrt((s1 * s1 + s0 * s0) / ep.COPIES)
    print("glass ball: on %s off %s max |z| %.2f" % (m1[0], m0[0], z.max()))
    assert z.max() <= ep.Z_CAP


@pytest.mark.parametrize("sample", [True, False], ids=["sampled", "plain"])
@pytest.mark.parametrize("mode", ["plain", "nee", "table"])
def test_physics_the_sun_next_to_a_sphere_lamp(mode, sample):
    case = ep.sun_and_lamp(sample)
    L = _render(case, mode=mode)
    _check(case, L, mode)
    _bits_equal(L, _render(case, mode=mode, real_only=True))
