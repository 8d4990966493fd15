"""CPU-only: the light table of the material renderer (include/render_mi355x.h "several lights") -- the host builder against its NumPy
restatement byte for byte and against the invariants the estimator needs, the entries' refusals (no GPU needed: the checks run before
any HIP call), the lamp helper, and the restatement tests/materials_ref.py with a table: equal to nee=True bit for bit with a one-light table,
equal to a closed form that does not depend on the library with three lights, and with the plain renderer's expectation."""
import ctypes

import numpy as np
import pytest

import lights_ref as lr
import materials_ref as mr

F = np.float32


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data
    pkg.gen_data = gen_data
    return pkg


def _scenes(apt):
    s9, m9 = apt.gen_data.gen_spheres_materials()
    return {"demo9": (s9, m9, 9, 7), "diff8": (apt.gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 8, 7)}


# ---- the table --------------------------------------------------------------------------------------------------------------------
def test_symbols_and_status_bit(apt):
    assert apt._lib.APT_DEV_LIGHTS_MISMATCH == 32 == lr.DEV_LIGHTS_MISMATCH
    text = open(mr.ROOT + "/include/render_mi355x.h").read()
    assert "APT_DEV_LIGHTS_MISMATCH = 32u" in text and "0x3C6EF372FE94F82B" in text and "0x4C474854" in text
    for name in ("apt_build_lights_host", "apt_lights_bytes", "apt_render_frame_lights", "apt_context_render_frame_lights",
                 "apt_render_paths_lights", "apt_context_render_paths_lights"):
        assert name in apt._lib.ABI_SYMBOLS and hasattr(apt._lib.lib(), name)


def test_the_selection_stream_is_a_fourth_one():
    paths = np.arange(4096, dtype=np.uint64)
    s1, _ = mr.uniforms(mr.light_key(7, paths), 0)
    for other in (mr.nee_key(7, paths), mr.mat_key(7, paths), mr.rr_key(7, paths)):
        o1, o2 = mr.uniforms(other, 0)
        assert not np.array_equal(s1, o1) and abs(float(np.corrcoef(s1, o1)[0, 1])) < 0.06 and abs(float(np.corrcoef(s1, o2)[0, 1])) < 0.06
    assert abs(float(s1.mean()) - 0.5) < 0.02
    assert len({int(mr.LIGHT_SALT), int(mr.NEE_SALT), 0x6A09E667F3BCC909}) == 3


def test_builder_equals_the_restatement_byte_for_byte(apt):
    gd = apt.gen_data
    sph8 = gd.gen_spheres()
    one = gd.build_lights(sph8, 8)                                          # NULL list: the stock light is the only emitter
    t = lr.check_table_invariants(one)
    assert one.dtype == np.uint32 and np.array_equal(one, lr.build_table(sph8, 8))
    assert t.n == 1 and t.idx.tolist() == [7] and t.cdf.tolist() == [1.0] and t.invp.tolist() == [1.0]
    assert one.nbytes == gd.lights_bytes(8, 1) == 4 * (16 + 3 + 1)
    sph2, _, _ = lr.two_lamps(apt.gen_data)
    for ind in (None, [6, 7], [7, 6], [0, 7, 3]):                            # unlisted order kept; a non-emitter gets the floor
        got = gd.build_lights(sph2, 8, ind)
        assert np.array_equal(got, lr.build_table(sph2, 8, ind)), ind
        t = lr.check_table_invariants(got)
        assert t.idx.tolist() == ([6, 7] if ind is None else ind)
    p = mr.Table(gd.build_lights(sph2, 8, [0, 7, 3])).prob()
    assert abs(p[0] - p[2]) <= 2.0 ** -24 and abs(p[0] - 1 / 6) < 2.0 ** -23 and abs(p[1] - 4 / 6) < 2.0 ** -23      # half by power (all sphere 7's), half uniform
    sph, _, ns, idx = lr.sixteen_lamps(apt.gen_data)
    got = gd.build_lights(sph, ns)                                          # NULL: the 16 lamps and the scene's own light
    assert np.array_equal(got, lr.build_table(sph, ns))
    t = lr.check_table_invariants(got)
    assert t.idx.tolist() == idx + [ns - 1] and got.nbytes == gd.lights_bytes(ns, 17)
    got = gd.build_lights(sph, ns, idx)
    assert np.array_equal(got, lr.build_table(sph, ns, idx))
    t = lr.check_table_invariants(got)
    p = t.prob()
    assert len(set(p.tolist())) == 16 and (p >= 0.5 / 16 - 2.0 ** -24).all() and abs(p.sum() - 1.0) == 0
    # every sphere of a scene listed: the size bound is exact, every probability at least the floor
    allk = gd.build_lights(sph, ns, list(range(ns)))
    assert np.array_equal(allk, lr.build_table(sph, ns, range(ns))) and allk.nbytes == gd.lights_bytes(ns, ns)
    assert (lr.check_table_invariants(allk).prob() >= 0.5 / ns - 2.0 ** -24).all()
    # no power at all: uniform
    dark = sph8.copy()
    dark[32:56] = 0
    t = lr.check_table_invariants(gd.build_lights(dark, 8, [1, 2, 3, 4]))
    assert t.prob().tolist() == [0.25] * 4 and np.array_equal(gd.build_lights(dark, 8, [1, 2, 3, 4]), lr.build_table(dark, 8, [1, 2, 3, 4]))


def test_builder_refusals(apt):
    L = apt._lib.lib()
    sph = apt.gen_data.gen_spheres()
    fp = sph.ctypes.data_as(ctypes.c_void_p)
    buf = np.full(64, 0xABABABAB, dtype=np.uint32)
    out = buf.ctypes.data_as(ctypes.c_void_p)
    nb = ctypes.c_size_t(77)
    u32 = ctypes.c_uint32

    def call(ind, ns=8, sp=fp, dst=out, cap=buf.nbytes):
        a = None if ind is None else (u32 * max(1, len(ind)))(*ind)
        return L.apt_build_lights_host(sp, u32(ns), a, u32(0 if ind is None else len(ind)), dst, ctypes.c_size_t(cap), ctypes.byref(nb))

    assert call([]) == 3 and b"empty" in L.apt_last_error()                     # APT_ERR_SCENE
    assert call([8]) == 3 and b"out of range" in L.apt_last_error()
    assert call([7, 3, 7]) == 3 and b"twice" in L.apt_last_error()
    assert call([7], dst=None) == 1 and call([7], sp=None) == 1                # APT_ERR_ARG
    assert call([7], ns=0) == 3
    dark = sph.copy()
    dark[32:56] = 0
    assert call(None, sp=dark.ctypes.data_as(ctypes.c_void_p)) == 3 and b"emits" in L.apt_last_error()
    assert nb.value == 77 and (buf == 0xABABABAB).all()                        # nothing written by any refusal so far
    assert call([6, 7], cap=91) == 1 and nb.value == 92 and (buf == 0xABABABAB).all() and b"capacity" in L.apt_last_error()
    assert call([6, 7], cap=92) == 0 and nb.value == 92 and buf[0] == lr.MAGIC and (buf[23:] == 0xABABABAB).all()
    with pytest.raises(apt.AptError):
        apt.gen_data.build_lights(sph, 8, [7, 7])
    with pytest.raises(apt.AptError):
        apt.gen_data.build_lights(sph, 8, [-1])
    with pytest.raises(ValueError):
        lr.build_table(sph, 8, [7, 7])


def test_entries_refuse_before_any_launch(apt):
    L = apt._lib.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first, or the range is empty
    u64 = ctypes.c_uint64
    frame = lambda q, mat=one, lt=one, c=10: L.apt_render_frame_lights(q, None, one, mat, lt, u64(0), u64(c), one, None)
    paths = lambda q, mat=one, lt=one: L.apt_render_paths_lights(q, None, one, one, mat, lt, one)
    ctx = L.apt_context_create()
    try:
        cframe = lambda q, lt=one, c=10: L.apt_context_render_frame_lights(ctypes.c_void_p(ctx), q, None, one, one, lt, u64(0), u64(c), one, None)
        cpaths = lambda q, lt=one: L.apt_context_render_paths_lights(ctypes.c_void_p(ctx), q, None, one, one, one, lt, one)
        ok = apt.make_params(16, 16, 1, light_index=7)
        for call in (frame, paths, cframe, cpaths):
            assert call(ctypes.byref(ok), lt=None) == 1                                  # APT_ERR_ARG
            assert b"lights" in L.apt_last_error()
        # the *_materials checks come first and keep their codes
        assert frame(ctypes.byref(ok), mat=None, lt=None) == 1 and b"materials" in L.apt_last_error()
        assert paths(ctypes.byref(ok), mat=None) == 1 and b"materials" in L.apt_last_error()
        o = apt.make_params(16, 16, 1, mode=apt.APT_MODE_ORACLE)
        assert frame(ctypes.byref(o)) == 1 and b"APT_MODE_KERNEL" in L.apt_last_error()
        assert frame(ctypes.byref(apt.make_params(16, 16, 1, accel=4096))) == 1 and b"APT_FLAG_GRID_SLOTS" in L.apt_last_error()
        assert frame(ctypes.byref(apt.make_params(16, 16, 1, light_index=9))) == 3 and b"out of range" in L.apt_last_error()
        assert frame(None) == 1 and L.apt_context_render_frame_lights(None, ctypes.byref(ok), None, one, one, one, u64(0), u64(0), one, None) == 1
        # neither APT_FLAG_NEE nor a light_index of -1 is read: empty ranges are no-ops, a range beyond the image is the range's own error
        no_light = apt.make_params(16, 16, 1, light_index=-1, flags=apt.APT_FLAG_NEE)
        assert frame(ctypes.byref(no_light), c=0) == 0 and cframe(ctypes.byref(no_light), c=0) == 0
        at_end = apt.make_params(16, 16, 1, light_index=-1, flags=apt.APT_FLAG_NEE | apt.APT_FLAG_RR, path_begin=1024)
        assert paths(ctypes.byref(at_end)) == 0 and cpaths(ctypes.byref(at_end)) == 0
        assert frame(ctypes.byref(ok), c=10 ** 9) == 1 and b"pixel range" in L.apt_last_error()
        assert paths(ctypes.byref(apt.make_params(16, 16, 1, path_begin=1025))) == 1
    finally:
        L.apt_context_destroy(ctypes.c_void_p(ctx))


def test_python_refuses_lights_without_materials(apt):
    import inspect
    from ascendpathtracing_amd import render
    for fn in (render.render_frame, render.render_do_ex, render.render_paths, render.Context.render_frame, render.Context.render_do_ex):
        assert "lights" in inspect.signature(fn).parameters
    with pytest.raises(apt.AptError, match="lights needs materials"):
        render._material_args("render_frame", apt.make_params(16, 16, 1), None, object())
    assert render._material_args("render_frame", apt.make_params(16, 16, 1), None, None) == ("render_frame", ())


def test_lamps_helper(apt):
    sph = apt.gen_data.gen_spheres()
    before = sph.copy()
    out = apt.gen_data.with_lamps(sph, 8, [6, 7], radius=[4.0, 1.5], centres=[(1.0, 2.0, 3.0), (50.0, 65.1, 81.6)], emission=[(60.0, 30.0, 15.0), 400.0])
    assert np.array_equal(sph, before) and out is not sph and out.dtype == np.float32 and out.shape == sph.shape
    a = out[:80].reshape(10, 8)
    assert a[:, 6].tolist() == [16.0, 1.0, 2.0, 3.0, 60.0, 30.0, 15.0, 0.0, 0.0, 0.0]
    step = apt.gen_data.with_lamp(apt.gen_data.with_lamp(sph, 8, 6, radius=4.0, centre=(1.0, 2.0, 3.0), emission=(60.0, 30.0, 15.0)), 8, 7)
    assert np.array_equal(out, step)                                           # built on with_lamp
    keep = apt.gen_data.with_lamps(sph, 8, [3], radius=2.0, emission=5.0)[:80].reshape(10, 8)
    assert keep[1:4, 3].tolist() == before[:80].reshape(10, 8)[1:4, 3].tolist() and keep[0, 3] == 4.0 and keep[4:7, 3].tolist() == [5.0] * 3
    for bad in ([7, 7], [8]):
        with pytest.raises(apt.AptError):
            apt.gen_data.with_lamps(sph, 8, bad)
    with pytest.raises(apt.AptError):
        apt.gen_data.with_lamps(sph, 8, [6, 7], radius=[1.0])


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["diff8", "demo9", "lamp8"])
def test_one_light_table_is_nee_ref_bit_for_bit(apt, scene):
    """table=a one-light table against nee=True on that light (the mode that tests/nee_ref.py once held): the same bits."""
    from oracle import oracle
    sph, mat, ns, light = _scenes(apt)["diff8" if scene == "lamp8" else scene]
    if scene == "lamp8":
        sph = apt.gen_data.with_lamp(sph, ns, light)
    table = apt.gen_data.build_lights(sph, ns, [light])
    for depth in (1, 2, 5):
        for rr in (0, 2):
            p = oracle.make_params(16, 12, 2, depth=depth, num_spheres=ns, light_index=light, seed=3 + depth)
            rays = oracle.gen_rays_counter(p)
            paths = np.arange(rays.shape[1], dtype=np.uint64)
            want, bad_w, seg_w = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, rr_start=rr, light=light, nee=True, gloss=False)
            got, bad, seg = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, rr_start=rr, table=table, gloss=False)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (depth, rr)
            assert np.array_equal(bad, bad_w) and seg == seg_w
    p = oracle.make_params(8, 8, 1, depth=4, num_spheres=ns, light_index=light, seed=1, flags=mr.FLAG_NEE)
    fb, u8, _, _ = mr.render_frame(p, sph, mat, table=table)
    fb_w, u8_w, _, _ = mr.render_frame(p, sph, mat)
    assert np.array_equal(fb.view(np.uint32), fb_w.view(np.uint32)) and np.array_equal(u8, u8_w)


def test_the_standing_sphere_is_never_sampled(apt):
    """The white furnace (albedo 0.5, emission 0.25 everywhere inside one sphere) listed as the only light: S is false at every bounce
    (we stand on it), so every colour is the plain renderer's, bit for bit, and exactly 0.5 (1 - 2^-D)."""
    from oracle import oracle
    sph, mat, _ = lr.furnace(False)
    table = apt.gen_data.build_lights(sph, 1)
    for depth in (1, 4, 9):
        p = oracle.make_params(16, 12, 2, depth=depth, num_spheres=1, light_index=0, seed=5, eps=0.5)
        rays = oracle.gen_rays_counter(p)
        paths = np.arange(rays.shape[1], dtype=np.uint64)
        got, _, seg = mr.trace(rays, sph, mat, 1, depth, p.eps, p.seed, paths, table=table, gloss=False)
        want, _, _ = mr.trace(rays, sph, mat, 1, depth, p.eps, p.seed, paths, gloss=False)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and seg == depth * paths.size
        assert (got == F(0.5 * (1 - 2.0 ** -depth))).all()


@pytest.mark.parametrize("j", range(8))
def test_closed_form_lambertian_point_under_three_lights(apt, j):
    """Independent of the library and of the estimator: a Lambertian point that sees two whole unoccluded sphere lights above its
    horizon (and none of a third below it) reflects sum_j albedo * Le_j * (r_j / dist_j)^2 * cos(theta_j).  Depth 2, so the second
    hit exercises the leave-out rule for whichever light was or was not chosen."""
    per = 4096
    rays, sph, mat, ns, paths, want = lr.three_lights_point(j, per)
    table = lr.build_table(sph, ns, [1, 2, 3])
    assert np.array_equal(table, apt.gen_data.build_lights(sph, ns))
    L, bad, _ = mr.trace(rays, sph, mat, ns, 2, 1e-4, 7, paths, table=table, gloss=False)
    assert not bad.any()
    for ch in range(3):
        x = L[ch].astype(np.float64)
        sigma = x.std(ddof=1) / np.sqrt(per)
        print("x = %4.1f ch %d  closed form %.6f  mean %.6f  sigma %.3e  z %+.2f" % (2.0 * j - 6.0, ch, want[ch], x.mean(), sigma, (x.mean() - want[ch]) / sigma))
        assert sigma > 0 and abs(x.mean() - want[ch]) < 4 * sigma


def test_closed_form_plain_renderer_agrees_too():
    """The plain renderer on the same scene has the same expectation (with far more noise): the closed form is the scene's."""
    per = 1 << 16
    rays, sph, mat, ns, paths, want = lr.three_lights_point(2, per)
    L, _, _ = mr.trace(rays, sph, mat, ns, 2, 1e-4, 7, paths, gloss=False)
    for ch in range(3):
        x = L[ch].astype(np.float64)
        sigma = x.std(ddof=1) / np.sqrt(per)
        assert sigma > 0 and abs(x.mean() - want[ch]) < 4 * sigma


@pytest.mark.parametrize("depth", [2, 5])
def test_same_expectation_and_less_variance_on_the_restatement(apt, depth):
    """Two lamps, 2^15 camera rays: per channel the table's mean is the plain renderer's within 4 sigma; and over the paths whose camera
    ray hits no lamp its variance is below the plain renderer's and below APT_FLAG_NEE's sampling either lamp alone."""
    from oracle import oracle
    sph, mat, ns = lr.two_lamps(apt.gen_data)
    table = apt.gen_data.build_lights(sph, ns)
    p = oracle.make_params(64, 32, 4, depth=depth, num_spheres=ns, light_index=7, seed=21)
    rays = oracle.gen_rays_counter(p)
    n = rays.shape[1]
    paths = np.arange(n, dtype=np.uint64)
    on = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, table=table, gloss=False)[0].astype(np.float64)
    off = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, gloss=False)[0].astype(np.float64)
    first = mr.trace(rays, sph, mat, ns, 1, p.eps, p.seed, paths, gloss=False)[0].any(axis=0)
    nee = [mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, light=l, nee=True, gloss=False)[0].astype(np.float64) for l in (6, 7)]
    for ch in range(3):
        s_on, s_off = on[ch].std(ddof=1) / np.sqrt(n), off[ch].std(ddof=1) / np.sqrt(n)
        z = (on[ch].mean() - off[ch].mean()) / np.hypot(s_on, s_off)
        v = [a[ch][~first].var(ddof=1) for a in (on, off, *nee)]
        print("depth %d channel %d: on %.5f off %.5f z %+.2f   variance plain / table %.1f  nee(6) / table %.1f  nee(7) / table %.1f"
              % (depth, ch, on[ch].mean(), off[ch].mean(), z, v[1] / v[0], v[2] / v[0], v[3] / v[0]))
        assert s_on > 0 and s_off > 0 and abs(z) < 4
        assert v[0] < v[1] and v[0] < v[2] and v[0] < v[3]
