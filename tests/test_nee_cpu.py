"""CPU-only: direct light sampling (APT_FLAG_NEE, include/render_mi355x.h "Direct light sampling") -- the flag and the entries'
argument checks (no GPU needed), the lamp helper, and the restatement tests/materials_ref.py with nee=True: with the flag off a light
index changes nothing, bit for bit; with it on, equal to a closed form that does not depend on the library with it on, and with the plain renderer's expectation."""
import ctypes

import numpy as np
import pytest

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


def test_flag_value(apt):
    assert apt.APT_FLAG_NEE == 32 == mr.FLAG_NEE and "APT_FLAG_NEE" in apt.__all__
    text = open(mr.ROOT + "/include/render_mi355x.h").read()
    assert "APT_FLAG_NEE = 32u" in text
    others = (apt.APT_FLAG_RETIRE, apt.APT_FLAG_RR, apt.APT_FLAG_EMISSION, apt.APT_FLAG_BAND_BUFFERS, apt.APT_FLAG_GRID_SLOTS)
    assert all(apt.APT_FLAG_NEE & f == 0 for f in others)


def test_entries_refuse_the_flag_without_a_light_and_need_no_gpu(apt):
    L = apt._lib.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first, or the range is empty
    u64 = ctypes.c_uint64
    frame = lambda q, mat=one, c=10: L.apt_render_frame_materials(q, None, one, mat, u64(0), u64(c), one, None)
    paths = lambda q, mat=one: L.apt_render_paths_materials(q, None, one, one, mat, one)
    ctx = L.apt_context_create()
    try:
        cframe = lambda q, c=10: L.apt_context_render_frame_materials(ctypes.c_void_p(ctx), q, None, one, one, u64(0), u64(c), one, None)
        cpaths = lambda q: L.apt_context_render_paths_materials(ctypes.c_void_p(ctx), q, None, one, one, one, one)
        no_light = apt.make_params(16, 16, 1, light_index=-1, flags=apt.APT_FLAG_NEE)
        for call in (frame, paths, cframe, cpaths):
            assert call(ctypes.byref(no_light)) == 3                                   # APT_ERR_SCENE
            msg = L.apt_last_error()
            assert b"APT_FLAG_NEE" in msg and b"light_index" in msg
        # every existing refusal keeps its code: the flag's rule comes after check_params' and check_materials'
        assert frame(ctypes.byref(no_light), mat=None) == 1 and b"materials" in L.apt_last_error()
        assert paths(ctypes.byref(no_light), mat=None) == 1
        o = apt.make_params(16, 16, 1, light_index=-1, flags=apt.APT_FLAG_NEE, mode=apt.APT_MODE_ORACLE)
        assert frame(ctypes.byref(o)) == 1 and b"APT_MODE_KERNEL" in L.apt_last_error()
        assert frame(ctypes.byref(apt.make_params(16, 16, 1, light_index=9, flags=apt.APT_FLAG_NEE))) == 3
        assert b"out of range" in L.apt_last_error()
        # with a valid index the flag is accepted: empty ranges are no-ops, a range beyond the image is the range's own error
        ok = apt.make_params(16, 16, 1, light_index=7, flags=apt.APT_FLAG_NEE)
        assert frame(ctypes.byref(ok), c=0) == 0 and cframe(ctypes.byref(ok), c=0) == 0
        begin_at_end = apt.make_params(16, 16, 1, light_index=7, flags=apt.APT_FLAG_NEE | apt.APT_FLAG_RR, path_begin=1024)
        assert paths(ctypes.byref(begin_at_end)) == 0 and cpaths(ctypes.byref(begin_at_end)) == 0
        assert frame(ctypes.byref(ok), c=10 ** 9) == 1
        # without the flag a light_index of -1 stays accepted, and the mirror entries ignore the bit
        assert frame(ctypes.byref(apt.make_params(16, 16, 1, light_index=-1)), c=0) == 0
        assert L.render_frame(ctypes.byref(no_light), None, one, u64(0), u64(0), one, None) == 0
    finally:
        L.apt_context_destroy(ctypes.c_void_p(ctx))


def test_lamp_helper(apt):
    want = np.array([1.5 ** 2, 50.0, 81.6 - 16.5, 81.6, 400, 400, 400, 0, 0, 0], dtype=np.float64).astype(F)
    for sph, ns, light in ((apt.gen_data.gen_spheres(), 8, 7), (apt.gen_data.gen_spheres_materials()[0], 9, 7),
                           (apt.gen_data.gen_scene(1030, seed=5), 1030, 1029)):
        before = sph.copy()
        out = apt.gen_data.with_lamp(sph, ns, light)
        assert np.array_equal(sph, before) and out is not sph                       # a copy
        assert out.shape == sph.shape and out.dtype == np.float32
        a, b = out[:10 * ns].reshape(10, ns), sph[:10 * ns].reshape(10, ns)
        assert np.array_equal(a[:, light], want)
        keep = np.arange(ns) != light
        assert np.array_equal(a[:, keep], b[:, keep]) and np.array_equal(out[10 * ns:], sph[10 * ns:])
    out = apt.gen_data.with_lamp(apt.gen_data.gen_spheres(), 8, 7, radius=8.0, centre=(1.0, 2.0, 3.0), emission=(40.0, 30.0, 20.0))
    assert out[:80].reshape(10, 8)[:, 7].tolist() == [64.0, 1.0, 2.0, 3.0, 40.0, 30.0, 20.0, 0.0, 0.0, 0.0]
    with pytest.raises(apt.AptError):
        apt.gen_data.with_lamp(apt.gen_data.gen_spheres(), 8, 8)


def _scenes(apt):
    s9, m9 = apt.gen_data.gen_spheres_materials()
    return {"demo9": (s9, m9, 9, 7), "diff8": (apt.gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 8, 7)}


@pytest.mark.parametrize("scene", ["demo9", "diff8"])
def test_flag_off_is_the_plain_renderer_bit_for_bit(apt, scene):
    """nee=False with a light index given against the same call without one (the plain renderer, whose bytes
    tests/test_restatement_frozen.py records)."""
    from oracle import oracle
    sph, mat, ns, light = _scenes(apt)[scene]
    for depth, rr in ((1, 0), (5, 0), (8, 2)):
        p = oracle.make_params(16, 12, 2, depth=depth, num_spheres=ns, light_index=light, seed=3 + depth)
        rays = oracle.gen_rays_counter(p)
        paths = np.arange(rays.shape[1], dtype=np.uint64)
        want, bad_w, _ = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, rr_start=rr, gloss=False)
        got, bad, seg = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, rr_start=rr, light=light, nee=False, gloss=False)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(bad, bad_w) and seg > 0
        on, _, seg_on = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, rr_start=rr, light=light, nee=True, gloss=False)
        if depth == 1:                                   # no sample at the last bounce: depth 1 has no other
            assert np.array_equal(on.view(np.uint32), want.view(np.uint32)) and seg_on == seg
        else:
            assert not np.array_equal(on, want) and seg_on > seg and on.dtype == np.float32
    p = oracle.make_params(8, 8, 1, depth=4, num_spheres=ns, light_index=light, seed=1)
    fb, u8, _, _ = mr.render_frame(p, sph, mat)
    fb_w, u8_w, _, _ = mr.render_frame(oracle.make_params(8, 8, 1, depth=4, num_spheres=ns, light_index=-1, seed=1), sph, mat)
    assert np.array_equal(fb.view(np.uint32), fb_w.view(np.uint32)) and np.array_equal(u8, u8_w)


def test_the_sampling_stream_is_a_third_one():
    paths = np.arange(4096, dtype=np.uint64)
    v1, v2 = mr.uniforms(mr.nee_key(7, paths), 0)
    u1, u2 = mr.uniforms(mr.mat_key(7, paths), 0)
    r1, _ = mr.uniforms(mr.rr_key(7, paths), 0)
    assert not np.array_equal(v1, u1) and not np.array_equal(v1, r1) and not np.array_equal(v2, u2)
    assert abs(float(v1.mean()) - 0.5) < 0.02 and abs(float(v2.mean()) - 0.5) < 0.02
    assert abs(float(np.corrcoef(v1, u1)[0, 1])) < 0.06 and abs(float(np.corrcoef(v2, u2)[0, 1])) < 0.06


def test_sampled_directions_stay_inside_the_cone():
    """Every sampled direction lies in the cone the light subtends (to fp32 accuracy), near and far, and the far lamp keeps a
    non-zero solid angle (what x / (1 + cmax) is for)."""
    rng = np.random.default_rng(0)
    n = 50000
    lc, r = [F(50), F(65.1), F(81.6)], 1.5
    for dist in (1.6, 20.0, 3000.0):
        u = rng.normal(size=(3, n))
        u /= np.linalg.norm(u, axis=0)
        h = [(np.float64(lc[i]) + dist * u[i]).astype(F) for i in range(3)]
        nl = [(-u[i]).astype(F) for i in range(3)]                                # facing the light
        ok, l, cosl, wgt = mr.light_sample(h, nl, mr.nee_key(1, np.arange(n, dtype=np.uint64)), 0, lc, F(r * r))
        assert ok.all() and (wgt > 0).all()
        w = np.stack([np.float64(lc[i]) - h[i].astype(np.float64) for i in range(3)])
        d = np.linalg.norm(w, axis=0)
        cos_to_centre = (np.stack(l).astype(np.float64) * w).sum(axis=0) / d
        cos_max = np.sqrt(np.maximum(0.0, 1 - (r / d) ** 2))
        assert (cos_to_centre >= cos_max - 1e-5).all()
        assert np.abs(np.linalg.norm(np.stack(l).astype(np.float64), axis=0) - 1).max() < 1e-6
        # mean of wgt = E[cos] * omega / pi ~ (r / d)^2 for a light seen head-on
        assert abs(float(wgt.astype(np.float64).mean()) / (r / d.mean()) ** 2 - 1) < 0.05


def _table(rows):
    rows = np.array(rows, dtype=np.float64)
    rows[:, 0] = rows[:, 0] ** 2
    ns = rows.shape[0]
    out = np.zeros((ns * 10 + 127) // 128 * 128, dtype=np.float32)
    out[:10 * ns] = rows.T.astype(np.float32).ravel()
    return out


def _floor_and_lamp_point(j, per, nee=True, rule=True):
    """One point of the closed-form scene -> (the `per` radiances, the closed form)."""
    R, r, Le, alb, height = 1000.0, 2.0, 50.0, 0.75, 10.0
    sph = _table([[R, 0, -R, 0, 0, 0, 0, alb, alb, alb], [r, 0, height, 0, Le, Le, Le, 0, 0, 0]])
    mat = np.array([mr.DIFF, mr.DIFF], dtype=np.int32)
    px = 3.0 * j
    tgt = np.array([px, np.sqrt(R * R - px * px) - R, 0.0])                           # on the floor sphere
    o = tgt + np.array([0.0, 5.0, 0.5])
    dd = (tgt - o) / np.linalg.norm(tgt - o)
    rays = np.tile(np.concatenate([o, dd])[:, None], (1, per)).astype(F)
    paths = np.arange(j * per, (j + 1) * per, dtype=np.uint64)
    L, bad, _ = mr.trace(rays, sph, mat, 2, 2, 1e-4, 7, paths, light=1, nee=nee, gloss=False)
    assert not bad.any()
    nrm = (tgt - np.array([0.0, -R, 0.0])) / R
    w = np.array([0.0, height, 0.0]) - tgt
    dist = np.linalg.norm(w)
    return L[0].astype(np.float64), alb * Le * (r / dist) ** 2 * (w @ nrm) / dist


@pytest.mark.parametrize("j", range(8))
def test_closed_form_lambertian_point_under_a_sphere_light(j):
    """Independent of the library: a Lambertian point that sees a whole unoccluded sphere light above its horizon reflects exactly
    albedo * Le * (r / dist)^2 * cos(theta).  Depth 2, so the second hit exercises "do not count the light again"."""
    per = 4096
    L, want = _floor_and_lamp_point(j, per)
    sigma = L.std(ddof=1) / np.sqrt(per)
    print("x = %4.1f  closed form %.6f  mean %.6f  sigma %.3e  z %.2f" % (3.0 * j, want, L.mean(), sigma, (L.mean() - want) / sigma))
    assert sigma > 0
    assert abs(L.mean() - want) < 4 * sigma


def test_closed_form_plain_renderer_agrees_too():
    """The plain renderer on the same scene has the same expectation (with far more noise): the closed form is the scene's, not the
    estimator's."""
    per = 1 << 16
    L, want = _floor_and_lamp_point(2, per, nee=False)
    sigma = L.std(ddof=1) / np.sqrt(per)
    assert sigma > 0 and abs(L.mean() - want) < 4 * sigma


@pytest.mark.parametrize("lamp,depth", [(False, 2), (True, 5)])
def test_same_expectation_on_the_restatement(apt, lamp, depth):
    """The flag changes the image by noise only: per channel, the means with and without it differ by less than 4 sigma."""
    from oracle import oracle
    sph, mat, ns, light = _scenes(apt)["diff8"]
    if lamp:
        sph = apt.gen_data.with_lamp(sph, ns, light)
    p = oracle.make_params(64, 32, 4, depth=depth, num_spheres=ns, light_index=light, seed=21)
    rays = oracle.gen_rays_counter(p)
    paths = np.arange(rays.shape[1], dtype=np.uint64)
    on = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, light=light, nee=True, gloss=False)[0].astype(np.float64)
    off = mr.trace(rays, sph, mat, ns, depth, p.eps, p.seed, paths, light=light, nee=False, gloss=False)[0].astype(np.float64)
    n = rays.shape[1]
    for ch in range(3):
        s_on, s_off = on[ch].std(ddof=1) / np.sqrt(n), off[ch].std(ddof=1) / np.sqrt(n)
        z = (on[ch].mean() - off[ch].mean()) / np.hypot(s_on, s_off)
        print("lamp %s depth %d channel %d: on %.5f off %.5f z %.2f" % (lamp, depth, ch, on[ch].mean(), off[ch].mean(), z))
        assert s_on > 0 and s_off > 0 and abs(z) < 4
