"""CPU-only: the arithmetic pieces of the material renderer's contract (include/render_mi355x.h "per-sphere materials") as
tests/materials_ref.py restates them, the demo scene helper, and the argument checks of the new entries (no GPU needed)."""
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


def test_sincos_polynomial_over_every_input():
    u1 = np.arange(1 << 24, dtype=np.uint32).astype(F) * F(2.0 ** -24)
    sn, cs = mr.sincos(u1)
    phi = 2 * np.pi * u1.astype(np.float64)
    assert np.abs(sn - np.sin(phi)).max() <= 2.0 ** -22
    assert np.abs(cs - np.cos(phi)).max() <= 2.0 ** -22
    s2c2 = sn.astype(np.float64) ** 2 + cs.astype(np.float64) ** 2
    assert np.abs(s2c2 - 1).max() <= 2.0 ** -21
    assert sn[0] == 0 and cs[0] == 1 and cs[1 << 22] == 0 and sn[1 << 22] == 1     # quadrant starts are exact


def test_duff_basis_is_orthonormal():
    rng = np.random.default_rng(0)
    v = rng.normal(size=(3, 200000))
    v[:, :4] = [[0, 0, 0, 1e-9], [0, 0, 1, 0], [1, -1, 0, -1]]   # poles, an equator point, near the seam
    n = (v / np.linalg.norm(v, axis=0)).astype(F)
    t, b = mr.basis(*n)
    t, b, n64 = np.array(t, np.float64), np.array(b, np.float64), n.astype(np.float64)
    for x, y in ((t, b), (t, n64), (b, n64)):
        assert np.abs((x * y).sum(axis=0)).max() < 1e-5
    for x in (t, b):
        assert np.abs((x * x).sum(axis=0) - 1).max() < 1e-5
    cr = np.cross(t.T, b.T).T                                   # right-handed frame (t, b, n)
    assert np.abs(cr - n64).max() < 1e-5


def test_fresnel():
    re, tr = mr.fresnel(np.array([0.0], F))                     # normal incidence: c = 0
    assert re[0] == F(0.04) and tr[0] == F(1) - F(0.04)
    c = np.linspace(0, 1, 100001).astype(F)
    re, tr = mr.fresnel(c)
    assert (re + tr == F(1)).all() or np.abs(re.astype(np.float64) + tr - 1).max() <= 2.0 ** -24
    assert (np.diff(re) >= 0).all() and re[-1] == F(1)


def test_uniform_streams_are_separate():
    key = mr.mat_key(7, np.arange(4096, dtype=np.uint64))
    u1, u2 = mr.uniforms(key, 0)
    assert u1.dtype == np.float32 and (u1 >= 0).all() and (u1 < 1).all() and (u2 < 1).all()
    rr = mr.splitmix64(mr.rr_key(7, np.arange(4096, dtype=np.uint64)) + np.uint64(0x9E3779B97F4A7C15))
    assert not np.array_equal((rr >> np.uint64(40)).astype(F) * F(2.0 ** -24), u1)
    assert abs(float(u1.mean()) - 0.5) < 0.02 and abs(float(u2.mean()) - 0.5) < 0.02


def _furnace_table(albedo, emission):
    rows = np.array([[1000.0 ** 2, 50.0, 52.0, 295.6, emission, emission, emission, albedo, albedo, albedo]])
    out = np.zeros(128, F)
    out[:10] = rows.T.astype(F).ravel()
    return out


def test_furnace_on_the_restatement():
    from oracle import oracle
    for depth in (1, 2, 5, 8):
        p = oracle.make_params(8, 8, 2, depth=depth, num_spheres=1, light_index=-1, eps=0.5, seed=depth)
        rays = oracle.gen_rays_counter(p)
        n = rays.shape[1]
        L, bad, _ = mr.trace(rays, _furnace_table(1.0, 1.0), np.array([mr.DIFF]), 1, depth, 0.5, p.seed, np.arange(n, dtype=np.uint64), gloss=False)
        assert not bad.any() and (L == F(depth)).all()
        fb, _, _, _ = mr.render_frame(p, _furnace_table(0.5, 0.25), np.array([mr.DIFF]))
        assert (fb == F(0.5 * (1 - 2.0 ** -depth))).all()


def test_restatement_stays_float32():
    with pytest.raises(AssertionError):
        mr.f32(np.zeros(2, np.float64))
    from oracle import oracle
    p = oracle.make_params(4, 4, 1, depth=3)
    rays = oracle.gen_rays_counter(p)
    sph = oracle.gen_spheres()
    L, _, _ = mr.trace(rays, sph, np.array([1, 1, 1, 1, 1, 1, 0, 2]), 8, 3, 1e-4, 0, np.arange(rays.shape[1], dtype=np.uint64), rr_start=1, gloss=False)
    assert L.dtype == np.float32


def test_demo_scene_helper(apt):
    sph, mat = apt.gen_data.gen_spheres_materials()
    assert sph.shape == (128,) and sph.dtype == np.float32 and not sph[90:].any()
    planes = sph[:90].reshape(10, 9)
    ref = apt.gen_data.gen_spheres()[:80].reshape(10, 8)         # gen_data.py:94-102 (via the existing, golden-tested gen_spheres)
    assert np.array_equal(planes[:, :8], ref)
    want8 = np.array([16.5 ** 2, 73, 16.5, 78, 0, 0, 0, 0.999, 0.999, 0.999], dtype=np.float64).astype(F)
    assert np.array_equal(planes[:, 8], want8)
    assert planes[0, 0] == F(1e10) and planes[4, 7] == F(12) and planes[1, 6] == F(27)     # a wall, the light, the mirror
    assert mat.tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 2]
    assert (apt.MAT_SPEC, apt.MAT_DIFF, apt.MAT_REFR) == (0, 1, 2)


def test_materials_argument_validation_needs_no_gpu(apt):
    L = apt._lib.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first
    p = apt.make_params(16, 16, 1)
    u64 = ctypes.c_uint64
    frame = lambda q, mat=one, sph=one, b=0, c=10, fb=one: L.apt_render_frame_materials(q, None, sph, mat, u64(b), u64(c), fb, None)
    paths = lambda q, mat=one, rays=one: L.apt_render_paths_materials(q, None, rays, one, mat, one)
    bad = apt.make_params(16, 16, 1); bad.struct_size = 8
    assert frame(ctypes.byref(bad)) == 2 and paths(ctypes.byref(bad)) == 2                    # APT_ERR_STRUCT
    assert frame(None) == 1 and paths(None) == 1
    assert frame(ctypes.byref(p), mat=None) == 1 and b"materials" in L.apt_last_error()
    assert paths(ctypes.byref(p), mat=None) == 1
    o = apt.make_params(16, 16, 1, mode=apt.APT_MODE_ORACLE)
    assert frame(ctypes.byref(o)) == 1 and b"APT_MODE_KERNEL" in L.apt_last_error()
    assert paths(ctypes.byref(o)) == 1
    g = apt.make_params(16, 16, 1, num_spheres=9, accel=4096)
    assert frame(ctypes.byref(g)) == 1 and b"accel" in L.apt_last_error()
    assert paths(ctypes.byref(g)) == 1
    assert frame(ctypes.byref(p), b=0, c=10 ** 9) == 1                                      # pixel range beyond the image
    assert frame(ctypes.byref(p), sph=None) == 1 and frame(ctypes.byref(p), fb=None) == 1
    assert paths(ctypes.byref(apt.make_params(16, 16, 1, path_begin=1000, path_count=100))) == 1
    assert paths(ctypes.byref(p), rays=None) == 1
    assert frame(ctypes.byref(apt.make_params(16, 16, 1, light_index=9))) == 3              # check_params' scene rules still apply
    assert frame(ctypes.byref(apt.make_params(16, 16, 1 << 20))) == 1                       # no pairwise plan
    assert frame(ctypes.byref(p), c=0) == 0                                                  # empty ranges are no-ops
    assert paths(ctypes.byref(apt.make_params(16, 16, 1, path_begin=1024))) == 0
    ctx = L.apt_context_create()
    try:
        assert L.apt_context_render_frame_materials(ctypes.c_void_p(ctx), ctypes.byref(o), None, one, one, u64(0), u64(1), one, None) == 1
        assert L.apt_context_render_paths_materials(ctypes.c_void_p(ctx), ctypes.byref(bad), None, one, one, one, one) == 2
        assert L.apt_context_render_frame_materials(None, ctypes.byref(p), None, one, one, u64(0), u64(1), one, None) == 1
    finally:
        L.apt_context_destroy(ctypes.c_void_p(ctx))
    # APT_FLAG_EMISSION with light_index -1 is accepted by the material entries (refused by the mirror entries, unchanged)
    em = apt.make_params(16, 16, 1, light_index=-1, flags=apt.APT_FLAG_EMISSION)
    assert L.render_frame(ctypes.byref(em), None, one, u64(0), u64(1), one, None) == 3
    assert frame(ctypes.byref(em), c=0) == 0
    assert L.apt_gen_spheres_materials_host(None, None) == 1
