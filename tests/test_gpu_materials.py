"""GPU: the per-sphere material renderer (include/render_mi355x.h "per-sphere materials") bit for bit against its NumPy restatement
(tests/materials_ref.py), and against analytic furnace values that do not depend on the restatement."""
import ctypes

import numpy as np
import pytest

import materials_ref as mr
from gpu_harness import Scene, apt, dev, oracle_params, scene  # noqa: F401

pytestmark = pytest.mark.gpu

CAMERA = (50.0, 52.0, 295.6)     # camera_init: the camera position of gen_rays


def _table(cols):
    """[ns][10] rows (r, cx, cy, cz, em*3, albedo*3) -> the padded [10][ns] table (r -> r^2 in float64, like gen_spheres)."""
    rows = np.array(cols, dtype=np.float64)
    rows[:, 0] = rows[:, 0] ** 2
    ns = rows.shape[0]
    out = np.zeros((ns * 10 + 127) // 128 * 128, dtype=np.float32)
    out[:10 * ns] = rows.T.astype(np.float32).ravel()
    return out


def _scene(apt, name):
    """-> (spheres, materials int32, light_index)"""
    if name == "big1030":                             # > one 1024-sphere tile: random codes, every 5th small sphere glass
        ns = 1030
        s = apt.gen_data.gen_scene(ns, seed=5)
        rng = np.random.default_rng(7)
        m = rng.integers(0, 3, ns).astype(np.int32)
        m[6:ns - 1:5] = 2
        m[:6] = 1
        m[ns - 1] = 1
        return s, m, ns - 1
    sc = scene(apt, name + "-stock")                  # demo9: the tile form, diff8: the 8-sphere form
    return sc.sph, sc.mat, sc.light


def _frame_gpu(apt, p, sph, mat, pixel_begin=0, pixel_count=None, u8="normal"):
    import torch
    L = apt._lib.lib()
    npix = p.width * p.height
    pc = npix - pixel_begin if pixel_count is None else pixel_count
    d_sph, d_mat = dev(sph), dev(mat, np.int32)
    fb = torch.full((3, pc), float("nan"), dtype=torch.float32, device="cuda")
    raw = torch.zeros(pc * 3 + 4, dtype=torch.uint8, device="cuda")
    off = 1 if u8 == "misaligned" else 0
    u8_ptr = None if u8 == "null" else ctypes.c_void_p(raw.data_ptr() + off)
    rc = L.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(d_sph.data_ptr()), ctypes.c_void_p(d_mat.data_ptr()),
                                      ctypes.c_uint64(pixel_begin), ctypes.c_uint64(pc), ctypes.c_void_p(fb.data_ptr()), u8_ptr)
    apt._lib.check(rc, "apt_render_frame_materials")
    torch.cuda.synchronize()
    return fb.cpu().numpy(), raw[off:off + 3 * pc].cpu().numpy().reshape(pc, 3)


# (136, 3): two pairwise leaves (64 + 72, no tail), combined through the LDS stack
FRAME_CASES = [(s_, d_, rr) for (s_, d_) in ((1, 1), (3, 2), (8, 5), (13, 8), (32, 32), (8, 32), (32, 5), (3, 8), (136, 3)) for rr in (False, True)]


@pytest.mark.parametrize("scene", ["demo9", "diff8"])
@pytest.mark.parametrize("s_,depth,rr", FRAME_CASES)
def test_frame_bitwise(apt, scene, s_, depth, rr):
    sph, mat, light = _scene(apt, scene)
    ns = mat.size
    p = apt.make_params(48, 32, s_, depth=depth, num_spheres=ns, light_index=light, seed=11 + s_,
                        flags=apt.APT_FLAG_RR if rr else 0, rr_start=2 if rr else 0)
    fb, u8 = _frame_gpu(apt, p, sph, mat)
    fb_w, u8_w, bad, _ = mr.render_frame(oracle_params(p), sph, mat)
    assert not bad.any()
    assert np.array_equal(fb.view(np.uint32), fb_w.view(np.uint32)), np.argwhere(fb.view(np.uint32) != fb_w.view(np.uint32))[:5]
    assert np.array_equal(u8, u8_w)


@pytest.mark.parametrize("s_,depth,rr", [(1, 2, False), (8, 5, True), (3, 1, False)])
def test_frame_bitwise_large_scene(apt, s_, depth, rr):
    sph, mat, light = _scene(apt, "big1030")
    p = apt.make_params(24, 16, s_, depth=depth, num_spheres=mat.size, light_index=light, seed=3,
                        flags=apt.APT_FLAG_RR if rr else 0, rr_start=1 if rr else 0)
    fb, u8 = _frame_gpu(apt, p, sph, mat)
    fb_w, u8_w, _, _ = mr.render_frame(oracle_params(p), sph, mat)
    assert np.array_equal(fb.view(np.uint32), fb_w.view(np.uint32))
    assert np.array_equal(u8, u8_w)


@pytest.mark.parametrize("scene", ["demo9", "diff8"])
@pytest.mark.parametrize("u8", ["null", "misaligned"])
def test_frame_pixel_range_and_u8_forms(apt, scene, u8):
    sph, mat, light = _scene(apt, scene)
    p = apt.make_params(48, 32, 16, depth=5, num_spheres=mat.size, light_index=light, seed=2, flags=apt.APT_FLAG_RETIRE)
    b, c = 517, 700
    fb, got8 = _frame_gpu(apt, p, sph, mat, b, c, u8=u8)
    fb_w, u8_w, _, _ = mr.render_frame(oracle_params(p), sph, mat, pixel_begin=b, pixel_count=c)
    assert np.array_equal(fb.view(np.uint32), fb_w.view(np.uint32))
    if u8 == "misaligned":
        assert np.array_equal(got8, u8_w)
    else:
        assert not got8.any()


def _paths_gpu(apt, p, rays, sph, mat):
    return Scene(apt, sph, mat, mat.size).paths(p, rays)


@pytest.mark.parametrize("scene", ["demo9", "diff8"])
def test_paths_bitwise_with_ranges(apt, scene):
    from oracle import oracle
    sph, mat, light = _scene(apt, scene)
    p = apt.make_params(16, 16, 4, depth=8, num_spheres=mat.size, light_index=light, seed=9, flags=apt.APT_FLAG_RR, rr_start=3)
    rays = oracle.gen_rays_counter(oracle_params(p))
    n = rays.shape[1]
    want, bad, _ = mr.trace(rays, sph, mat, mat.size, 8, p.eps, p.seed, np.arange(n, dtype=np.uint64), rr_start=3, gloss=False)
    assert not bad.any()
    got = _paths_gpu(apt, p, rays, sph, mat)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    b, c = 1001, 1537                                 # a path range of the whole-image buffers, then the same range in band buffers
    pr = p.copy(path_begin=b, path_count=c)
    got = _paths_gpu(apt, pr, rays, sph, mat)
    assert np.array_equal(got[:, b:b + c].view(np.uint32), want[:, b:b + c].view(np.uint32))
    assert np.isnan(got[:, :b]).all() and np.isnan(got[:, b + c:]).all()
    pb = p.copy(path_begin=b, path_count=c, flags=p.flags | apt.APT_FLAG_BAND_BUFFERS)
    got = _paths_gpu(apt, pb, np.ascontiguousarray(rays[:, b:b + c]), sph, mat)
    assert np.array_equal(got.view(np.uint32), want[:, b:b + c].view(np.uint32))


def _handmade_rays(n):
    """Rays at the demo scene's glass ball (centre (73, 16.5, 78), r 16.5) and mirror: normal incidence from outside, from inside
    towards the surface at angles past the critical one (total internal reflection), and grazing the rim."""
    rng = np.random.default_rng(1)
    c = np.array([73.0, 16.5, 78.0])
    rays = np.zeros((6, n))
    for i in range(n):
        kind = i % 4
        if kind == 0:      # normal incidence from outside
            d = rng.normal(size=3); d /= np.linalg.norm(d)
            o, dd = c + d * 40.0, -d
        elif kind == 1:    # inside the glass, far off-centre, nearly tangential: total internal reflection
            a = rng.normal(size=3); a /= np.linalg.norm(a)
            t = np.cross(a, rng.normal(size=3)); t /= np.linalg.norm(t)
            o, dd = c + a * 15.5, t
        elif kind == 2:    # grazing the rim from outside
            a = rng.normal(size=3); a /= np.linalg.norm(a)
            t = np.cross(a, rng.normal(size=3)); t /= np.linalg.norm(t)
            o, dd = c + a * 16.4999 - t * 30.0, t
        else:              # towards the mirror ball at normal incidence
            m = np.array([27.0, 16.5, 47.0])
            d = rng.normal(size=3); d[1] = abs(d[1]); d /= np.linalg.norm(d)
            o, dd = m + d * 30.0, -d
        rays[:3, i], rays[3:, i] = o, dd
    return rays.astype(np.float32)


def test_paths_bitwise_handmade_rays(apt):
    sph, mat, light = _scene(apt, "demo9")
    p = apt.make_params(16, 16, 1, depth=6, num_spheres=9, light_index=light, seed=4)
    rays = _handmade_rays(p.num_paths)
    want, _, _ = mr.trace(rays, sph, mat, 9, 6, p.eps, p.seed, np.arange(p.num_paths, dtype=np.uint64), gloss=False)
    got = _paths_gpu(apt, p, rays, sph, mat)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---- white furnace: analytic values, independent of the restatement ----------------------------------------------------------------
def _furnace(albedo, emission, eight):
    rows = [[1000.0, *CAMERA, emission, emission, emission, albedo, albedo, albedo]]
    if eight:                                          # the 8-sphere form: 7 tiny spheres far outside the enclosure
        rows += [[1.0, 5000.0 + 10 * k, 0.0, 0.0, 1.0, 1.0, 1.0, 0.5, 0.5, 0.5] for k in range(7)]
    return _table(rows), np.full(len(rows), mr.DIFF, dtype=np.int32)


@pytest.mark.parametrize("eight", [False, True])
def test_furnace_paths_exact(apt, eight):
    from oracle import oracle
    sph, mat = _furnace(1.0, 1.0, eight)
    for depth in (1, 2, 5, 8, 32):
        p = apt.make_params(16, 16, 2, depth=depth, num_spheres=mat.size, light_index=-1, eps=0.5, seed=depth,
                            flags=apt.APT_FLAG_EMISSION)
        rays = oracle.gen_rays_counter(oracle_params(p))
        got = _paths_gpu(apt, p, rays, sph, mat)
        assert (got == np.float32(depth)).all(), (depth, np.unique(got))


@pytest.mark.parametrize("eight", [False, True])
def test_furnace_frame_exact(apt, eight):
    sph, mat = _furnace(0.5, 0.25, eight)
    for depth, s_ in ((1, 1), (2, 3), (5, 8), (8, 16)):
        p = apt.make_params(32, 16, s_, depth=depth, num_spheres=mat.size, eps=0.5, seed=depth)
        fb, _ = _frame_gpu(apt, p, sph, mat)
        assert (fb == np.float32(0.5 * (1 - 2.0 ** -depth))).all(), (depth, np.unique(fb))


@pytest.mark.parametrize("eight", [False, True])
def test_furnace_roulette_mean(apt, eight):
    from oracle import oracle
    sph, mat = _furnace(0.5, 0.25, eight)
    depth = 8
    p = apt.make_params(32, 32, 8, depth=depth, num_spheres=mat.size, eps=0.5, seed=17, flags=apt.APT_FLAG_RR, rr_start=1)
    rays = oracle.gen_rays_counter(oracle_params(p))
    got = _paths_gpu(apt, p, rays, sph, mat)[0].astype(np.float64)
    want = 0.5 * (1 - 2.0 ** -depth)
    sigma = got.std() / np.sqrt(got.size)
    assert got.std() > 0 and abs(got.mean() - want) < 4 * sigma, (got.mean(), want, sigma)
    fb, _ = _frame_gpu(apt, p, sph, mat)
    assert abs(fb.astype(np.float64).mean() - want) < 4 * sigma


@pytest.mark.parametrize("scene", ["demo9", "diff8"])
def test_bad_material_code_is_reported(apt, scene):
    sph, mat, light = _scene(apt, scene)
    mat = mat.copy()
    mat[2] = 3                                         # the back wall: every frame hits it
    p = apt.make_params(16, 16, 1, depth=3, num_spheres=mat.size, light_index=light, seed=1)
    apt.render.check_device_status()                   # nothing pending from earlier tests
    _frame_gpu(apt, p, sph, mat)
    with pytest.raises(apt.AptError) as e:
        apt.render.check_device_status()               # (reads and clears the word: the autouse check after this test sees it clean)
    msg = str(e.value)
    assert "bad-material" in msg and "unknown-bits" not in msg and "queue" not in msg and "grid" not in msg and "lds" not in msg


def test_materials_none_is_the_mirror_renderer(apt):
    """materials=None takes the existing entry: the frame equals the oracle's mirror frame."""
    from oracle import oracle
    sph = apt.gen_data.gen_spheres()
    p = apt.make_params(16, 16, 8, depth=5, seed=1)
    fb, u8 = apt.render.render_frame(p, dev(sph), materials=None)
    fb_w, u8_w, _, _ = oracle.render_frame(oracle_params(p), sph)
    assert np.array_equal(fb.cpu().numpy().view(np.uint32), fb_w.view(np.uint32))
    mat = dev(np.zeros(8, dtype=np.int32))       # and a zero table is all mirrors -- but with emitted light, not gain x throughput
    fb_m, _ = apt.render.render_frame(p, dev(sph), materials=mat)
    assert not np.array_equal(fb_m.cpu().numpy(), fb.cpu().numpy())
