"""GPU: the material renderer through the uniform grid (include/render_mi355x.h "per-sphere materials": accel with APT_FLAG_GRID_SLOTS).
The walk only drops spheres that cannot be hit, so every comparison is on the float bits of the image and on its 8-bit form: against
the NumPy restatement (tests/materials_ref.py, brute force by definition) and against the tile form on the same inputs.
tests/test_materials_grid_cpu.py shows that the frames compared here hit binned spheres of every code, with binned skip spheres."""
import ctypes

import numpy as np
import pytest

import materials_ref as mr
from gpu_harness import Scene, apt, oracle_params, same  # noqa: F401

pytestmark = pytest.mark.gpu

SCENE_SEED, RENDER_SEED = 5, 3


def _header(sc):
    """The GridHeader's integer fields by name (pt_core.h)."""
    names = ("magic num_spheres n0 n1 n2 ncells nlarge nitems off_large off_cells off_items off_geom off_item_geom").split()
    h = dict(zip(names, (int(x) for x in sc.hgrid[:13])))
    h["margin"] = float(sc.hgrid[25:26].view(np.float32)[0])
    h["slot_base"] = int(sc.hgrid[30])
    return h


def _grid_scene(apt, sph, mat, builder="host", light=None):
    """A scene with a grid built for it; the light is the last sphere unless given."""
    ns = int(np.asarray(mat).size)
    return Scene(apt, sph, mat, ns, light=ns - 1 if light is None else light, grid=True, builder=builder)


_scenes, _wanted = {}, {}


def _generated(apt, ns, builder="host"):
    key = (ns, builder)
    if key not in _scenes:
        sph, mat = apt.gen_data.gen_scene_materials(ns, seed=SCENE_SEED)
        _scenes[key] = _grid_scene(apt, sph, mat, builder)
    return _scenes[key]


def _want_frame(sc, p, key):
    """The restatement's frame, computed once per case (it does not depend on who built the grid)."""
    if key not in _wanted:
        fb_w, u8_w, bad, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat)
        assert not bad.any()
        _wanted[key] = (fb_w, u8_w)
    return _wanted[key]


# both GROUP instantiations (samples < 8, >= 8), a tail (13 = 8 + 5), roulette; (2, 6, no) is the CPU test's coverage frame
FRAME_CASES = [(1, 1, False), (2, 6, False), (8, 5, True), (13, 8, False), (3, 8, True)]


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("s_,depth,rr", FRAME_CASES)
def test_frame_bitwise_against_the_restatement(apt, builder, s_, depth, rr):
    sc = _generated(apt, 2000, builder)
    p = sc.params(24, 16, s_, depth, rr=rr, grid=True)
    fb, u8 = sc.frame(p, check=False)
    same((fb, u8), _want_frame(sc, p, (2000, s_, depth, rr)))


def test_frame_bitwise_10k_spheres_against_the_restatement(apt):
    """The CPU test's second coverage frame: the scene, camera and depth of the 480x270 comparison below at a size NumPy can restate."""
    sc = _generated(apt, 10000)
    p = sc.params(16, 12, 1, 6, grid=True)
    fb, u8 = sc.frame(p, check=False)
    same((fb, u8), _want_frame(sc, p, (10000, 1, 6, False)))


def test_grid_form_equals_tile_form_at_10k_spheres(apt):
    """The frame size of the mirror renderer's 10 000-sphere test, whole frame, and the same number of traced segments."""
    sc = _generated(apt, 10000)
    with apt.render.TraceCounter() as tg:
        fb_g, u8_g = sc.frame(sc.params(480, 270, 8, 8, grid=True), check=False)
    with apt.render.TraceCounter() as tt:
        fb_t, u8_t = sc.frame(sc.params(480, 270, 8, 8, grid=False), check=False)
    same((fb_g, u8_g), (fb_t, u8_t))
    print("traced segments", tg.value, tt.value, "grid (segments, cells, candidates)", tg.stats)
    assert tg.value == tt.value > 480 * 270 * 4 * 8


def _degenerate(apt, name):
    if name == "demo9":            # nothing is large: walls and light binned, the always-tested list empty
        sph, mat = apt.gen_data.gen_spheres_materials()
        sc = _grid_scene(apt, sph, mat, light=7)
        h = _header(sc)
        assert (h["nlarge"], h["slot_base"], h["nitems"]) == (0, 0, 111) and (h["n0"], h["n1"], h["n2"]) == (3, 3, 3)
        assert abs(h["margin"] - 20.0) < 0.1
        return sc
    sph, mat = apt.gen_data.gen_scene_materials(16, seed=SCENE_SEED)
    sc = _grid_scene(apt, sph, mat)
    h = _header(sc)
    assert (h["n0"], h["n1"], h["n2"], h["nitems"], h["nlarge"]) == (3, 2, 4, 9, 7)
    return sc


@pytest.mark.parametrize("name", ["demo9", "scene16"])
def test_degenerate_grids(apt, name):
    sc = _degenerate(apt, name)
    light = getattr(sc, "light", sc.ns - 1)
    for rr in (False, True):
        p = sc.params(48, 32, 8, 5, rr=rr, seed=11, grid=True)
        p.light_index = light
        fb, u8 = sc.frame(p, check=False)
        pt = p.copy(accel=0, flags=p.flags & ~apt.APT_FLAG_GRID_SLOTS)
        same((fb, u8), sc.frame(pt, check=False))
        fb_w, u8_w, bad, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat)
        assert not bad.any()
        same((fb, u8), (fb_w, u8_w))


@pytest.mark.parametrize("per_cell", [0.25, 2.0])
def test_cell_size_knob(apt, per_cell):
    sph, mat = apt.gen_data.gen_scene_materials(2000, seed=SCENE_SEED)
    default_cells = _header(_generated(apt, 2000))["ncells"]
    with apt.render.debug_knob("grid_spheres_per_cell", per_cell):
        sc = _grid_scene(apt, sph, mat)
    assert (_header(sc)["ncells"] > default_cells) == (per_cell < 0.5) and _header(sc)["ncells"] != default_cells
    p = sc.params(48, 32, 8, 5, grid=True)
    fb, u8 = sc.frame(p, check=False)
    same((fb, u8), sc.frame(p.copy(accel=0, flags=0), check=False))
    same((fb, u8), _want_frame(sc, p, (2000, "48x32", 8, 5)))


def test_paths_bitwise_with_ranges(apt):
    from oracle import oracle
    sc = _generated(apt, 2000)
    p = sc.params(16, 16, 4, 8, rr=True, seed=9, grid=True)
    rays = oracle.gen_rays_counter(oracle_params(p))
    n = rays.shape[1]
    want, bad, _ = mr.trace(rays, sc.sph, sc.mat, sc.ns, 8, p.eps, p.seed, np.arange(n, dtype=np.uint64), rr_start=2, gloss=False)
    assert not bad.any()
    got = sc.paths(p, rays, check=False)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    b, c = 1001, 1537                                 # a path range of the whole-image buffers, then the same range in band buffers
    got = sc.paths(p.copy(path_begin=b, path_count=c), rays, check=False)
    assert np.array_equal(got[:, b:b + c].view(np.uint32), want[:, b:b + c].view(np.uint32))
    assert np.isnan(got[:, :b]).all() and np.isnan(got[:, b + c:]).all()
    pb = p.copy(path_begin=b, path_count=c, flags=p.flags | apt.APT_FLAG_BAND_BUFFERS)
    got = sc.paths(pb, np.ascontiguousarray(rays[:, b:b + c]), check=False)
    assert np.array_equal(got.view(np.uint32), want[:, b:b + c].view(np.uint32))


def _handmade_rays(sc, n):
    """Rays that start where the walk's set-up has its cases: inside a glass sphere, far outside the grid's box (towards it and away
    from it), with directions of length 0.5 and 2 (the every-sphere fallback), a NaN direction, and along each axis."""
    rng = np.random.default_rng(2)
    planes = sc.sph[:10 * sc.ns].reshape(10, sc.ns).astype(np.float64)
    glass = np.nonzero(sc.mat[6:sc.ns - 1] == mr.REFR)[0] + 6
    rays = np.zeros((6, n))
    for i in range(n):
        kind = i % 8
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        o = np.array([1.0 + 98.0 * rng.random(), 81.6 * rng.random(), 170.0 * rng.random()])   # somewhere among the small spheres
        if kind == 0:      # inside a glass sphere, off-centre
            k = glass[rng.integers(glass.size)]
            o = planes[1:4, k] + d * 0.6 * np.sqrt(planes[0, k])
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
        elif kind == 1:    # far outside the box, aimed at a point inside it
            far = o + d * 5000.0
            o, d = far, -d
        elif kind == 2:    # far outside the box, leaving
            o = o + d * 5000.0
        elif kind == 3:
            d = d * 0.5
        elif kind == 4:
            d = d * 2.0
        elif kind == 5:
            d = np.array([np.nan, d[1], d[2]]) if i % 16 == 5 else d * np.nan
        else:              # parallel to an axis (two zero components), either sense
            a = np.zeros(3)
            a[(i // 8) % 3] = 1.0 if kind == 6 else -1.0
            d = a
        rays[:3, i], rays[3:, i] = o, d
    return rays.astype(np.float32)


def test_paths_bitwise_handmade_rays(apt):
    sc = _generated(apt, 2000)
    p = sc.params(16, 16, 1, 6, seed=4, grid=True)
    rays = _handmade_rays(sc, p.num_paths)
    want, bad, _ = mr.trace(rays, sc.sph, sc.mat, sc.ns, 6, p.eps, p.seed, np.arange(p.num_paths, dtype=np.uint64), gloss=False)
    assert not bad.any()
    got = sc.paths(p, rays, check=False)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (diff[:8], rays[:, diff[0][1]])
    assert (want[:, 0::8] != 0).any() and (want[:, 3::8] != 0).any()       # such rays do reach the light


def test_frame_pixel_range_and_u8_forms(apt):
    import torch
    sc = _generated(apt, 2000)
    p = sc.params(24, 16, 8, 5, seed=2, flags=apt.APT_FLAG_RETIRE, grid=True)
    b, c = 117, 203
    fb_w, u8_w, _, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat, pixel_begin=b, pixel_count=c)
    L = apt._lib.lib()
    for off in (None, 1):                              # fb_u8 null, then one byte off a dword
        fb = torch.full((3, c), float("nan"), dtype=torch.float32, device="cuda")
        raw = torch.zeros(c * 3 + 4, dtype=torch.uint8, device="cuda")
        u8_ptr = None if off is None else ctypes.c_void_p(raw.data_ptr() + off)
        rc = L.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(sc.d_sph.data_ptr()), ctypes.c_void_p(sc.d_mat.data_ptr()),
                                          ctypes.c_uint64(b), ctypes.c_uint64(c), ctypes.c_void_p(fb.data_ptr()), u8_ptr)
        apt._lib.check(rc, "apt_render_frame_materials")
        torch.cuda.synchronize()
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), fb_w.view(np.uint32))
        raw = raw.cpu().numpy()
        if off is None:
            assert not raw.any()
        else:
            assert np.array_equal(raw[1:1 + 3 * c].reshape(c, 3), u8_w) and raw[0] == 0 and not raw[1 + 3 * c:].any()


def test_bad_material_code_on_a_binned_sphere_is_reported(apt):
    base = _generated(apt, 2000)
    mat = base.mat.copy()
    mat[6:base.ns - 1][base.mat[6:base.ns - 1] == mr.REFR] = 3      # every glass sphere: the coverage frame sends 14.7 % of its segments there
    sc = _grid_scene(apt, base.sph, mat)
    p = sc.params(24, 16, 2, 6, grid=True)
    _, _, bad, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat)
    assert bad.any()
    apt.render.check_device_status()                   # nothing pending from earlier tests
    sc.frame(p, check=False)
    with pytest.raises(apt.AptError) as e:
        apt.render.check_device_status()               # (reads and clears the word: the autouse check after this test sees it clean)
    msg = str(e.value)
    assert "bad-material" in msg and "grid" not in msg and "unknown-bits" not in msg


def test_a_broken_promise_renders_nothing_and_is_reported(apt):
    import torch
    sc = _generated(apt, 2000)
    other = _generated(apt, 10000).grid                # another scene's grid, and a buffer of zeros
    apt.render.check_device_status()
    for g in (other, torch.zeros(4096, dtype=torch.int32, device="cuda")):
        for s_ in (8, 2):
            p = sc.params(16, 12, s_, 6, grid=True).copy(accel=g.data_ptr())
            fb = torch.full((3, 16 * 12), -1.0, device="cuda")
            u8 = torch.full((16 * 12, 3), 7, dtype=torch.uint8, device="cuda")
            apt.render.render_frame(p, sc.d_sph, fb=fb, fb_u8=u8, materials=sc.d_mat)
            with pytest.raises(apt.AptError, match="grid-mismatch"):
                apt.render.check_device_status()
            assert bool((fb == -1.0).all()) and bool((u8 == 7).all())      # nothing was walked, nothing was written
            apt.render.check_device_status()           # cleared by the check
        p = sc.params(16, 12, 1, 6, grid=True).copy(accel=g.data_ptr())
        colors = torch.full((3 * p.num_paths,), -1.0, device="cuda")
        rays = torch.zeros(6 * p.num_paths, device="cuda")
        apt.render.render_do_ex(p, None, rays, sc.d_sph, colors, materials=sc.d_mat)
        with pytest.raises(apt.AptError, match="grid-mismatch"):
            apt.render.check_device_status()
        assert bool((colors == -1.0).all())
        apt.render.check_device_status()


def test_materials_none_with_a_grid_is_the_mirror_renderer(apt):
    """materials=None takes the mirror entry, grid and flag included, untouched: the oracle's mirror frame."""
    from oracle import oracle
    ns = 300
    sph = apt.gen_data.gen_scene(ns, seed=7)
    sc = _grid_scene(apt, sph, np.ones(ns, dtype=np.int32))
    p = sc.params(16, 12, 8, 6, seed=4, grid=True)
    fb, _ = apt.render.render_frame(p, sc.d_sph, materials=None)
    fb_w = oracle.render_frame(oracle_params(p), sph)[0]
    assert np.array_equal(fb.cpu().numpy().view(np.uint32), fb_w.view(np.uint32))
