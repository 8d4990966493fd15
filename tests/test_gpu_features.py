"""GPU: the first-hit feature planes (include/render_mi355x.h "features") through the C-ABI, bit for bit against the NumPy restatement
tests/features_ref.py with the status word clean.

  planes    the three scene forms -- the stock 8-sphere room and gen_spheres_open() (8-sphere form), 40 open spheres by tiles, 220 through
            the grid with grid planes == tile planes -- over samples 1, 3, 8, 9 and 16, with no camera, a moved pinhole camera and a thin
            lens; 16 x 8 at 129 samples, a sum of 516 terms per pixel.
  buffer    two seeds; a buffer of NaN; a mid-image pixel range inside guard words; two bands that split a column; a grid that is not the
            scene's; the entry's own refusals.
  Film      render.Film.features end to end, through a context with a camera.
  renderer  the albedo planes against one film pass at depth 1 in a scene whose spheres emit their albedo: the same first hit.

On the parent every test here fails: the entries do not exist."""
import ctypes
import math

import numpy as np
import pytest

import camera_ref as cr
import features_ref as ft
import materials_ref as mr
from gpu_harness import Scene, apt, assert_bits_equal, dev, lens, pinhole  # noqa: F401

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
W, H = 48, 32
SIZE = {"open220": (24, 16)}            # the restatement tests every path against every sphere: a quarter of the pixels for 220 of them
EPS = 1e-4                              # make_params' default, which the launches take
DEPTH = 5                               # not read by the entry: make_params' default


def _ref(sc, p, cam=None):
    """features_ref's planes of the whole frame (the grid changes no plane: not part of the key); read-only, shared."""
    key = ("planes", p.width, p.height, p.samples, p.seed, None if cam is None else bytes(cam))
    if key not in sc.ref:
        rec = cr.default_record(p.width, p.height) if cam is None else cr.from_ctypes(cam)
        planes = ft.planes(rec, p.width, p.height, p.samples, p.seed, sc.sph, sc.ns, EPS)
        planes.setflags(write=False)
        sc.ref[key] = planes
    return sc.ref[key]


_scenes = {}


def _scene(apt, name):
    """Sphere tables alone (the open ones without the lamps of the catalogue's): the entry reads no material word and no light, so the
    words are DIFF and never uploaded, and the light is make_params' default, the last sphere."""
    if name not in _scenes:
        gd = apt.gen_data
        if name == "room8":
            sph, ns = gd.gen_spheres(), 8
        elif name == "open8":
            sph, ns = gd.gen_spheres_open()[0], 8
        elif name == "glow8":                                                     # every sphere emits its albedo (all positive)
            sph, ns = gd.gen_spheres_open()[0].copy(), 8
            t = sph[:80].reshape(10, 8)
            t[4:7] = t[7:10]
            assert (t[7:10] > 0).all()
        else:
            ns = 40 if name == "open40" else 220
            sph = gd.gen_scene_open(ns, seed=2)[0]
        _scenes[name] = Scene(apt, sph, np.full(ns, mr.DIFF, dtype=np.int32), ns, light=ns - 1, grid=ns > 64)
    return _scenes[name]


def _camera(apt, kind, w, h):
    return None if kind is None else {"lens": lens, "pinhole": pinhole}[kind](apt, w, h)


# (samples, camera) per scene: every sample count and every camera meets both 8-sphere scenes and each of the other forms
LAUNCHES = {"room8": [(1, None), (8, "pinhole"), (16, "lens"), (3, "lens"), (9, None)],
            "open8": [(3, None), (9, "lens"), (16, "pinhole"), (1, "lens"), (8, None)],
            "open40": [(1, "lens"), (8, None), (3, "pinhole"), (9, "pinhole"), (16, None)],
            "open220": [(3, None), (9, "lens"), (1, "pinhole"), (8, "lens"), (16, None)]}


@pytest.mark.parametrize("name,grid", [("room8", False), ("open8", False), ("open40", False), ("open220", True)], ids=["room8", "open8", "tiles40", "grid220"])
def test_planes_equal_the_restatement(apt, name, grid):
    sc = _scene(apt, name)
    w, h = SIZE.get(name, (W, H))
    seen = np.zeros(3, dtype=bool)
    for s_, kind in LAUNCHES[name]:
        cam = _camera(apt, kind, w, h)
        p = sc.params(w, h, s_, DEPTH, seed=50 + s_, grid=grid)
        got = sc.features(p, cam)
        want = _ref(sc, p, cam)
        assert_bits_equal(got, want)
        cov = want[ft.COVERAGE]
        seen |= [(cov == 0).any(), ((cov > 0) & (cov < 1)).any(), (cov == 1).any()]
        if grid:                                                                  # the grid form is the tile form
            tiles = sc.params(w, h, s_, DEPTH, seed=50 + s_)
            assert tiles.accel == 0 and p.accel != 0
            assert_bits_equal(sc.features(tiles, cam), got)
    assert seen[2] and (name == "room8" or seen.all())                            # hits everywhere; the open scenes also miss and straddle


def test_a_sum_of_516_terms(apt):
    """16 x 8 at 129 samples: the longest per-pixel sum of this file (tests/test_features_cpu.py says why it is not a test of the order)."""
    sc = _scene(apt, "open8")
    p = sc.params(16, 8, 129, DEPTH, seed=13)
    assert_bits_equal(sc.features(p), _ref(sc, p))
    cam = _camera(apt, "lens", 16, 8)
    assert_bits_equal(sc.features(p, cam), _ref(sc, p, cam))


def test_seeds(apt):
    sc = _scene(apt, "open8")
    a, b = sc.features(sc.params(W, H, 3, DEPTH, seed=53)), sc.features(sc.params(W, H, 3, DEPTH, seed=54))
    assert_bits_equal(a, sc.features(sc.params(W, H, 3, DEPTH, seed=53)))
    assert_bits_equal(a, _ref(sc, sc.params(W, H, 3, DEPTH, seed=53)))
    assert (a != b).any(axis=1)[[ft.COVERAGE, ft.DEPTH, ft.NORMAL, ft.ALBEDO]].all()


def test_a_buffer_of_nan_is_overwritten(apt):
    import torch
    for name, s_ in (("open8", 3), ("open40", 8)):
        sc = _scene(apt, name)
        p = sc.params(W, H, s_, DEPTH, seed=50 + s_)
        buf = torch.full((8, W * H), float("nan"), dtype=torch.float32, device="cuda")
        got = sc.features(p, features=buf)
        assert not np.isnan(got).any() and not np.isnan(_ref(sc, p)).any()
        assert_bits_equal(got, _ref(sc, p))


@pytest.mark.parametrize("name,grid", [("open8", False), ("open40", False), ("open220", True)], ids=["8", "tiles40", "grid220"])
def test_a_pixel_range_inside_guards(apt, name, grid):
    """Pixels [37, 37 + 1001) -- or what a smaller frame has from 37 on --: not a multiple of a workgroup's 256 pixels, more than one workgroup."""
    import torch
    sc = _scene(apt, name)
    w, h = SIZE.get(name, (W, H))
    b, guard = 37, 64
    c = min(1001, w * h - b - 3)
    assert c > 256 and c % 256
    p = sc.params(w, h, 3, DEPTH, seed=53, grid=grid)
    block = torch.full((guard + 8 * c + guard,), -9.0, dtype=torch.float32, device="cuda")
    sc.features(p, features=block[guard:guard + 8 * c].view(8, c), pixel_begin=b, pixel_count=c)
    host = block.cpu().numpy()
    assert (host[:guard] == -9.0).all() and (host[guard + 8 * c:] == -9.0).all()
    assert_bits_equal(host[guard:guard + 8 * c].reshape(8, c), _ref(sc, p)[:, b:b + c])


def test_two_bands_that_split_a_column(apt):
    sc = _scene(apt, "open8")
    p = sc.params(W, H, 9, DEPTH, seed=59)
    cam = _camera(apt, "lens", W, H)
    whole = sc.features(p, cam)
    cut = H + 18                                                                  # inside column 1
    assert_bits_equal(sc.features(p, cam, pixel_begin=0, pixel_count=cut), whole[:, :cut])
    assert_bits_equal(sc.features(p, cam, pixel_begin=cut, pixel_count=W * H - cut), whole[:, cut:])
    assert_bits_equal(whole, _ref(sc, p, cam))


def test_a_grid_that_is_not_the_scenes_leaves_the_buffer_untouched(apt):
    import torch
    sc = _scene(apt, "open220")
    other = apt.gen_data.build_grid(apt.gen_data.gen_scene_open(100, seed=9)[0], 100)
    d_other = torch.from_numpy(other.view(np.int32)).cuda()
    apt.render.check_device_status()                                             # nothing pending
    p = sc.params(24, 16, 3, DEPTH)
    p.flags |= apt.APT_FLAG_GRID_SLOTS
    p.accel = d_other.data_ptr()
    buf = torch.full((8, 24 * 16), -2.0, dtype=torch.float32, device="cuda")
    apt.render.render_frame_features(p, sc.d_sph, features=buf)
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == -2.0).all()
    with pytest.raises(apt.AptError, match="grid-mismatch"):
        apt.render.check_device_status()                                         # reads and clears the word


def test_the_entrys_own_refusals(apt):
    import torch
    sc = _scene(apt, "open8")
    L = apt._lib.lib()
    p = sc.params(W, H, 8, DEPTH)
    buf = torch.full((8, W * H), -2.0, dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    call = lambda q, sph, out, n=W * H: L.apt_render_frame_features(ctypes.byref(q), None, ptr(sph), ctypes.c_uint64(0), ctypes.c_uint64(n), ptr(out))
    assert call(p, sc.d_sph, None) == 1 and b"features" in L.apt_last_error()
    assert call(p, None, buf) == 1 and b"spheres" in L.apt_last_error()
    assert call(p.copy(samples=4200), sc.d_sph, buf) == 1 and b"44 leaves" in L.apt_last_error()
    assert call(p.copy(samples=4200), sc.d_sph, None) == 1 and b"44 leaves" in L.apt_last_error()
    assert call(p, sc.d_sph, buf, W * H + 1) == 1 and b"pixel range" in L.apt_last_error()
    assert call(p.copy(num_spheres=40, accel=buf.data_ptr()), sc.d_sph, buf) == 1 and b"APT_FLAG_GRID_SLOTS" in L.apt_last_error()
    bad = p.copy()
    bad.struct_size = 8
    assert call(bad, sc.d_sph, buf) == 2
    assert call(p, sc.d_sph, None, 0) == 0                                       # an empty range launches nothing
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == -2.0).all()
    with pytest.raises(apt.AptError, match="features"):
        apt.render.render_frame_features(p, sc.d_sph, features=torch.zeros((8, 5), dtype=torch.float32, device="cuda"))
    # fields the entry does not read: a film pass's record as it is
    q = p.copy(depth=0, flags=apt.APT_FLAG_NEE | apt.APT_FLAG_RR | apt.APT_FLAG_GLOSS, light_index=-1, mode=1)
    assert_bits_equal(sc.features(q), _ref(sc, p))


def test_film_features_end_to_end(apt):
    import torch
    sc = _scene(apt, "open40")
    p = sc.params(W, H, 8, DEPTH, seed=58)
    cam = _camera(apt, "pinhole", W, H)
    ctx = apt.render.Context()
    try:
        ctx.set_camera(cam)
        film = apt.render.Film(W, H)
        got = film.features(p, sc.d_sph, context=ctx)
        torch.cuda.synchronize()
        ctx.check()
        assert tuple(got.shape) == (apt.APT_FEATURE_PLANES, W * H) and film.passes == 0
        assert_bits_equal(got.cpu().numpy(), _ref(sc, p, cam))
        band = apt.render.Film(W, H, pixel_begin=100, pixel_count=300)
        got = band.features(p, sc.d_sph, context=ctx)
        torch.cuda.synchronize()
        assert_bits_equal(got.cpu().numpy(), _ref(sc, p, cam)[:, 100:400])
        assert_bits_equal(ctx.render_frame_features(p, sc.d_sph, pixel_begin=100, pixel_count=300).cpu().numpy(), _ref(sc, p, cam)[:, 100:400])
        assert_bits_equal(film.features(p, sc.d_sph).cpu().numpy(), _ref(sc, p))        # the default context: no camera
        with pytest.raises(apt.AptError, match="width / height"):
            film.features(sc.params(W, H + 1, 8, DEPTH), sc.d_sph)
        ctx.check()
    finally:
        ctx.close()
    apt.render.check_device_status()


@pytest.mark.parametrize("s_", [3, 8, 9, 16])
def test_albedo_planes_against_a_film_pass_at_depth_one(apt, s_):
    """Every sphere emits its albedo, so one film pass at depth 1 without an environment gathers, per path, L = 0 + 1 * emission = the
    albedo of the first hit, exactly, or 0 on a miss: per path the very values of the albedo planes.  The two entries differ in how
    they average a pixel's n = 4 S values v >= 0, of mean m <= M = the largest of them; u = 2^-24.
      film      each sub-pixel's S values are added in float32 along numpy's pairwise plan, where a value passes through a additions:
                a = S - 1 for S < 8, else (the chain) ceil(S / 8) - 1 + (the tree) 3, + 1 where a tail is added: a = 2, 3, 4, 4 for
                S = 3, 8, 9, 16, never more than ceil(log2(S)) + 1 = ceil(log2(n)) - 1.  The computed sum is within a * u of the true one,
                relatively (all terms have one sign: the pairwise-sum bound (1 + u)^a - 1); the division by S rounds once more; the four
                means are added in float64 and divided by 4, exactly at this scale; the result is rounded to float32: a + 2 roundings.
      features  the float64 sum of 4 S float32 values and its quotient are exact at this scale; one rounding to float32.
    So |film - features| <= (a + 3) u M to first order, and (a + 3) <= ceil(log2(n)) + 2 leaves the second-order terms a whole u: the
    bound is (ceil(log2(4 S)) + 2) * 2^-24 * M per pixel.  A first hit that differs moves a path's value by a whole albedo
    difference, 2^20 times as much."""
    import torch
    sc = _scene(apt, "glow8")
    a = {3: 2, 8: 3, 9: 4, 16: 4}[s_]
    assert a + 3 <= math.ceil(math.log2(4 * s_)) + 2
    p = sc.params(W, H, s_, 1, seed=61).copy(light_index=-1)
    mat = dev(np.full(8, mr.DIFF, dtype=np.int32))
    film = apt.render.render_frame_film(p, sc.d_sph, mat)
    torch.cuda.synchronize()
    apt.render.check_device_status()
    film = film.cpu().numpy().astype(D)
    got = sc.features(p)
    assert_bits_equal(got, _ref(sc, p))
    rays = cr.rays(cr.default_record(W, H), W, H, s_, seed=61)
    M = ft.path_values(rays, sc.sph, 8, EPS)[ft.ALBEDO:ft.ALBEDO + 3].reshape(3, W * H, 4 * s_).max(axis=2).astype(D)
    bound = (math.ceil(math.log2(4 * s_)) + 2) * 2.0 ** -24 * M
    err = np.abs(film - got[ft.ALBEDO:ft.ALBEDO + 3].astype(D))
    assert (err <= bound).all(), (err.max(), float((err / np.where(bound > 0, bound, 1)).max()))
    assert (M > 0).any() and (M == 0).any() and (film[M == 0] == 0).all()
