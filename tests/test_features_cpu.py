"""CPU-only: the first-hit feature planes (include/render_mi355x.h "features") -- the symbols, every refusal of the entry through the
C-ABI without a GPU and their order against a film launch, and the restatement tests/features_ref.py against closed forms written from
geometry alone, against the material restatement's first segment, and in the two stock scenes.

Without the feature nothing here passes: the entries, the constants and the restatement do not exist."""
import ctypes
import math

import numpy as np
import pytest

import camera_ref as cr
import features_ref as ft
import materials_ref as mr

F, D, U = np.float32, np.float64, np.uint64
APT_ERR_ARG, APT_ERR_STRUCT, APT_ERR_SCENE = 1, 2, 3


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data, render
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def test_symbols_and_constants(apt):
    assert apt._lib.lib().apt_abi_version() == 3                                  # additive: same ABI version
    for name in ("apt_render_frame_features", "apt_context_render_frame_features"):
        assert name in apt._lib.ABI_SYMBOLS and hasattr(apt._lib.lib(), name)
    header = open(mr.ROOT + "/include/render_mi355x.h").read()
    assert "#define APT_ABI_VERSION 3 " in header
    want = dict(APT_FEATURE_COVERAGE=0, APT_FEATURE_DEPTH=1, APT_FEATURE_NORMAL=2, APT_FEATURE_ALBEDO=5, APT_FEATURE_PLANES=8)
    for name, v in want.items():
        assert getattr(apt, name) == v and "%s = %d" % (name, v) in header
    assert (ft.COVERAGE, ft.DEPTH, ft.NORMAL, ft.ALBEDO, ft.PLANES) == (0, 1, 2, 5, 8)
    assert hasattr(apt.render, "render_frame_features") and hasattr(apt.render.Context, "render_frame_features") and hasattr(apt.render.Film, "features")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_without_a_gpu_and_its_order_against_a_film_launch(apt):
    """Every call here is refused before anything is launched: a NULL stream, pointers that are never followed, no GPU needed.  Where a
    film launch refuses the same bad parameters, it refuses with the same status and the same text."""
    L = apt._lib.lib()
    ptr = ctypes.c_void_p(0x1000)                                                 # non-null; the host never follows it
    W, H = 48, 32
    good = apt.make_params(W, H, 8, depth=3, num_spheres=8, seed=1)
    err = lambda: L.apt_last_error()

    def feat(p, sph=ptr, out=ptr, b=0, n=W * H):
        return L.apt_render_frame_features(None if p is None else ctypes.byref(p), None, sph, ctypes.c_uint64(b), ctypes.c_uint64(n), out)

    def film(p, sph=ptr, out=ptr, b=0, n=W * H):
        return L.apt_render_frame_film(None if p is None else ctypes.byref(p), None, sph, ptr, None, ctypes.c_uint64(b), ctypes.c_uint64(n), out,
                                       ctypes.c_uint32(0))

    def both(status, text, *a, **kw):
        assert feat(*a, **kw) == status and text in err(), err()
        msg = err()
        assert film(*a, **kw) == status and err() == msg, (msg, err())

    # the params record's own
    both(APT_ERR_ARG, b"params", None)
    bad = good.copy()
    bad.struct_size = 8
    both(APT_ERR_STRUCT, b"struct_size", bad)
    for zero in ("width", "height", "samples"):
        both(APT_ERR_ARG, b"non-zero", good.copy(**{zero: 0}))
    both(APT_ERR_SCENE, b"num_spheres", good.copy(num_spheres=0))
    assert feat(good.copy(num_spheres=40, accel=0x2000)) == APT_ERR_ARG and b"APT_FLAG_GRID_SLOTS" in err()
    assert film(good.copy(num_spheres=40, accel=0x2000, light_index=0)) == APT_ERR_ARG and b"APT_FLAG_GRID_SLOTS" in err()
    assert L.apt_context_render_frame_features(None, ctypes.byref(good), None, ptr, ctypes.c_uint64(0), ctypes.c_uint64(1), ptr) == APT_ERR_ARG
    assert b"context" in err()
    # fields the entry does not read are not checked: what a film refuses for them, the features accept up to the next refusal
    ignored = good.copy(mode=7, light_index=99, flags=apt.APT_FLAG_NEE, depth=0)
    assert feat(ignored, n=0) == 0 and feat(ignored, out=None) == APT_ERR_ARG and b"features" in err()
    # a film's, in its order: pointers, range, size (the plan), the 44 leaves, the default camera's record -- and only then `features`
    both(APT_ERR_ARG, b"spheres", good, sph=None)
    both(APT_ERR_ARG, b"spheres", good, sph=None, n=W * H + 1)
    both(APT_ERR_ARG, b"pixel range", good, n=W * H + 1)
    both(APT_ERR_ARG, b"pixel range", good, b=W * H + 1, n=0)
    both(APT_ERR_ARG, b"pixel range", good.copy(samples=4200), n=W * H + 1, out=None)
    both(APT_ERR_ARG, b"64 leaves", good.copy(samples=7689))
    both(APT_ERR_ARG, b"64 leaves", good.copy(samples=7689), out=None)
    assert feat(good.copy(samples=4200)) == APT_ERR_ARG and b"44 leaves" in err()
    assert film(good.copy(samples=4200)) == APT_ERR_ARG and b"44 leaves" in err()
    assert feat(good.copy(samples=4200), out=None) == APT_ERR_ARG and b"44 leaves" in err()
    wide = good.copy(width=1 << 22, height=1)                                     # cx = 2^22 * 0.5135 leaves the record's bound of 2^20
    cam = apt._lib.ApCamera()
    cam.struct_size = ctypes.sizeof(cam)
    assert L.apt_camera_default_host(ctypes.c_uint32(1 << 22), ctypes.c_uint32(1), ctypes.byref(cam)) == APT_ERR_ARG
    text = err()
    both(APT_ERR_ARG, text, wide, n=5)
    both(APT_ERR_ARG, text, wide, n=5, out=None)                                  # before the null buffer
    assert feat(wide.copy(samples=4200), n=5) == APT_ERR_ARG and b"44 leaves" in err()   # after the 44 leaves
    assert feat(good, out=None) == APT_ERR_ARG and b"features must be non-null" in err()
    assert film(good, out=None) == APT_ERR_ARG and b"film must be non-null" in err()
    # an empty range is APT_OK and launches nothing, whatever the buffer
    for kw in (dict(n=0), dict(b=W * H, n=0), dict(n=0, out=None)):
        assert feat(good, **kw) == 0 and err() == b"" and film(good, **kw) == 0


# ---- the restatement against geometry ---------------------------------------------------------------------------------------------------
def _one_sphere(r, dist):
    """A sphere of radius r at distance `dist` straight ahead of an eye at the origin that looks along -z; albedo (0.25, 0.5, 0.75)."""
    from ascendpathtracing_amd import gen_data
    return gen_data._table_of([[r, 0.0, 0.0, -dist, 0, 0, 0, 0.25, 0.5, 0.75]])


def _pinhole(apt, w, h, scale):
    cam = apt.gen_data.camera(eye=(0.0, 0.0, 0.0), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), scale=scale, offset=0.0, width=w, height=h)
    return cr.from_ctypes(cam)


def test_depth_and_normal_at_the_nearest_point(apt):
    """The centre pixel of an odd x odd image looks straight at the sphere's nearest point: its centre ray is the axis.
    Tolerance, from the pixel's angular size alone.  A sample of pixel (i, j) has xa - i = (sx + 0.5 + dd) / 2 with sx in {0, 1} and the
    tent's dd in (-1, 1): within 0.75 pixel of the pixel's centre on each axis.  A pixel is scale / h wide at forward depth 1, so every ray of
    the centre pixel makes an angle theta with the axis of at most theta_max, tan(theta_max) = sqrt(2) * 0.75 * scale / h.  A ray at
    angle theta meets the sphere (centre distance R, radius r) at t(theta) = R cos(theta) - sqrt(r^2 - R^2 sin^2(theta)), which grows
    with theta from t(0) = R - r; the normal there makes the angle phi with the direction to the eye, sin(phi) = t sin(theta) / r.  So the
    pixel's mean depth lies in [R - r, t(theta_max)], its mean normal has n_z in [cos(phi_max), 1] and |n_x|, |n_y| <= sin(phi_max).  On
    top of that the float32 arithmetic: a few ulp of the largest intermediate, R -- 8 * 2^-24 * R is allowed for."""
    w, h, s, scale, R, r = 33, 17, 16, 0.5, 10.0, 2.0
    rec = _pinhole(apt, w, h, scale)
    got = ft.planes(rec, w, h, s, 5, _one_sphere(r, R), 1, 1e-4).astype(D)
    px = (w // 2) * h + h // 2
    tan_max = math.sqrt(2.0) * 0.75 * scale / h
    th = math.atan(tan_max)
    t_max = R * math.cos(th) - math.sqrt(r * r - (R * math.sin(th)) ** 2)
    sin_phi = t_max * math.sin(th) / r
    slack = 8 * 2.0 ** -24 * R
    assert t_max - (R - r) < 0.025 and sin_phi < 0.15                             # the bounds say something: 0.3 % of the depth, 8 degrees
    assert got[ft.COVERAGE, px] == 1.0
    assert R - r - slack <= got[ft.DEPTH, px] <= t_max + slack
    assert math.sqrt(1 - sin_phi ** 2) - slack <= got[ft.NORMAL + 2, px] <= 1.0 + slack
    assert abs(got[ft.NORMAL, px]) <= sin_phi + slack and abs(got[ft.NORMAL + 1, px]) <= sin_phi + slack
    assert tuple(got[ft.ALBEDO:ft.ALBEDO + 3, px]) == (0.25, 0.5, 0.75)           # a mean of equal values that float32 holds exactly
    corner = got[:, 0]
    assert (corner == 0.0).all()                                                  # the image's corner sees no sphere: all eight are 0


def test_coverage_is_the_projected_area(apt):
    """A sphere so small that its image lies wholly inside the centre pixel (and so inside one pixel row).  A ray hits it iff its point on
    the plane at forward depth 1 lies in the disc of radius tan(alpha), sin(alpha) = r / R: area pi r^2 / (R^2 - r^2).  A pixel's samples
    are spread by the mean of four tents of half-width half a pixel on sub-pixel centres half a pixel apart; over all pixels those
    weights add up to 1 everywhere, so the SUM of all coverages tends to that area in pixel areas, A.
    Tolerance: the paths are independent draws, a pixel of hit probability p has variance p (1 - p) / (4 S) <= p / (4 S), and the p add
    up to A: sigma <= sqrt(A / (4 S)); six sigma are allowed."""
    w, h, s, scale, R = 9, 9, 1024, 0.5, 10.0
    pixel = scale / h                                                             # at forward depth 1
    radius = 0.4 * pixel                                                          # of the disc: wholly inside the centre pixel
    r = R * math.sin(math.atan(radius))
    area = math.pi * r * r / (R * R - r * r) / (pixel * pixel)
    assert abs(area - math.pi * 0.16) < 1e-9
    rec = _pinhole(apt, w, h, scale)
    cov = ft.planes(rec, w, h, s, 9, _one_sphere(r, R), 1, 1e-4)[ft.COVERAGE].astype(D).reshape(w, h)
    assert abs(cov.sum() - area) <= 6 * math.sqrt(area / (4 * s)), (cov.sum(), area)
    far = np.ones((w, h), dtype=bool)
    far[3:6, 3:6] = False                                                         # samples reach 0.75 pixel from their pixel's centre: the 3 x 3 block
    assert (cov[far] == 0.0).all() and 0.0 < cov[4, 4] < 1.0


def test_the_albedo_values_are_the_material_restatements_first_segment(apt):
    """Per path: with every sphere's emission equal to its albedo, one segment of materials_ref.trace gathers exactly the albedo of the
    first hit, or 0 -- the same first hit, or the planes differ by whole albedos."""
    sph, mat = apt.gen_data.gen_spheres_open()
    sph = sph.copy()
    t = sph[:80].reshape(10, 8)
    t[4:7] = t[7:10]
    rays = cr.rays(cr.default_record(16, 8), 16, 8, 2, seed=3)
    L, bad, _ = mr.trace(rays, sph, np.full(8, mr.DIFF, dtype=np.int32), 8, 1, 1e-4, 3, np.arange(rays.shape[1], dtype=U))
    vals = ft.path_values(rays, sph, 8, 1e-4)
    assert not bad.any() and np.array_equal(L.view(np.uint32), vals[ft.ALBEDO:ft.ALBEDO + 3].view(np.uint32))
    assert np.array_equal(vals[ft.COVERAGE] == 1, L[0] > 0) and 0 < (vals[ft.COVERAGE] == 0).sum() < vals.shape[1]


def test_stock_scenes_cover_and_miss(apt):
    """The closed room: coverage exactly 1 everywhere, unit normals facing the ray.  gen_spheres_open(): sky above the horizon, so there
    are pixels of coverage exactly 0 and pixels partly covered -- the miss arm is exercised."""
    w, h, s = 24, 16, 4
    rec = cr.default_record(w, h)
    room = ft.planes(rec, w, h, s, 1, apt.gen_data.gen_spheres(), 8, 1e-4)
    assert (room[ft.COVERAGE] == 1.0).all() and (room[ft.DEPTH] > 0).all() and np.isfinite(room).all()
    n = room[ft.NORMAL:ft.NORMAL + 3].astype(D)
    assert (np.sqrt((n * n).sum(axis=0)) <= 1.0 + 1e-6).all()                     # a mean of unit vectors
    open_ = ft.planes(rec, w, h, s, 1, apt.gen_data.gen_spheres_open()[0], 8, 1e-4)
    cov = open_[ft.COVERAGE]
    assert (cov == 0.0).any() and ((cov > 0.0) & (cov < 1.0)).any() and (cov == 1.0).any()
    assert (open_[:, cov == 0.0] == 0.0).all()                                    # a miss is eight zeros


def test_bands_and_seeds():
    from ascendpathtracing_amd import gen_data
    w, h, s = 12, 8, 3
    rec, sph = cr.default_record(w, h), gen_data.gen_spheres_open()[0]
    whole = ft.planes(rec, w, h, s, 4, sph, 8, 1e-4)
    assert np.array_equal(ft.planes(rec, w, h, s, 4, sph, 8, 1e-4, 13, 37).view(np.uint32), whole[:, 13:50].view(np.uint32))
    assert not np.array_equal(ft.planes(rec, w, h, s, 5, sph, 8, 1e-4), whole)


def test_the_order_of_the_sum_cannot_be_seen_at_129_samples():
    """The contract fixes ascending path order.  Could a GPU test tell a kernel that sums in another order?  Not at these sizes: a float32
    value has 24 significant bits and 516 of them add up exactly in float64's 53 unless their exponents span more than 53 - 24 - 10 = 19
    binades, and an inexact sum changes the float32 result only when it falls within 2^-53 of a rounding boundary.  The restatement
    summed in DESCENDING order gives the same bits in every pixel of the 129-sample case of tests/test_gpu_features.py, so that case
    is a long sum, not a test of the order, and no test claims to be one."""
    from ascendpathtracing_amd import gen_data
    w, h, s = 16, 8, 129
    rec, sph = cr.default_record(w, h), gen_data.gen_spheres_open()[0]
    rays = cr.rays(rec, w, h, s, seed=13)
    vals = ft.path_values(rays, sph, 8, 1e-4)
    up, down = ft.pixel_means(vals, s), ft.pixel_means(vals, s, reverse=True)
    assert np.array_equal(up.view(np.uint32), down.view(np.uint32))
