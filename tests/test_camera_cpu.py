"""CPU-only: the camera record (include/render_mi355x.h "camera") -- its host helpers against the restatement tests/camera_ref.py and
against properties that depend on neither, the restatement's rays against the oracle's (default record) and against plain geometry
(look-at, thin lens), every refusal, and the context state: a camera set makes the mirror frame entries refuse, without a GPU."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import camera_ref as cr

U53 = 2.0 ** -53          # unit roundoff of float64
U24 = 2.0 ** -24          # unit roundoff of float32


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data, render
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


# (eye, dir, up, scale, offset, aperture, focus, w, h): oblique, straight down each kind of axis, non-unit dir and up, non-square images
POSES = [
    ((50.0, 52.0, 295.6), (0.3, -0.2, -1.0), (0.0, 1.0, 0.0), 0.5135, 140.0, 0.0, 0.0, 64, 48),
    ((10.0, 40.0, 200.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 0.5135, 0.0, 0.0, 0.0, 31, 17),
    ((5.0, 5.0, 5.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), 1.25, 3.0, 0.0, 0.0, 16, 16),
    ((1.0, 80.0, 100.0), (0.0, -1.0, 0.0), (0.0, 0.0, -1.0), 0.7, 1.0, 0.5, 60.0, 48, 64),
    ((20.0, 30.0, 250.0), (12.0, -5.0, -170.0), (0.1, 7.0, 0.3), 0.5135, 100.0, 1.5, 172.5, 17, 31),
    ((-30.0, 60.0, 120.0), (3.0, -2.0, -4.0), (0.0, 10.0, 0.0), 2.0 * math.tan(math.radians(100.0) / 2), 0.0, 0.25, 40.0, 40, 24),
]


def _build(apt, pose):
    eye, dirv, up, scale, offset, aperture, focus, w, h = pose
    return apt.gen_data.camera(eye, dir=dirv, up=up, scale=scale, offset=offset, aperture=aperture, focus=focus, width=w, height=h)


def test_record_layout(apt):
    from ascendpathtracing_amd._lib import ApCamera
    assert ctypes.sizeof(ApCamera) == 184 and ApCamera.pos.offset == 8 and ApCamera.offset_over_focus.offset == 176
    assert ctypes.sizeof(apt.RenderParams) == 80                       # no new frame entries, no new field


def test_default_record_is_the_restatement_byte_for_byte(apt):
    for w, h in ((16, 16), (31, 17), (64, 48), (1920, 1080)):
        assert bytes(apt.gen_data.default_camera(w, h)) == cr.record_bytes(cr.default_record(w, h)), (w, h)


@pytest.mark.parametrize("shape", [(16, 16, 1), (31, 17, 3), (64, 48, 2), (24, 20, 9)])
def test_default_record_rays_are_the_oracles_bit_for_bit(apt, oracle, shape):
    w, h, s = shape
    for seed in (0, 7):
        want = oracle.gen_rays_counter(oracle.make_params(w, h, s, seed=seed))
        for rec in (cr.default_record(w, h), cr.from_ctypes(apt.gen_data.default_camera(w, h))):
            got = cr.rays(rec, w, h, s, seed=seed)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    lo, n = 37, 101                                                    # a path range of the same rays
    got = cr.rays(cr.default_record(w, h), w, h, s, seed=7, path_begin=lo, path_count=n)
    assert np.array_equal(got.view(np.uint32), want[:, lo:lo + n].view(np.uint32))


@pytest.mark.parametrize("pose", POSES)
def test_builder_is_the_restatement_byte_for_byte(apt, pose):
    assert bytes(_build(apt, pose)) == cr.record_bytes(cr.build_record(*pose))


def _fr(v):
    return [Fraction(float(x)) for x in v]


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


@pytest.mark.parametrize("pose", POSES)
def test_builder_frame_is_orthogonal_independent_of_the_restatement(apt, pose):
    """Checked in exact rational arithmetic on the doubles the library wrote, so the test adds no rounding of its own.  With u = 2^-53:
      g = dir / norm(dir): the norm (two FMAs and a product, a sqrt) is within 2.5 u relative, each quotient adds u: | |g|^2 - 1 | <= 8 u.
      c = cross(g, up): a component is two rounded products and a rounded difference, absolute error <= 3 u |g| |up|, so c is off by at
      most 3 sqrt(3) u |g| |up| -- relative to |c| = |g| |up| sin(theta) that is 5.2 u / sin(theta), the angle by which `right` can lean
      out of the plane normal to g; normalising adds 4 u in length, none in direction.  cross(cx, g) has sin = 1: its direction is good
      to 5.2 u + the lean of cx.  So every cosine below is bounded by 16 u / sin(theta), and the lengths |right|, |lens_v| by 1 +- 8 u:
      |cx| / |cy| = ((w * scale) / h) / scale up to two more roundings each: the squared ratio within 64 u of (w / h)^2."""
    eye, dirv, up, scale, offset, aperture, focus, w, h = pose
    cam = _build(apt, pose)
    g, cx, cy, lu, lv = _fr(cam.g), _fr(cam.cx), _fr(cam.cy), _fr(cam.lens_u), _fr(cam.lens_v)
    d, upf = _fr(dirv), _fr(up)
    c = [d[1] * upf[2] - d[2] * upf[1], d[2] * upf[0] - d[0] * upf[2], d[0] * upf[1] - d[1] * upf[0]]
    sin2 = _dot(c, c) / (_dot(d, d) * _dot(upf, upf))                 # exact sin^2 of the angle between dir and up
    assert sin2 > Fraction(1, 100)
    bound2 = Fraction(16 * U53) ** 2 / sin2                            # squared cosine bound
    assert abs(_dot(g, g) - 1) <= Fraction(8 * U53)
    for a, b in ((g, cx), (g, cy), (cx, cy), (g, lu), (g, lv), (lu, lv)):
        assert _dot(a, b) ** 2 <= bound2 * _dot(a, a) * _dot(b, b)
    for v in (lu, lv):
        assert abs(_dot(v, v) - 1) <= Fraction(16 * U53)
    ratio2 = _dot(cx, cx) * h * h / (_dot(cy, cy) * w * w)
    assert abs(ratio2 - 1) <= Fraction(64 * U53)
    # g points along dir, lens_v to up's side, and (right, up, -forward) is right-handed like the reference's frame
    assert _dot(g, d) > 0 and _dot(lv, upf) > 0 and _dot(cy, lv) > 0 and _dot(cx, lu) > 0
    ref = apt.gen_data.default_camera(64, 48)
    assert ref.cx[0] > 0 and ref.cy[1] > 0 and ref.g[2] < 0            # x right, y up, looking down -z
    up_ref = apt.gen_data.camera((50, 52, 295.6), dir=(0, -0.042612, -1), width=64, height=48)
    assert up_ref.cx[0] > 0 and up_ref.cy[1] > 0
    assert tuple(cam.pos) == tuple(float(x) for x in eye) and cam.offset == offset and cam.aperture == aperture
    assert cam.offset_over_focus == (offset / focus if aperture > 0 else 0.0)


def _line_distance(o, d, p):
    """Distance of point p from the line o + t d (float64 from the ray's fp32 values), and the distance of p from o."""
    o, d, p = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(p, np.float64)
    d = d / np.linalg.norm(d)
    r = p - o
    return float(np.linalg.norm(r - d * float(r @ d))), float(np.linalg.norm(r))


def _fp32_ray_bound(o, reach):
    """How far a ray rounded to fp32 can pass from a point it passes through exactly, `reach` from its origin: the origin moves by at
    most sqrt(3) * 2^-24 * max|o_k| (one rounding per component), the direction (components <= 1) turns by at most sqrt(3) * 2^-24,
    which is that times `reach` at the point.  1 % on top for the float64 evaluation of the distance."""
    return 1.01 * math.sqrt(3.0) * U24 * (float(np.max(np.abs(o))) + reach)


def test_the_central_ray_passes_through_the_target(apt):
    for eye, target, w, h, offset in (((50.0, 52.0, 295.6), (73.0, 16.5, 78.0), 64, 48, 140.0), ((-40.0, 90.0, 30.0), (27.0, 16.5, 47.0), 33, 20, 0.0),
                                      ((10.0, 10.0, 10.0), (10.0, 10.0, -90.0), 16, 16, 20.0)):
        for up in ((0, 1, 0), (0.2, 1.0, -0.1)):
            cam = apt.gen_data.camera(eye, target=target, up=up, vfov_deg=40.0, offset=offset, width=w, height=h)
            dist = math.dist(eye, target)
            assert cam.focus == pytest.approx(dist, rel=1e-15)         # focus None with a target: the distance to it
            ray = cr.rays_ab(cr.from_ctypes(cam), np.zeros(1), np.zeros(1))[:, 0]
            miss, reach = _line_distance(ray[:3], ray[3:], target)
            assert miss <= _fp32_ray_bound(ray[:3], reach), (eye, target, miss)
            assert np.dot(ray[3:].astype(np.float64), np.subtract(target, eye)) > 0
            # and the segment starts `offset` units of forward depth from the eye (forward component of d is 1 at the centre)
            assert abs(math.dist(ray[:3].astype(np.float64), eye) - offset) <= 4 * U24 * (np.max(np.abs(ray[:3])) + 1)


def test_lens_samples_of_one_image_point_meet_in_the_plane_in_focus(apt):
    rng = np.random.default_rng(5)
    for pose in (POSES[3], POSES[4], POSES[5]):
        cam = _build(apt, pose)
        rec = cr.from_ctypes(cam)
        n = 512
        ang, rad = rng.uniform(0, 2 * np.pi, n), np.sqrt(rng.uniform(0, 1, n)) * cam.aperture
        lx, ly = (np.cos(ang) * rad).astype(np.float32), (np.sin(ang) * rad).astype(np.float32)
        for a, b in ((0.0, 0.0), (0.37, -0.45), (-0.5, 0.5)):
            d = np.array([(cam.cx[k] * a + cam.cy[k] * b) + cam.g[k] for k in range(3)])
            point = np.array(cam.pos) + d * cam.focus                  # the point in focus: forward depth `focus` (d . g = 1)
            assert abs(float(d @ np.array(cam.g)) - 1.0) < 1e-12
            rays = cr.rays_ab(rec, np.full(n, a), np.full(n, b), lx, ly)
            origins = set()
            for i in range(n):
                miss, reach = _line_distance(rays[:3, i], rays[3:, i], point)
                assert miss <= _fp32_ray_bound(rays[:3, i], reach), (pose, a, b, i, miss)
                origins.add(rays[:3, i].tobytes())
            assert len(origins) > n // 2                               # the rays do start all over the lens
            # and at offset 0 every origin lies on the lens disc
            if cam.offset == 0.0:
                r = np.linalg.norm(rays[:3].astype(np.float64) - np.array(cam.pos)[:, None], axis=0)
                assert (r <= cam.aperture * (1 + 1e-6) + 4 * U24 * np.max(np.abs(cam.pos))).all()


def test_lens_points_cover_the_disc(apt):
    rec = cr.from_ctypes(_build(apt, POSES[4]))
    lx, ly = cr.lens_points(rec, seed=3, paths=np.arange(20000))
    r = np.hypot(lx.astype(np.float64), ly.astype(np.float64)) / rec["aperture"]
    assert r.max() <= 1 + 1e-6 and abs(float((r * r).mean()) - 0.5) < 0.01      # uniform over the disc: E r^2 = 1/2
    assert abs(float(lx.mean())) < 0.02 * rec["aperture"] and abs(float(ly.mean())) < 0.02 * rec["aperture"]
    other, _ = cr.lens_points(rec, seed=4, paths=np.arange(20000))
    assert not np.array_equal(other, lx)


def _fresh(apt):
    from ascendpathtracing_amd._lib import ApCamera
    c = ApCamera()
    c.struct_size = ctypes.sizeof(ApCamera)
    return c


def test_every_refusal_returns_its_code_and_writes_nothing(apt):
    L = apt._lib.lib()
    d3 = ctypes.c_double * 3
    dbl, u32 = ctypes.c_double, ctypes.c_uint32
    good = dict(eye=(1.0, 2.0, 3.0), dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), scale=0.5, offset=1.0, aperture=0.0, focus=0.0, w=16, h=16)

    def build(out, **kw):
        a = dict(good, **kw)
        ptr = lambda v: None if v is None else d3(*v)
        return L.apt_camera_build_host(ptr(a["eye"]), ptr(a["dir"]), ptr(a["up"]), dbl(a["scale"]), dbl(a["offset"]), dbl(a["aperture"]),
                                       dbl(a["focus"]), u32(a["w"]), u32(a["h"]), None if out is None else ctypes.byref(out))

    out = _fresh(apt)
    assert build(out) == 0 and L.apt_last_error() == b""
    inf, nan = float("inf"), float("nan")
    bad = [dict(eye=None), dict(dir=None), dict(up=None), dict(eye=(nan, 0, 0)), dict(dir=(0, inf, -1)), dict(up=(0, nan, 0)),
           dict(scale=nan), dict(offset=inf), dict(aperture=nan), dict(focus=inf), dict(dir=(0.0, 0.0, 0.0)), dict(up=(0.0, 0.0, 0.0)),
           dict(up=(0.0, 0.0, -2.0)), dict(up=(0.0, 0.0, 5.0)), dict(dir=(1.0, 1.0, 1.0), up=(3.0, 3.0, 3.0)), dict(scale=0.0),
           dict(scale=-1.0), dict(offset=-1.0), dict(aperture=-0.5), dict(aperture=1.0, focus=0.0), dict(aperture=1.0, focus=-3.0),
           dict(w=0), dict(h=0),
           # the magnitude bound of the fast float64 sequences
           dict(eye=(2.0 ** 31, 0, 0)), dict(dir=(0, 0, -2.0 ** 31)), dict(up=(0, 2.0 ** 31, 0)), dict(scale=2.0 ** 21), dict(scale=2.0 ** -21),
           dict(scale=2.0 ** 19, w=64, h=16), dict(offset=2.0 ** 31), dict(aperture=2.0 ** 21, focus=1.0), dict(aperture=1.0, focus=2.0 ** 31),
           dict(aperture=1.0, focus=2.0 ** -21)]
    for kw in bad:
        out = _fresh(apt)
        before = bytes(out)
        assert build(out, **kw) == 1, kw                               # APT_ERR_ARG
        assert bytes(out) == before and L.apt_last_status() == 1 and L.apt_last_error() != b"", kw
    assert build(None) == 1
    out = _fresh(apt)
    out.struct_size = 8
    before = bytes(out)
    assert build(out) == 2 and bytes(out) == before                     # APT_ERR_STRUCT
    assert L.apt_camera_default_host(u32(16), u32(16), ctypes.byref(out)) == 2 and bytes(out) == before
    assert L.apt_camera_default_host(u32(16), u32(16), None) == 1
    out = _fresh(apt)
    before = bytes(out)
    assert L.apt_camera_default_host(u32(0), u32(16), ctypes.byref(out)) == 1 and bytes(out) == before
    assert L.apt_camera_default_host(u32(16), u32(16), ctypes.byref(out)) == 0 and bytes(out) != before


def _bad_records(apt):
    """(what, record): hand-filled records apt_camera_check_host refuses with APT_ERR_ARG."""
    lens = _build(apt, POSES[4])
    pin = _build(apt, POSES[0])
    inf, nan = float("inf"), float("nan")
    out = [("nan pos", pin.copy(pos=(nan, 0.0, 0.0))), ("inf cx", pin.copy(cx=(inf, 0.0, 0.0))), ("nan focus", pin.copy(focus=nan)),
           ("nan oof", pin.copy(offset_over_focus=nan)), ("zero g", pin.copy(g=(0.0, 0.0, 0.0))), ("zero cx", pin.copy(cx=(0.0, 0.0, 0.0))),
           ("zero cy", pin.copy(cy=(0.0, 0.0, 0.0))), ("offset < 0", pin.copy(offset=-1.0)), ("aperture < 0", pin.copy(aperture=-1.0)),
           ("pos bound", pin.copy(pos=(0.0, -2.0 ** 31, 0.0))), ("cx bound", pin.copy(cx=(2.0 ** 21, 0.0, 0.0))),
           ("cy bound", pin.copy(cy=(0.0, 2.0 ** 21, 0.0))), ("g bound", pin.copy(g=(0.0, 0.0, -3.0))), ("offset bound", pin.copy(offset=2.0 ** 31)),
           ("lens focus 0", lens.copy(focus=0.0)), ("lens focus < 0", lens.copy(focus=-1.0)), ("lens focus bound", lens.copy(focus=2.0 ** 31)),
           ("lens focus tiny", lens.copy(focus=2.0 ** -21, offset_over_focus=lens.offset / 2.0 ** -21)),
           ("lens aperture bound", lens.copy(aperture=2.0 ** 21)), ("lens zero lens_u", lens.copy(lens_u=(0.0, 0.0, 0.0))),
           ("lens zero lens_v", lens.copy(lens_v=(0.0, 0.0, 0.0))), ("lens quotient", lens.copy(offset_over_focus=lens.offset_over_focus * 1.5)),
           ("lens_u bound", lens.copy(lens_u=(3.0, 0.0, 0.0)))]
    return pin, lens, out


def test_check_host_and_set_camera_refuse_the_same_records(apt):
    L = apt._lib.lib()
    pin, lens, bad = _bad_records(apt)
    ctx = ctypes.c_void_p(L.apt_context_create())
    try:
        assert L.apt_camera_check_host(ctypes.byref(pin)) == 0 and L.apt_camera_check_host(ctypes.byref(lens)) == 0
        # aperture 0: focus and the quotient are not read, whatever they hold (the second pin of the GPU tests relies on it)
        assert L.apt_camera_check_host(ctypes.byref(pin.copy(focus=-7.0, offset_over_focus=123.0))) == 0
        assert L.apt_camera_check_host(None) == 1
        short = pin.copy(struct_size=176)
        assert L.apt_camera_check_host(ctypes.byref(short)) == 2 and L.apt_context_set_camera(ctx, ctypes.byref(short)) == 2
        assert L.apt_context_set_camera(None, ctypes.byref(pin)) == 1
        one = ctypes.c_void_p(16)
        u64 = ctypes.c_uint64
        p = apt.make_params(16, 16, 1)
        refused = lambda: L.apt_context_render_frame(ctx, ctypes.byref(p), None, one, u64(0), u64(10), one, None) == 1 and b"camera" in L.apt_last_error()
        assert L.apt_context_set_camera(ctx, ctypes.byref(pin)) == 0 and refused()
        for what, rec in bad:
            assert L.apt_camera_check_host(ctypes.byref(rec)) == 1 and L.apt_last_error() != b"", what
            assert L.apt_context_set_camera(ctx, ctypes.byref(rec)) == 1, what
            assert refused(), what                                     # the previous camera is still in place
            p2 = apt.make_params(16, 16, 1)
            assert L.apt_gen_rays_camera_device(ctypes.byref(p2), ctypes.byref(rec), None, one) == 1, what
        assert L.apt_gen_rays_camera_device(ctypes.byref(p), None, None, one) == 1
        assert L.apt_gen_rays_camera_device(ctypes.byref(p), ctypes.byref(pin), None, None) == 1
        assert L.apt_gen_rays_camera_device(None, ctypes.byref(pin), None, one) == 1
        empty = apt.make_params(16, 16, 1, path_begin=1024)
        assert L.apt_gen_rays_camera_device(ctypes.byref(empty), ctypes.byref(pin), None, one) == 0       # an empty range is a no-op
        beyond = apt.make_params(16, 16, 1, path_begin=1000, path_count=100)
        assert L.apt_gen_rays_camera_device(ctypes.byref(beyond), ctypes.byref(pin), None, one) == 1
    finally:
        L.apt_context_destroy(ctx)


def test_mirror_frame_entries_refuse_with_a_camera_set_and_need_no_gpu(apt):
    L = apt._lib.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: the refusal comes first
    u64 = ctypes.c_uint64
    cam = apt.gen_data.camera((50, 52, 295.6), target=(50, 40, 80), width=16, height=16)
    p = apt.make_params(16, 16, 1)
    ctx = apt.render.Context()
    other = apt.render.Context()
    frame = lambda q, c=10: L.render_frame(q, None, one, u64(0), u64(c), one, None)
    cframe = lambda h, q, c=10: L.apt_context_render_frame(h, q, None, one, u64(0), u64(c), one, None)
    frame_mt = lambda q: L.apt_render_frame_mt(q, None, one, u64(1), u64(0), one, u64(0), u64(10), one, None)
    ids = (ctypes.c_int * 1)(0)
    sph = apt.gen_data.gen_spheres()
    handle = ctypes.c_void_p()
    multi = lambda q: L.apt_multi_create(ids, ctypes.c_uint32(1), ctypes.c_uint32(1), q, ctypes.c_void_p(sph.ctypes.data), ctypes.byref(handle))
    is_camera = lambda: b"camera" in L.apt_last_error() and L.apt_last_status() == 1
    try:
        ctx.set_camera(cam)
        assert cframe(ctx._h, ctypes.byref(p)) == 1 and is_camera()
        assert cframe(other._h, ctypes.byref(p), c=0) == 0               # another context has no camera
        apt.render.set_camera(cam)
        for call in (frame, frame_mt, multi):
            assert call(ctypes.byref(p)) == 1 and is_camera(), call
        # their existing refusals keep their codes, messages and order: the camera's comes last
        bad = apt.default_params(); bad.struct_size = 8
        assert frame(ctypes.byref(bad)) == 2 and frame_mt(ctypes.byref(bad)) == 2 and multi(ctypes.byref(bad)) == 2
        assert frame(None) == 1 and b"params is null" in L.apt_last_error()
        assert L.render_frame(ctypes.byref(p), None, None, u64(0), u64(10), one, None) == 1 and b"spheres/fb" in L.apt_last_error()
        assert frame(ctypes.byref(p), c=10 ** 9) == 1 and b"pixel range" in L.apt_last_error()
        assert frame(ctypes.byref(p), c=0) == 0                          # an empty range stays a no-op
        big = apt.make_params(16, 16, 1 << 20)
        assert frame(ctypes.byref(big)) == 1 and b"samples too large" in L.apt_last_error()
        s0 = apt.make_params(16, 16, 1, num_spheres=8, light_index=9)
        assert frame(ctypes.byref(s0)) == 3 and frame_mt(ctypes.byref(s0)) == 3
        nine = apt.make_params(16, 16, 1, num_spheres=9)
        assert frame_mt(ctypes.byref(nine)) == 3 and b"8-sphere" in L.apt_last_error()
        rr = apt.make_params(16, 16, 1, flags=apt.APT_FLAG_RR)
        assert frame_mt(ctypes.byref(rr)) == 1 and b"APT_FLAG_RR" in L.apt_last_error()
        assert L.apt_render_frame_mt(ctypes.byref(p), None, one, u64(1), u64(5), one, u64(0), u64(10), one, None) == 1 and b"checkpoint table" in L.apt_last_error()
        acc = apt.make_params(16, 16, 1, accel=4096)
        assert multi(ctypes.byref(acc)) == 1 and b"accel" in L.apt_last_error()
        # buffer-mode entries take rays and do not look at the camera (an empty range: nothing is launched)
        e = apt.make_params(16, 16, 1, path_begin=1024)
        assert L.render_do_ex(ctypes.byref(e), None, one, one, one) == 0
        assert L.apt_render_paths_materials(ctypes.byref(e), None, one, one, one, one) == 0
        assert L.apt_gen_rays_device(ctypes.byref(e), None, one) == 0
        # NULL: the reference's camera again, the entries accept again (without a GPU: they get as far as the device)
        apt.render.set_camera(None)
        ctx.set_camera(None)
        rc = multi(ctypes.byref(p))
        assert not is_camera() and rc in (0, apt._lib.APT_ERR_DEVICE)
        if rc == 0:
            L.apt_multi_destroy(handle)
        assert cframe(ctx._h, ctypes.byref(p), c=10 ** 9) == 1 and b"pixel range" in L.apt_last_error()
    finally:
        apt.render.set_camera(None)
        ctx.close()
        other.close()


def test_python_helpers(apt):
    g = apt.gen_data
    with pytest.raises(apt.AptError):
        g.camera((0, 0, 0), width=16, height=16)                       # neither dir nor target
    with pytest.raises(apt.AptError):
        g.camera((0, 0, 0), dir=(0, 0, -1), target=(0, 0, -5), width=16, height=16)
    with pytest.raises(apt.AptError):
        g.camera((0, 0, 0), dir=(0, 0, -1))                            # no image size
    with pytest.raises(apt.AptError):
        g.camera((0, 0, 0), dir=(0, 0, -1), aperture=1.0, width=16, height=16)   # a lens needs focus or target
    for v in (0.0, 180.0, -5.0):
        with pytest.raises(apt.AptError):
            g.camera((0, 0, 0), dir=(0, 0, -1), vfov_deg=v, width=16, height=16)
    with pytest.raises(apt.AptError, match="parallel"):
        g.camera((0, 0, 0), dir=(0, 1, 0), width=16, height=16)        # the default up
    c = g.camera((0, 0, 0), dir=(0, 0, -1), vfov_deg=90.0, width=32, height=16)
    assert math.hypot(*c.cy) == pytest.approx(2.0, rel=1e-14) and math.hypot(*c.cx) == pytest.approx(4.0, rel=1e-14)
    near = g.camera((0, 0, 0), dir=(0, 0, -1), vfov_deg=179.999, width=16, height=16)      # near the bound on the scale (2^20)
    assert 2.0 ** 17 < math.hypot(*near.cy) < 2.0 ** 20
    d = g.default_camera(16, 16)
    assert d.offset == 140.0 and d.aperture == 0.0 and tuple(d.pos) == (50.0, 52.0, 295.6)
    for name in ("apt_camera_default_host", "apt_camera_build_host", "apt_camera_check_host", "apt_context_set_camera", "apt_set_camera",
                 "apt_gen_rays_camera_device"):
        assert name in apt._lib.ABI_SYMBOLS
