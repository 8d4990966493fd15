"""GPU: the movable camera of the material renderer (include/render_mi355x.h "camera").
Pinned to the code that exists -- apt_camera_default_host's record set gives the no-camera launch bit for bit, and aperture 0 gives the
pinhole whatever `focus` holds --, then bit for bit against the NumPy restatement tests/camera_ref.py (rays, and frames through
materials_ref) for look-at cameras with and without a lens on all three scene forms, fused against buffers, and a
check that the lens blurs what is out of focus by the thin-lens circle of confusion, which depends on neither."""
import ctypes
import math

import numpy as np
import pytest

import camera_ref as cr
import lights_ref as lr
from gpu_harness import apt, bits_equal, dev, same, scene  # noqa: F401

pytestmark = pytest.mark.gpu
MODES = ["plain", "nee", "table"]


def _scene(apt, name):
    """two8: 8 spheres (SGPR form), two lamps; demo9x2: the demo scene with the glass ball (tiles), two lights; big: 1030 spheres by tiles
    and through a grid, a two-light table of the stock light and one lamp."""
    return scene(apt, "big1030x2" if name == "big" else name)


def _frame(sc, p, mode, cam=None, **kw):
    """-> (fb, u8, traced)"""
    return sc.frame(p, mode, cam, count=True, **kw)


# (samples, depth, roulette): both GROUP arms (samples < 8, >= 8), a tail (13 = 8 + 5), roulette
CASES = [(3, 5, True), (8, 5, False), (13, 8, True)]


# ---- the pin: the default record IS the camera every frame has had --------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["two8", "demo9x2", "big"])
def test_pin_default_record_is_the_frame_without_a_camera(apt, name, mode):
    sc = _scene(apt, name)
    big = name == "big"
    w, h = (24, 16) if big else (48, 32)
    cam = apt.gen_data.default_camera(w, h)
    for grid in ((True, False) if big else (False,)):
        for s_, depth, rr in CASES:
            p = sc.params(w, h, s_, depth, mode=mode, rr=rr, seed=11 + s_, grid=grid)
            want, got = _frame(sc, p, mode), _frame(sc, p, mode, cam)
            same(got, want)
            assert got[2] == want[2] > 0                           # the trace counter
        b, c = (117, 203) if big else (517, 700)                   # a mid-image pixel range
        p = sc.params(w, h, 16, 5, mode=mode, seed=2, grid=grid)
        want, got = _frame(sc, p, mode, pixel_begin=b, pixel_count=c), _frame(sc, p, mode, cam, pixel_begin=b, pixel_count=c)
        same(got, want)
        assert got[2] == want[2] > 0
    p136 = sc.params(w, h, 136, 2, mode=mode, seed=5, grid=big)       # two pairwise leaves: the LDS stack, next to the camera's tail in the plan
    same(_frame(sc, p136, mode, cam), _frame(sc, p136, mode))


def test_pin_gen_rays_camera_with_the_default_record_is_gen_rays_device(apt):
    import torch
    for w, h, s_, seed in ((16, 16, 1, 0), (31, 17, 3, 7), (64, 48, 9, 2)):
        p = apt.make_params(w, h, s_, seed=seed)
        want = apt.render.gen_rays_device(p)
        got = apt.render.gen_rays_camera(p, apt.gen_data.default_camera(w, h))
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        b, c = 101, 700                                               # inside the smallest image (1024 paths)
        q = p.copy(path_begin=b, path_count=c, flags=apt.APT_FLAG_BAND_BUFFERS)
        band = apt.render.gen_rays_camera(q, apt.gen_data.default_camera(w, h))
        torch.cuda.synchronize()
        assert band.shape == (6, c) and torch.equal(band.view(torch.int32), want[:, b:b + c].contiguous().view(torch.int32))
    apt.render.check_device_status()


# ---- the cameras of the restatement tests -----------------------------------------------------------------------------------------------
def _cameras(apt, w, h):
    """Three look-at cameras, each without and with a lens: oblique inside the room; inside the crowd of the 1030-sphere scene; a field of
    view near the bound on the scale (2 * tan(vfov / 2) <= 2^20, vfov = 179.9997 degrees)."""
    gd = apt.gen_data
    looks = [dict(eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05), vfov_deg=55.0, offset=0.0),
             dict(eye=(50.0, 40.0, 150.0), target=(45.0, 25.0, 40.0), vfov_deg=70.0, offset=2.0),
             dict(eye=(50.0, 40.0, 100.0), target=(50.0, 40.0, 0.0), vfov_deg=179.999, offset=0.0)]
    out = []
    for look in looks:
        out.append(gd.camera(width=w, height=h, **look))
        out.append(gd.camera(width=w, height=h, aperture=2.5, **look))   # focus None with a target: the distance to it
    assert out[5].cx[0] > 2.0 ** 17
    return out


def test_second_pin_aperture_zero_is_the_pinhole_whatever_focus_holds(apt):
    sc = _scene(apt, "demo9x2")
    w, h = 48, 32
    pin = _cameras(apt, w, h)[0]
    odd = pin.copy(focus=77.0, offset_over_focus=5.0, lens_u=(0.0, 1.0, 0.0))
    assert odd.aperture == 0.0
    for mode, (s_, depth, rr) in zip(MODES, CASES):
        p = sc.params(w, h, s_, depth, mode=mode, rr=rr, seed=4)
        want, got = _frame(sc, p, mode, pin), _frame(sc, p, mode, odd)
        same(got, want)
        assert got[2] == want[2]
        assert not np.array_equal(want[0], _frame(sc, p, mode)[0])    # and it is not the reference's viewpoint
    import torch
    p = apt.make_params(w, h, 3, seed=4)
    assert torch.equal(apt.render.gen_rays_camera(p, pin).view(torch.int32), apt.render.gen_rays_camera(p, odd).view(torch.int32))


@pytest.mark.parametrize("ci", range(6))
def test_gen_rays_camera_is_the_restatement_bit_for_bit(apt, ci):
    import torch
    for w, h, s_, seed in ((31, 17, 3, 7), (64, 48, 9, 2)):
        cam = _cameras(apt, w, h)[ci]
        rec = cr.from_ctypes(cam)
        p = apt.make_params(w, h, s_, seed=seed)
        n = p.num_paths
        want = cr.rays(rec, w, h, s_, seed=seed)
        got = apt.render.gen_rays_camera(p, cam).cpu().numpy()
        assert np.isfinite(got).all() and bits_equal(got, want)
        norm = np.linalg.norm(got[3:].astype(np.float64), axis=0)
        assert np.abs(norm - 1).max() < 1e-6
        # a path range of whole buffers: nothing outside it is written; and a band buffer
        b, c = 1003, 777
        buf = torch.full((6 * n,), float("nan"), dtype=torch.float32, device="cuda")
        q = p.copy(path_begin=b, path_count=c)
        apt._lib.check(apt._lib.lib().apt_gen_rays_camera_device(ctypes.byref(q), ctypes.byref(cam), None, ctypes.c_void_p(buf.data_ptr())),
                       "apt_gen_rays_camera_device")
        torch.cuda.synchronize()
        part = buf.cpu().numpy().reshape(6, n)
        assert bits_equal(part[:, b:b + c], want[:, b:b + c]) and np.isnan(part[:, :b]).all() and np.isnan(part[:, b + c:]).all()
        band = apt.render.gen_rays_camera(q.copy(flags=apt.APT_FLAG_BAND_BUFFERS), cam).cpu().numpy()
        assert band.shape == (6, c) and bits_equal(band, want[:, b:b + c])
        tail = apt.render.gen_rays_camera(p.copy(path_begin=n - 5, flags=apt.APT_FLAG_BAND_BUFFERS), cam).cpu().numpy()   # path_count 0: to the end
        assert tail.shape == (6, 5) and bits_equal(tail, want[:, n - 5:])
    if cam.aperture > 0:                                               # the lens does move the origins
        assert not bits_equal(got[:3], apt.render.gen_rays_camera(p, _cameras(apt, w, h)[ci - 1]).cpu().numpy()[:3])
    apt.render.check_device_status()


@pytest.mark.parametrize("ci", range(6))
def test_fused_frames_are_the_restatement_bit_for_bit(apt, ci):
    """Every camera on every scene form; over the six cameras every scene meets every light mode and every case of the pin list (both
    GROUP arms, a tail, roulette), and a mid-image pixel range; the grid frame equals the tile frame."""
    for si, name in enumerate(["two8", "demo9x2", "big"]):
        sc = _scene(apt, name)
        big = name == "big"
        w, h = (24, 16) if big else (48, 32)
        cam = _cameras(apt, w, h)[ci]
        mode = MODES[(ci + si) % 3]
        s_, depth, rr = CASES[(ci // 3 + ci + si) % 3]
        p = sc.params(w, h, s_, depth, mode=mode, rr=rr, seed=20 + ci, grid=big)
        got = _frame(sc, p, mode, cam)
        want = sc.frame_ref(p, mode, cam)[:2]
        same(got, want)
        assert got[0].max() > 0                                        # the camera sees something
        b, c = (117, 203) if big else (517, 700)
        part = _frame(sc, p, mode, cam, pixel_begin=b, pixel_count=c)
        same(part, (want[0][:, b:b + c], want[1][b:b + c]))
        if big:
            tiles = _frame(sc, sc.params(w, h, s_, depth, mode=mode, rr=rr, seed=20 + ci, grid=False), mode, cam)
            same(tiles, got)
            assert tiles[2] == got[2]


@pytest.mark.parametrize("name,mode", [("demo9x2", "plain"), ("demo9x2", "table"), ("two8", "nee"), ("big", "plain")])
def test_fused_equals_buffers(apt, name, mode):
    """gen_rays_camera -> render_paths(materials=) -> decode_color_device is the fused frame, bit for bit, for a lens camera."""
    import torch
    sc = _scene(apt, name)
    w, h = (24, 16) if name == "big" else (48, 32)
    cam = _cameras(apt, w, h)[1 if name != "big" else 3]
    assert cam.aperture > 0
    for s_, depth, rr in CASES:
        p = sc.params(w, h, s_, depth, mode=mode, rr=rr, seed=31, grid=name == "big")
        fused = _frame(sc, p, mode, cam)
        rays = apt.render.gen_rays_camera(p, cam)
        with apt.render.TraceCounter() as tc:
            colors = apt.render.render_paths(p, rays.reshape(-1), sc.d_sph, materials=sc.d_mat, lights=sc.d_table if mode == "table" else None)
        fb, u8 = apt.render.decode_color_device(p, colors)
        torch.cuda.synchronize()
        apt.render.check_device_status()
        same((fb.cpu().numpy(), u8.cpu().numpy()), fused)
        assert tc.value == fused[2]


def test_the_mirror_renderer_gets_the_camera_through_buffers_and_refuses_frames(apt, oracle):
    import torch
    w, h, s_ = 48, 32, 8
    cam = _cameras(apt, w, h)[1]
    sph = apt.gen_data.gen_spheres()
    d_sph = dev(sph)
    p = apt.make_params(w, h, s_, depth=5, seed=6)
    apt.render.set_camera(cam)
    try:
        with pytest.raises(apt.AptError, match="camera"):
            apt.render.render_frame(p, d_sph)
        rays = apt.render.gen_rays_camera(p, cam)                      # buffer mode does not look at the context's camera
        colors = apt.render.render_paths(p, rays.reshape(-1), d_sph)
        fb, u8 = apt.render.decode_color_device(p, colors)
        torch.cuda.synchronize()
    finally:
        apt.render.set_camera(None)
    want, _ = oracle.render_paths(oracle.Params.from_buffer_copy(bytes(p)), cr.rays(cr.from_ctypes(cam), w, h, s_, seed=6), sph)
    _, fb_w, u8_w = oracle.decode_color(want, w, h, s_)
    same((fb.cpu().numpy(), u8.cpu().numpy()), (fb_w, u8_w))
    fb2, _ = apt.render.render_frame(p, d_sph)                         # NULL: the entry accepts again
    torch.cuda.synchronize()
    assert fb2.shape == (3, w * h)


def test_a_plan_that_reaches_the_cameras_words_is_refused(apt):
    sc = _scene(apt, "two8")
    cam = apt.gen_data.default_camera(8, 4)
    ok = sc.params(8, 4, 4199, 1)                                 # the last count whose plan leaves the words free
    assert _frame(sc, ok, "plain", cam)[0].shape == (3, 32)
    many = sc.params(8, 4, 4200, 1)                               # the first with more than 44 leaves
    assert _frame(sc, many, "plain")[0].shape == (3, 32)            # fine without a camera
    with pytest.raises(apt.AptError, match="44 leaves"):
        _frame(sc, many, "plain", cam)


# ---- the lens does what a lens does ------------------------------------------------------------------------------------------------
def test_lens_blurs_by_the_circle_of_confusion(apt):
    """Two small emitting spheres on black at forward depths 20 and 60, camera at the origin looking down -z, depth 1 (a pixel is lit iff
    one of its samples hits a sphere), focus on the near one.  Along the image row through the centres the lit extent must be the
    sphere's pinhole projection widened, on each side, by the thin-lens circle of confusion aperture * |z - focus| / z (its radius in the
    plane in focus), in pixels.  Pixel i spans [i, i + 1); an edge is measured at the CENTRE of the outermost lit pixel.

    Tolerance: 2 pixels on the extent, 1 per edge, from pixel quantisation.  The samples of pixel i land in [i - 0.25, i + 1.25) (two
    sub-pixel columns, each jittered by a tent of half-width 0.5 pixel): 0.75 either side of its centre.  So the outermost pixel that CAN
    be lit has its centre at most 0.75 outside the edge, and some pixel has its centre within (0, 1] inside it; if that one is lit, the
    measured edge is within 1 pixel.  Small next to that: the projection + circle formula against the exact tangent construction
    (asserted below: < 0.15 pixel; the near sphere spans depths 19 .. 21, so its rim is not exactly in focus), and the row against the
    centres' line (each of the two rows tested holds that line in its band).
    Why that pixel is lit at this sample count: its samples reach at least 0.75 pixel into the lit region.  In focus the edge is sharp:
    a quarter of its samples hit.  Out of focus, a point t pixels inside the blurred edge is lit from the cap of the lens beyond
    1 - t / c of its radius (c = the circle of confusion in pixels, 6.4 here), a fraction ~0.6 (t / c)^1.5 of the lens: 2.4 % at
    t = 0.75, ~1 % on average over 0 < t < 0.75; with a third of the pixel's samples there, >= 0.3 % of its samples light it.  A pixel
    has 4 * 2048 = 8192 samples: it stays dark with probability 0.997^8192 < 1e-10.  The seed is fixed, so the outcome is reproducible."""
    import torch
    W, H, S = 256, 32, 2048
    scale, A, focus = 0.25, 1.5, 20.0
    spheres = [(-3.0, 20.0, 1.0), (15.0, 60.0, 3.0)]                   # (x, forward depth z, radius); y = 0
    rows = [[r, x, 0.0, -z, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0] for x, z, r in spheres]
    sph, mat = lr.table_of(rows), np.array([1, 1], dtype=np.int32)
    d_sph, d_mat = dev(sph), dev(mat)
    px_per_unit = H / scale                                            # pixels per unit length at forward depth 1
    p = apt.make_params(W, H, S, depth=1, num_spheres=2, light_index=-1, seed=12)

    def lit_extents(cam, j):
        apt.render.set_camera(cam)
        try:
            fb, _ = apt.render.render_frame(p, d_sph, materials=d_mat)
            torch.cuda.synchronize()
            apt.render.check_device_status()
        finally:
            apt.render.set_camera(None)
        row = fb.cpu().numpy()[0].reshape(W, H)[:, j] > 0             # pixel q = i * H + j
        out = []
        for lo, hi in ((0, W // 2), (W // 2, W)):                     # sphere 0 in the left half, sphere 1 in the right half
            idx = np.nonzero(row[lo:hi])[0] + lo
            assert idx.size and (np.diff(idx) == 1).all()              # one run of lit pixels, no holes
            out.append((idx[0] + 0.5, idx[-1] + 0.5))
        return out

    def predicted(x, z, r, aperture):
        """Edges in pixels: the pinhole projection of the sphere (tangent lines from the eye in the row's plane) -+ the circle of confusion."""
        mid, half = math.atan2(x, z), math.asin(r / math.hypot(x, z))
        coc = aperture * abs(z - focus) / z / focus                    # radius in the plane in focus, brought to forward depth 1
        to_px = lambda t: (t / (W * scale / H) + 0.5) * W
        lo, hi = to_px(math.tan(mid - half) - coc), to_px(math.tan(mid + half) + coc)
        # the exact construction: tangent lines from the lens's two extreme points, met with the plane in focus
        ex = []
        for lx in (-aperture, aperture):
            m, hf = math.atan2(x - lx, z), math.asin(r / math.hypot(x - lx, z))
            ex += [(lx + focus * math.tan(m - hf)) / focus, (lx + focus * math.tan(m + hf)) / focus]
        assert abs(to_px(min(ex)) - lo) < 0.15 and abs(to_px(max(ex)) - hi) < 0.15
        return lo, hi

    lens = apt.gen_data.camera((0, 0, 0), dir=(0, 0, -1), scale=scale, offset=0.0, aperture=A, focus=focus, width=W, height=H)
    pin = lens.copy(aperture=0.0)
    coc_px = A * (60.0 - focus) / 60.0 / focus * px_per_unit
    assert 6.3 < coc_px < 6.5
    for j in (H // 2, H // 2 - 1):                                     # the two rows next to the centres' line
        got_lens, got_pin = lit_extents(lens, j), lit_extents(pin, j)
        for k, (x, z, r) in enumerate(spheres):
            for got, aperture in ((got_lens[k], A), (got_pin[k], 0.0)):
                lo, hi = predicted(x, z, r, aperture)
                print(f"row {j} sphere {k} aperture {aperture}: lit {got}, predicted ({lo:.3f}, {hi:.3f})")
                assert abs(got[0] - lo) <= 1.0 and abs(got[1] - hi) <= 1.0, (j, k, aperture, got, (lo, hi))   # one pixel per edge
                assert abs((got[1] - got[0]) - (hi - lo)) <= 2.0       # the extent: 2 pixels
        # in focus the lens changes nothing beyond the tolerance; out of focus it widens the extent by two circles of confusion
        assert abs((got_lens[0][1] - got_lens[0][0]) - (got_pin[0][1] - got_pin[0][0])) <= 2.0
        assert abs((got_lens[1][1] - got_lens[1][0]) - (got_pin[1][1] - got_pin[1][0]) - 2 * coc_px) <= 2.0


# ---- cleanliness -----------------------------------------------------------------------------------------------------------------------
def test_a_contexts_camera_does_not_leak_into_another_context(apt):
    import torch
    sc = _scene(apt, "demo9x2")
    w, h = 48, 32
    cams = _cameras(apt, w, h)
    p = sc.params(w, h, 8, 5, seed=9)
    want_a, want_b, want_none = _frame(sc, p, "plain", cams[0]), _frame(sc, p, "plain", cams[3]), _frame(sc, p, "plain")
    assert not np.array_equal(want_a[0], want_b[0]) and not np.array_equal(want_a[0], want_none[0])
    a, b = apt.render.Context(), apt.render.Context()
    try:
        a.set_camera(cams[0])
        b.set_camera(cams[3])
        for _ in range(2):                                             # interleaved launches
            for ctx, want in ((a, want_a), (b, want_b)):
                fb, u8 = ctx.render_frame(p, sc.d_sph, materials=sc.d_mat)
                ctx.check()
                same((fb.cpu().numpy(), u8.cpu().numpy()), want)
            fb, u8 = apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat)     # the default context has none
            torch.cuda.synchronize()
            same((fb.cpu().numpy(), u8.cpu().numpy()), want_none)
        a.set_camera(None)
        fb, u8 = a.render_frame(p, sc.d_sph, materials=sc.d_mat)
        a.check()
        same((fb.cpu().numpy(), u8.cpu().numpy()), want_none)
        fb, u8 = b.render_frame(p, sc.d_sph, materials=sc.d_mat)
        b.check()
        same((fb.cpu().numpy(), u8.cpu().numpy()), want_b)
    finally:
        a.close()
        b.close()
    apt.render.check_device_status()
