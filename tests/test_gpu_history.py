"""GPU: temporal accumulation (libhistory_mi355x.so, include/render_mi355x_history.h) through the C-ABI and render.History, bit for bit
(NaN positions included) against the CPU twins and the NumPy restatement tests/history_ref.py.

  reproject   apt_film_history_device against apt_film_history_host on the CPU test's sizes and camera cases, on heights at and just
              past a wave's 64 lanes and past two (3 x 64, 3 x 65, 2 x 130), and 9 x 5; NaN-filled outputs inside guard floats; the
              first-frame form.
  export      apt_film_history_export_device against its twin on 1 / 63 / 64 / 65 / 1001 pixels.
  refusals    the device entries'.
  end to end  open8 under the sky and the sun at 48 x 32, six 1-sample frames from an eye that moves a unit a frame, through
              render.History: the history, its lengths and denoise_inputs() against the restatement, then film_denoise(passes = 2) and
              Film.resolve(source=...) against theirs; and the benefit condition on the pixels whose first surface is DIFF.

On the parent every test here fails: the library does not exist."""
import ctypes

import numpy as np
import pytest

import camera_ref as cr
import denoise_ref as dr
import features_ref as ft
import film_ref as fr
import history_ref as hr
import materials_ref as mr
from gpu_harness import apt, assert_bits_equal, dev, inside_pinhole, oracle_params, scene, sky_and_sun  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
GUARD = hr.GUARD


def _sync():
    import torch
    torch.cuda.synchronize()


def _history_device(apt, rec, cur_cam, prev_cam, cur, cur_feat, prev_feat, prev_hist, W, H):
    """render.film_history into a NaN-filled output inside guard floats -> (out [6][N], guards intact)."""
    import torch
    N = W * H
    block = torch.full((6 * N + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    block[:GUARD] = -7.0
    block[-GUARD:] = -7.0
    out = block[GUARD:GUARD + 6 * N].view(6, W, H)
    prev = None if prev_hist is None else (dev(prev_hist), dev(prev_feat), hr.ctypes_camera(apt, prev_cam))
    apt.render.film_history(rec, dev(cur), dev(cur_feat), hr.ctypes_camera(apt, cur_cam), out, prev)
    _sync()
    b = block.cpu().numpy()
    return b[GUARD:GUARD + 6 * N].reshape(6, N), bool(np.all(b[:GUARD] == -7.0) and np.all(b[-GUARD:] == -7.0))


@pytest.mark.parametrize("shape", hr.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_history_device_equals_the_twin(apt, shape):
    W, H = shape
    for name in ("same", "translate", "rotate", "behind"):
        args = hr.case(W, H, name)
        for mh in ((1, 2, 32) if shape == (33, 17) else (32,)):
            rec = hr.record(apt, max_history=mh)
            rc, want, intact, _ = hr.history_host(apt, rec, *args, W, H)
            assert rc == 0 and intact
            got, guards = _history_device(apt, rec, *args, W, H)
            assert guards
            hr.assert_same(got, want)
    # NaN in the guides and in the values, and the first-frame form
    cc, pc, cur, cf, pf, hist = hr.case(W, H, "translate", seed=3)
    N = W * H
    for a in (cur, cf, pf, hist):
        for p in range(a.shape[0]):
            a[p, (3 + 5 * p) % N] = np.nan
    rec = hr.record(apt)
    for args in ((cc, pc, cur, cf, pf, hist), (cc, None, cur, cf, None, None)):
        rc, want, intact, _ = hr.history_host(apt, rec, *args, W, H)
        assert rc == 0 and intact
        got, guards = _history_device(apt, rec, *args, W, H)
        assert guards
        hr.assert_same(got, want)
    assert (got[5] == 1).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1001])
def test_export_device_equals_the_twin(apt, n):
    import torch
    hist = hr.export_case(n)
    rc, want_film, want_mom = hr.export_host(apt, hist)
    assert rc == 0
    fb = torch.full((3 * n + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
    mb = torch.full((2 * n + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
    film, mom = apt.render.film_history_export(dev(hist), fb[GUARD:GUARD + 3 * n], mb[GUARD:GUARD + 2 * n])
    _sync()
    hr.assert_same(film.cpu().numpy().reshape(3, n), want_film)
    hr.assert_same(mom.cpu().numpy().reshape(2, n), want_mom)
    for b, k in ((fb, 3), (mb, 2)):
        b = b.cpu().numpy()
        assert np.all(b[:GUARD] == -7.0) and np.all(b[GUARD + k * n:] == -7.0)
    f2, m2 = apt.render.film_history_export(dev(hist))                  # new tensors
    _sync()
    hr.assert_same(f2.cpu().numpy(), want_film)
    hr.assert_same(m2.cpu().numpy(), want_mom)


def test_device_refusals(apt):
    import torch
    L = apt._lib.history_lib()
    W, H = 5, 3
    N = W * H
    cc, pc, cur, cf, pf, hist = hr.case(W, H, "translate")
    c1, c2 = hr.ctypes_camera(apt, cc), hr.ctypes_camera(apt, pc)
    bufs = {"cur": dev(cur), "cf": dev(cf), "pf": dev(pf), "hist": dev(hist),
            "out": torch.full((6 * N,), -7.0, dtype=torch.float32, device="cuda")}

    def call(rec, cam1=c1, cam2=c2, w=W, h=H, alias=False, **null):
        a = {k: (None if k in null else ctypes.c_void_p(t.data_ptr())) for k, t in bufs.items()}
        rc = L.apt_film_history_device(None if rec is None else ctypes.byref(rec), None, None if cam1 is None else ctypes.byref(cam1),
                                       None if cam2 is None else ctypes.byref(cam2), a["cur"], a["cf"], a["pf"], a["hist"], w, h,
                                       a["hist"] if alias else a["out"])
        assert rc != 0 and L.apt_film_history_last_error() != b""
        return rc

    good = lambda **kw: hr.record(apt, **kw)
    assert call(None) == APT_ERR_ARG and call(good(), cam1=None) == APT_ERR_ARG and call(good(), cam2=None) == APT_ERR_ARG
    for k in ("cur", "cf", "pf", "out"):
        assert call(good(), **{k: True}) == APT_ERR_ARG
    assert call(good(), w=0) == APT_ERR_ARG and call(good(), h=0) == APT_ERR_ARG and call(good(), w=1 << 14, h=(1 << 14) + 1) == APT_ERR_ARG
    assert call(good(), alias=True) == APT_ERR_ARG
    assert call(good(max_history=0)) == APT_ERR_ARG and call(good(max_history=(1 << 24) + 1)) == APT_ERR_ARG
    assert call(good(tol_plane=-1.0)) == APT_ERR_ARG and call(good(tol_normal=float("nan"))) == APT_ERR_ARG
    assert call(good(min_weight=0.0)) == APT_ERR_ARG and call(good(min_weight=2.0)) == APT_ERR_ARG
    rec = good()
    rec.struct_size = 20
    assert call(rec) == APT_ERR_STRUCT
    bad = hr.ctypes_camera(apt, cc)
    bad.struct_size = 100
    assert call(good(), cam1=bad) == APT_ERR_STRUCT and call(good(), cam2=bad) == APT_ERR_STRUCT
    bad = hr.ctypes_camera(apt, cc)
    bad.cx[0] = float("inf")
    assert call(good(), cam1=bad) == APT_ERR_ARG
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    film, mom = torch.full((3 * N,), -7.0, device="cuda"), torch.full((2 * N,), -7.0, device="cuda")
    for a in ((None, N, p(film), p(mom)), (p(bufs["hist"]), N, None, p(mom)), (p(bufs["hist"]), N, p(film), None),
              (p(bufs["hist"]), 0, p(film), p(mom)), (p(bufs["hist"]), (1 << 28) + 1, p(film), p(mom))):
        assert L.apt_film_history_export_device(None, *a) == APT_ERR_ARG
    with pytest.raises(apt.AptError, match="max_history"):
        apt.render.film_history(good(max_history=0), bufs["cur"], bufs["cf"], c1, bufs["out"].view(6, W, H))
    with pytest.raises(apt.AptError, match="shape"):
        apt.render.film_history(good(), bufs["cur"], bufs["cf"], c1, bufs["out"])
    _sync()
    assert all(bool((t == -7.0).all()) for t in (bufs["out"], film, mom))                # nothing was written
    assert_bits_equal(bufs["hist"].cpu().numpy(), hist)


# ---- end to end through render.History ------------------------------------------------------------------------------------------------------
W, H, DEPTH, FRAMES, REF_PASSES = 48, 32, 4, 6, 64


def _camera(apt, k):
    """inside_pinhole with the eye moved k units along x: the target and every other field are its own."""
    return apt.gen_data.camera(width=W, height=H, aperture=0.0, eye=(20.0 + k, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05),
                               vfov_deg=55.0, offset=0.0)


def _clipped_mse(a, ref, mask):
    d = np.clip(a.astype(np.float64), 0, 1) - np.clip(ref.astype(np.float64), 0, 1)
    return float((d[:, mask] ** 2).mean())


def test_history_end_to_end_and_its_benefit(apt):
    """Six 1-sample frames (a film of one pass each, seeds 40 .. 45), Film.mean() and Film.features() of each pushed with its camera.

    The benefit is a condition, not a tolerance: over the pixels whose first surface is DIFF (coverage 1 and a DIFF sphere's albedo in
    the last frame's planes) the clipped MSE of the history's radiance against a 64-pass film of the last camera is below that of the
    last frame alone.  Measured on an MI355X: DESIGN.md "Temporal accumulation" and profiles/history_benefit.txt."""
    assert bytes(_camera(apt, 0)) == bytes(inside_pinhole(apt, W, H))
    sc = scene(apt, "open8")
    env = sky_and_sun(apt)
    menv = mr.Env.from_ctypes(env)
    history = apt.render.History(W, H)
    film = apt.render.Film(W, H)
    want = want_feat = prev_rec = None
    for k in range(FRAMES):
        cam = _camera(apt, k)
        p = sc.params(W, H, 1, DEPTH, seed=40 + k)
        with sc.view(cam, env):
            film.reset()
            film.add_pass(p, sc.d_sph, sc.d_mat)
            mean, feat = film.mean(), film.features(p, sc.d_sph)
        history.push(mean, feat, cam)
        _sync()
        apt.render.check_device_status()
        rec = cr.from_ctypes(cam)
        planes, _ = fr.render_pass(oracle_params(p), sc.sph, sc.mat, env=menv, rays=lambda seed: cr.rays(rec, W, H, 1, seed=seed))
        cur_feat = ft.planes(rec, W, H, 1, p.seed, sc.sph, sc.ns, p.eps)
        assert_bits_equal(mean.cpu().numpy(), planes)
        assert_bits_equal(feat.cpu().numpy(), cur_feat)
        want = hr.reproject(hr.DEFAULTS, rec, prev_rec, planes, cur_feat, want_feat, want, W, H)
        want_feat, prev_rec = cur_feat, rec
        hr.assert_same(history.buffer.cpu().numpy().reshape(6, -1), want)
        hr.assert_same(history.length().cpu().numpy(), want[5])
    assert history.frames == FRAMES and abs(want[5].max() - FRAMES) < 1e-4 and (want[5] == 1).sum() < W * H // 3   # (hl is a rounded quotient)
    last = planes

    e_film, e_mom = history.denoise_inputs()
    drec = apt._lib.film_denoise_record(2)
    den = apt.render.film_denoise(drec, e_film, e_mom, feat, W, H)
    u8, y = film.resolve(exposure=1.5, want_float=True, source=den)
    _sync()
    w_film, w_mom = hr.export(want)
    hr.assert_same(e_film.cpu().numpy(), w_film)
    hr.assert_same(e_mom.cpu().numpy(), w_mom)
    w_den = dr.denoise(drec, w_film, w_mom, want_feat, W, H)
    dr.assert_same(den.cpu().numpy(), w_den)
    w_y, w_u8 = fr.resolve(w_den, 1, 1.5, fr.TONEMAP_CLIP, 0.0, apt.gen_data.film_curve("srgb"))
    assert_bits_equal(y.cpu().numpy(), w_y)
    assert np.array_equal(u8.cpu().numpy(), w_u8)

    # the benefit: a 64-pass film of the last camera as the reference
    ref_film = apt.render.Film(W, H)
    p = sc.params(W, H, 1, DEPTH, seed=1000)
    with sc.view(cam, env):
        for _ in range(REF_PASSES):
            ref_film.add_pass(p, sc.d_sph, sc.d_mat)
        ref = ref_film.mean().cpu().numpy()
    table = sc.sph[:10 * sc.ns].reshape(10, sc.ns)
    diff = np.zeros(W * H, dtype=bool)
    for s in np.nonzero(sc.mat == mr.DIFF)[0]:
        diff |= (want_feat[ft.COVERAGE] == 1) & np.all(want_feat[ft.ALBEDO:ft.ALBEDO + 3] == table[7:10, s][:, None], axis=0)
    everything = np.ones(W * H, dtype=bool)
    assert diff.sum() > W * H // 4
    ratios = {name: _clipped_mse(want[:3], ref, m) / _clipped_mse(last, ref, m) for name, m in (("diff", diff), ("all", everything))}
    den_ratio = _clipped_mse(w_den, ref, everything) / _clipped_mse(last, ref, everything)
    print("history benefit: clipped MSE of the history / of the last frame alone: DIFF pixels %.4f (%d pixels), all pixels %.4f; "
          "denoised history / last frame, all pixels %.4f" % (ratios["diff"], diff.sum(), ratios["all"], den_ratio))
    assert ratios["diff"] < 1.0, ratios

    # reset(): the next push is a first frame again
    history.reset()
    history.push(mean, feat, cam)
    _sync()
    assert history.frames == 1 and bool((history.length() == 1).all())
    assert_bits_equal(history.radiance().cpu().numpy(), last)
    with pytest.raises(apt.AptError, match="no frame"):
        apt.render.History(W, H).buffer
