"""GPU: the film's moments and its filter (libdenoise_mi355x.so, include/render_mi355x_denoise.h) through the C-ABI, bit for bit (NaN positions included)
against the CPU twins and the NumPy restatement tests/denoise_ref.py, with the status word clean.

  accumulate  apt_film_accumulate_device against apt_film_accumulate_host on 1 / 3 / 64 / 257 / 1001 pixels, pass 0 over NaN.
  Film        render.Film(moments=True) after 3 passes against a plain Film after the same 3 passes, bit for bit: two8 with APT_FLAG_NEE,
              open8 under the sky with the sun sampled.
  denoise     apt_film_denoise_device against apt_film_denoise_host on the CPU test's synthetic inputs: its shapes, heights at and just
              past a wave's 64 lanes and past two (3 x 64, 3 x 65, 2 x 130), and 9 x 5, two workgroups' 4 columns plus one; guard floats
              round work and out.
  end to end  a 48 x 32 diff8-lamp film of 4 NEE passes with its features through Film.denoise against the restatement, and
              Film.resolve(source=...) against film_ref.resolve of it with passes = 1.
  refusals    the device entry's.

On the parent every test here fails: the entries do not exist."""
import ctypes

import numpy as np
import pytest

import camera_ref as cr
import denoise_ref as dr
import features_ref as ft
import film_ref as fr
from gpu_harness import apt, assert_bits_equal, dev, oracle_params, scene, sky_and_sun  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
GUARD = dr.GUARD


def _sync():
    import torch
    torch.cuda.synchronize()


def test_accumulate_device_equals_the_twin(apt):
    import torch
    rng = np.random.default_rng(8)
    for n in (1, 3, 64, 257, 1001):
        ps = [(rng.random((3, n)) * 40).astype(F) for _ in range(3)]
        ps[1][2, n // 2] = np.nan
        film = torch.full((3, n), float("nan"), dtype=torch.float32, device="cuda")          # pass 0 stores over NaN
        mom = torch.full((2, n), float("nan"), dtype=torch.float32, device="cuda")
        for k, p in enumerate(ps):
            apt.render.film_accumulate(dev(p), film, mom, k)
        _sync()
        want_film, want_mom = dr.accumulate_host(apt, ps)
        dr.assert_same(film.cpu().numpy(), want_film)
        dr.assert_same(mom.cpu().numpy(), want_mom)
        assert np.isnan(want_film).sum() == 1 and np.isnan(want_mom).sum() == 2


@pytest.mark.parametrize("name", ["two8", "open8"])
def test_a_film_with_moments_is_the_plain_film(apt, name):
    sc = scene(apt, name)
    w, h = 24, 16
    env = sky_and_sun(apt) if name == "open8" else None
    p = sc.params(w, h, 3, 4, mode="nee" if name == "two8" else "plain", seed=9)
    with sc.view(None, env):
        plain, mom = apt.render.Film(w, h), apt.render.Film(w, h, moments=True)
        for _ in range(3):
            plain.add_pass(p, sc.d_sph, sc.d_mat)
            mom.add_pass(p, sc.d_sph, sc.d_mat)
        _sync()
    assert plain.passes == mom.passes == 3
    film = plain.buffer.cpu().numpy()
    assert_bits_equal(mom.buffer.cpu().numpy(), film)
    assert np.isfinite(film).all() and film.max() > 0
    # the moments are those of the three passes taken apart again: pass k alone is what a film of passes 0..k adds to one of 0..k-1
    m = mom.moments.cpu().numpy()
    assert np.isfinite(m).all() and (m[1] > 0).any() and np.all(m[0] >= 0)
    mom.reset()
    assert mom.passes == 0
    with pytest.raises(apt.AptError):
        apt.render.Film(w, h, pixel_begin=h, moments=True)
    with pytest.raises(apt.AptError):
        plain.denoise(p, sc.d_sph)


def _denoise_device(apt, rec, film, mom, feat, W, H):
    """apt_film_denoise_device inside guard floats -> (out [3][N], work [16 N], guards intact)."""
    import torch
    N = W * H
    wb = torch.full((16 * N + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
    ob = torch.full((3 * N + 2 * GUARD,), -7.0, dtype=torch.float32, device="cuda")
    work, out = wb[GUARD:GUARD + 16 * N], ob[GUARD:GUARD + 3 * N]
    assert work.data_ptr() % 16 == 0
    apt.render.film_denoise(rec, dev(film), dev(mom), dev(feat), W, H, work=work, out=out)
    _sync()
    wb, ob = wb.cpu().numpy(), ob.cpu().numpy()
    guards = (np.all(wb[:GUARD] == -7.0) and np.all(wb[GUARD + 16 * N:] == -7.0) and np.all(ob[:GUARD] == -7.0)
              and np.all(ob[GUARD + 3 * N:] == -7.0))
    return ob[GUARD:GUARD + 3 * N].reshape(3, N), wb[GUARD:GUARD + 16 * N], guards


@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape", dr.SHAPES + [(3, 64), (3, 65), (2, 130), (9, 5)], ids=lambda s: "%dx%d" % s)
def test_denoise_device_equals_the_twin(apt, shape, nan):
    W, H = shape
    ps, feat = dr.synthetic(W, H, passes=3, nan=nan)
    film, mom = dr.accumulate_host(apt, list(ps))
    for it in (range(1, 6) if shape == (33, 17) else (5,)):
        rec = apt._lib.film_denoise_record(3, it)
        rc, want, want_work, ok = dr.denoise_host(apt, rec, film, mom, feat, W, H)
        assert rc == 0 and ok
        out, work, guards = _denoise_device(apt, rec, film, mom, feat, W, H)
        assert guards
        dr.assert_same(out, want)
        dr.assert_same(work, want_work)                                           # every record of the work buffer too
        assert np.isnan(want).any() == nan
    apt.render.check_device_status()


def test_film_denoise_end_to_end(apt):
    """diff8-lamp, 48 x 32, 4 NEE passes of 2 samples: Film.denoise is the restatement of the film, its moments and its features, and
    Film.resolve(source=...) is film_ref.resolve of those planes with passes = 1."""
    import torch
    sc = scene(apt, "diff8-lamp")
    w, h, K = 48, 32, 4
    p = sc.params(w, h, 2, 4, mode="nee", seed=21)
    film = apt.render.Film(w, h, moments=True)
    for _ in range(K):
        film.add_pass(p, sc.d_sph, sc.d_mat)
    got = film.denoise(p, sc.d_sph)
    u8, y = film.resolve(exposure=1.5, tonemap="reinhard", white=4.0, want_float=True, source=got)
    _sync()
    apt.render.check_device_status()
    op = oracle_params(p)
    passes = [fr.render_pass(op, sc.sph, sc.mat, pass_index=k)[0] for k in range(K)]
    want_film, want_mom = dr.accumulate(passes)
    assert_bits_equal(film.buffer.cpu().numpy(), want_film)
    dr.assert_same(film.moments.cpu().numpy(), want_mom)
    feat = ft.planes(cr.default_record(w, h), w, h, p.samples, p.seed, sc.sph, sc.ns, p.eps)
    rec = apt._lib.film_denoise_record(K)
    want = dr.denoise(rec, want_film, want_mom, feat, w, h)
    dr.assert_same(got.cpu().numpy(), want)
    assert np.isfinite(want).all()
    want_y, want_u8 = fr.resolve(want, 1, 1.5, fr.TONEMAP_REINHARD, 1.0 / 16.0, apt.gen_data.film_curve("srgb"))
    assert_bits_equal(y.cpu().numpy(), want_y)
    assert np.array_equal(u8.cpu().numpy(), want_u8)
    # fewer iterations and another sigma reach the kernel: the restatement again
    got2 = film.denoise(p, sc.d_sph, iterations=2, sigma_l=1.0, features=dev(feat))
    _sync()
    dr.assert_same(got2.cpu().numpy(), dr.denoise(apt._lib.film_denoise_record(K, 2, sigma_l=1.0), want_film, want_mom, feat, w, h))


def test_device_refusals(apt):
    import torch
    L = apt._lib.denoise_lib()
    W, H = 5, 3
    N = W * H
    bufs = {k: torch.full((n,), -7.0, dtype=torch.float32, device="cuda") for k, n in
            (("film", 3 * N), ("mom", 2 * N), ("feat", 8 * N), ("work", 16 * N), ("out", 3 * N))}

    def call(rec, w=W, h=H, shift=0, **null):
        a = {k: (None if k in null else ctypes.c_void_p(t.data_ptr() + (shift if k == "work" else 0))) for k, t in bufs.items()}
        rc = L.apt_film_denoise_device(None if rec is None else ctypes.byref(rec), None, a["film"], a["mom"], a["feat"], w, h, a["work"], a["out"])
        assert rc != 0 and L.apt_film_denoise_last_error() != b""
        return rc

    good = lambda **kw: apt._lib.film_denoise_record(kw.pop("passes", 3), kw.pop("iterations", None), **kw)
    assert call(None) == APT_ERR_ARG
    for k in bufs:
        assert call(good(), **{k: True}) == APT_ERR_ARG
    assert call(good(), shift=4) == APT_ERR_ARG
    assert call(good(), w=0) == APT_ERR_ARG and call(good(), h=0) == APT_ERR_ARG
    assert call(good(passes=1)) == APT_ERR_ARG and call(good(passes=(1 << 24) + 1)) == APT_ERR_ARG
    assert call(good(iterations=0)) == APT_ERR_ARG and call(good(iterations=6)) == APT_ERR_ARG
    assert call(good(sigma_z=-1.0)) == APT_ERR_ARG and call(good(sigma_l=float("nan"))) == APT_ERR_ARG
    assert call(good(albedo_floor=0.0)) == APT_ERR_ARG
    assert call(good(), w=1 << 14, h=(1 << 14) + 1) == APT_ERR_ARG
    rec = good()
    rec.struct_size = 44
    assert call(rec) == APT_ERR_STRUCT
    a = bufs["film"]
    assert L.apt_film_accumulate_device(None, None, N, a.data_ptr(), bufs["mom"].data_ptr(), 0) == APT_ERR_ARG
    assert L.apt_film_accumulate_device(None, a.data_ptr(), 1 << 40, a.data_ptr(), bufs["mom"].data_ptr(), 0) == APT_ERR_ARG
    _sync()
    assert all(bool((t == -7.0).all()) for t in bufs.values())                    # nothing was written
