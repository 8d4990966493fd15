"""GPU: metering and bloom (libpost_mi355x.so, include/render_mi355x_post.h) through the C-ABI, render.film_meter / film_exposure /
film_bloom and Film.auto_exposure / Film.bloom, bit for bit (NaN positions included) against the CPU twins and the NumPy restatement
tests/post_ref.py.

  meter       apt_film_meter_device against apt_film_meter_host on the CPU test's sizes (64 pixels and the multiples of 4 take the
              16-byte loads, the others the 4-byte ones), on 70 001 and 70 000 pixels of ONE value (every lane on one bin) and spread
              over all bins (several workgroups, several rows of work), without pixels; work and hist inside guard words, hist
              pre-filled with garbage; a film at a 4-byte offset.
  bloom       apt_film_bloom_device against apt_film_bloom_host on the CPU test's sizes, on heights at and just past a wave's 64 lanes
              and past two (3 x 64, 3 x 65, 2 x 130), 9 x 5 and 64 x 48, at 1, 2 and 6 levels; out and work NaN-filled inside guard
              floats, every record of work compared; NaN / inf / negative films.
  refusals    the device entries'.
  end to end  the 32 x 24 lamp room (diff8-lamp), 4 film passes of depth 4: Film.auto_exposure(), Film.bloom() and
              Film.resolve(source=, exposure=) against post_ref and film_ref, byte for byte; then the same from the denoised mean.

On the parent every test here fails: the library does not exist."""
import ctypes

import numpy as np
import pytest

import camera_ref as cr
import denoise_ref as dr
import features_ref as ft
import film_ref as fr
import post_ref as pr
from gpu_harness import apt, assert_bits_equal, dev, oracle_params, scene  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
GUARD = pr.GUARD
GUARD_WORD = 0x5A5A5A5A


def _sync():
    import torch
    torch.cuda.synchronize()


def _meter_device(apt, rec, film, offset=0):
    """render.film_meter with work and hist inside guard words, both pre-filled with garbage -> (hist uint32 [257], guards intact).
    offset: the film's first float lies that many floats past a 16-byte boundary."""
    import torch
    n = film.shape[1]
    words = apt._lib.post_lib().apt_film_meter_work_words(n)
    wb = torch.full((words + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device="cuda")
    hb = torch.full((pr.WORDS + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device="cuda")
    wb[GUARD:GUARD + words] = 0x7BADF00D
    hb[GUARD:GUARD + pr.WORDS] = 0x7BADF00D
    d_film = torch.empty(3 * n + 8, dtype=torch.float32, device="cuda")
    assert d_film.data_ptr() % 16 == 0
    d_film = d_film[offset:offset + 3 * n].view(3, n)
    d_film.copy_(torch.from_numpy(film))
    hist = apt.render.film_meter(rec, d_film, wb[GUARD:GUARD + words],
                                 hb[GUARD:GUARD + pr.WORDS])
    _sync()
    w, h = wb.cpu().numpy(), hb.cpu().numpy()
    intact = all(bool(np.all(b[:GUARD] == GUARD_WORD) and np.all(b[GUARD + k:] == GUARD_WORD)) for b, k in ((w, words), (h, pr.WORDS)))
    return hist.cpu().numpy().view(np.uint32), intact


@pytest.mark.parametrize("n", pr.METER_SIZES + [1024, 70000, 70001])
def test_meter_device_equals_the_twin(apt, n):
    films = [(pr.meter_film(n, seed=n), 1), (pr.meter_film(n, seed=n + 1), 3)]
    if n >= 70000:
        films.append((np.full((3, n), 0.37, dtype=F), 1))              # every lane on one bin
        films.append((np.ascontiguousarray(np.tile(pr.bin_film(), (1, n // 256 + 1))[:, :n]), 1))   # spread over all bins
    for film, passes in films:
        rec = apt._lib.film_meter_record(passes)
        rc, want, intact, _ = pr.meter_host(apt, rec, film)
        assert rc == 0 and intact and int(want.sum()) == n
        for offset in ((0, 1) if n in (64, 1001, 70000) else (0,)):
            got, guards = _meter_device(apt, rec, film, offset)
            assert guards
            assert np.array_equal(got, want), (n, passes, offset, np.argwhere(got != want)[:5])
    if n >= 70000:
        assert want[:256].min() >= n // 256 and apt._lib.post_lib().apt_film_meter_work_words(n) == 69 * 257
    apt.render.check_device_status()


def test_meter_device_without_pixels_and_the_exposure(apt):
    import torch
    L = apt._lib.post_lib()
    rec = apt._lib.film_meter_record(1)
    hist = torch.full((pr.WORDS,), 0x7BADF00D, dtype=torch.int32, device="cuda")
    assert L.apt_film_meter_device(ctypes.byref(rec), None, None, 0, None, ctypes.c_void_p(hist.data_ptr())) == 0
    _sync()
    assert not hist.cpu().numpy().any()
    assert apt.render.film_exposure(rec, hist, prev=2.5) == 2.5         # nothing metered: the exposure stays
    film = pr.meter_film(1001, seed=9)
    h = apt.render.film_meter(rec, dev(film))                           # new work and hist tensors
    want = pr.meter(film, 1)
    for kw in ({}, dict(adapt=0.25), dict(low_q=1, high_q=65536, key=1.0)):
        r = apt._lib.film_meter_record(1, **kw)
        e = apt.render.film_exposure(r, h, prev=3.0)                    # reads the words back: synchronises
        assert F(e) == pr.exposure(dict(pr.METER_DEFAULTS, **kw), want, 3.0)
        assert apt.render.film_exposure(r, want, prev=3.0) == e         # a host array of the words
    with pytest.raises(apt.AptError, match="words"):
        apt.render.film_exposure(rec, want[:100])
    with pytest.raises(apt.AptError, match="work"):
        apt.render.film_meter(rec, dev(pr.meter_film(5000, seed=1)), work=torch.empty(257, dtype=torch.int32, device="cuda"))


def _bloom_device(apt, rec, film, W, H):
    """render.film_bloom into NaN-filled out and work inside guard floats -> (out [3][N], work, guards intact)."""
    import torch
    N = W * H
    floats = apt._lib.post_lib().apt_film_bloom_work_floats(W, H, rec.levels)
    ob = torch.full((3 * N + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    wb = torch.full((floats + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    for b in (ob, wb):
        b[:GUARD] = -7.0
        b[-GUARD:] = -7.0
    assert wb.data_ptr() % 16 == 0
    apt.render.film_bloom(rec, dev(film), W, H, wb[GUARD:GUARD + floats], ob[GUARD:GUARD + 3 * N].view(3, N))
    _sync()
    o, w = ob.cpu().numpy(), wb.cpu().numpy()
    intact = all(bool(np.all(b[:GUARD] == -7.0) and np.all(b[-GUARD:] == -7.0)) for b in (o, w))
    return o[GUARD:GUARD + 3 * N].reshape(3, N), w[GUARD:GUARD + floats], intact


@pytest.mark.parametrize("shape", pr.BLOOM_GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_bloom_device_equals_the_twin(apt, shape):
    W, H = shape
    for levels in pr.BLOOM_LEVELS:
        for bad, passes, kw in ((False, 1, {}), (True, 3, dict(threshold=0.5, cap=12.0, spread=0.75, intensity=0.3))):
            film = pr.bloom_film(W, H, seed=levels, bad=bad)
            rec = apt._lib.film_bloom_record(passes, levels=levels, **kw)
            rc, want, intact, _, want_work = pr.bloom_host(apt, rec, film, W, H, detail=True)
            assert rc == 0 and intact
            got, work, guards = _bloom_device(apt, rec, film, W, H)
            assert guards
            pr.assert_same(got, want)
            pr.assert_same(work, want_work)                            # every record of the pyramid too
            assert np.isnan(want).any() == bad
    apt.render.check_device_status()


def test_device_refusals(apt):
    import torch
    L = apt._lib.post_lib()
    nan, inf = float("nan"), float("inf")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    n = 65
    film = dev(pr.meter_film(n, seed=1))
    work = torch.full((257,), 7, dtype=torch.int32, device="cuda")
    hist = torch.full((257,), 7, dtype=torch.int32, device="cuda")
    good = lambda **kw: apt._lib.film_meter_record(2, **kw)

    def meter(rec, f=film, count=n, w=work, h=hist):
        rc = L.apt_film_meter_device(None if rec is None else ctypes.byref(rec), None, None if f is None else p(f), count,
                                     None if w is None else p(w), None if h is None else p(h))
        assert rc != 0 and L.apt_film_post_last_error() != b""
        return rc

    assert meter(None) == APT_ERR_ARG and meter(good(), f=None) == APT_ERR_ARG and meter(good(), w=None) == APT_ERR_ARG
    assert meter(good(), h=None) == APT_ERR_ARG and meter(good(), count=(1 << 28) + 1) == APT_ERR_ARG
    for kw in (dict(low_q=0), dict(low_q=60000), dict(high_q=65537), dict(key=0.0), dict(key=nan), dict(min_exposure=inf), dict(max_exposure=-1.0),
               dict(min_exposure=8.0, max_exposure=4.0), dict(adapt=-0.5), dict(adapt=2.0), dict(adapt=nan)):
        assert meter(good(**kw)) == APT_ERR_ARG, kw
    rec = good()
    rec.passes = 0
    assert meter(rec) == APT_ERR_ARG
    rec = good()
    rec.struct_size = 28
    assert meter(rec) == APT_ERR_STRUCT
    with pytest.raises(apt.AptError, match="adapt"):
        apt.render.film_meter(good(adapt=2.0), film)

    W, H = 5, 3
    N = W * H
    bfilm = dev(pr.bloom_film(W, H))
    floats = L.apt_film_bloom_work_floats(W, H, 2)
    bwork = torch.full((floats + 4,), -7.0, dtype=torch.float32, device="cuda")
    out = torch.full((3 * N,), -7.0, dtype=torch.float32, device="cuda")
    bgood = lambda **kw: apt._lib.film_bloom_record(2, **dict(dict(levels=2), **kw))

    def bloom(rec, f=bfilm, w=W, h=H, wk=bwork, o=out, shift=0):
        rc = L.apt_film_bloom_device(None if rec is None else ctypes.byref(rec), None, None if f is None else p(f), w, h,
                                     None if wk is None else ctypes.c_void_p(wk.data_ptr() + shift), None if o is None else p(o))
        assert rc != 0 and L.apt_film_post_last_error() != b""
        return rc

    assert bloom(None) == APT_ERR_ARG and bloom(bgood(), f=None) == APT_ERR_ARG and bloom(bgood(), wk=None) == APT_ERR_ARG
    assert bloom(bgood(), o=None) == APT_ERR_ARG and bloom(bgood(), w=0) == APT_ERR_ARG and bloom(bgood(), h=0) == APT_ERR_ARG
    assert bloom(bgood(), w=1 << 14, h=(1 << 14) + 1) == APT_ERR_ARG
    assert bloom(bgood(), shift=4) == APT_ERR_ARG and bloom(bgood(), o=bfilm) == APT_ERR_ARG
    for kw in (dict(levels=0), dict(levels=7), dict(threshold=-1.0), dict(threshold=nan), dict(cap=0.0), dict(cap=inf), dict(spread=-1.0),
               dict(spread=inf), dict(intensity=-0.1), dict(intensity=nan)):
        assert bloom(bgood(**kw)) == APT_ERR_ARG, kw
    rec = bgood()
    rec.passes = (1 << 24) + 1
    assert bloom(rec) == APT_ERR_ARG
    rec = bgood()
    rec.struct_size = 36
    assert bloom(rec) == APT_ERR_STRUCT
    with pytest.raises(apt.AptError, match="levels"):
        apt.render.film_bloom(bgood(levels=7), bfilm, W, H)
    band = apt.render.Film(W, H, pixel_begin=H)
    with pytest.raises(apt.AptError, match="band"):
        band.bloom()
    with pytest.raises(apt.AptError, match="no pass"):
        apt.render.Film(W, H).bloom()
    with pytest.raises(apt.AptError, match="no pass"):
        apt.render.Film(W, H).auto_exposure()
    _sync()
    assert all(bool((t == 7).all()) for t in (work, hist)) and all(bool((t == -7.0).all()) for t in (bwork, out))     # nothing was written
    assert_bits_equal(bfilm.cpu().numpy(), pr.bloom_film(W, H))


def test_post_end_to_end(apt):
    """diff8-lamp (the closed room under smallpt's small lamp), 32 x 24, 4 NEE film passes of 1 sample and depth 4.  The film's own
    sums with passes = 4, then the denoised mean as `source` with passes = 1: the metered exposure, the bloom planes and the resolved
    bytes are the restatements' of the restated film."""
    sc = scene(apt, "diff8-lamp")
    w, h, K = 32, 24, 4
    p = sc.params(w, h, 1, 4, mode="nee", seed=33)
    film = apt.render.Film(w, h, moments=True)
    for _ in range(K):
        film.add_pass(p, sc.d_sph, sc.d_mat)
    e = film.auto_exposure()
    e_slow = film.auto_exposure(prev=0.5, adapt=0.25, key=0.3)
    planes = film.bloom(levels=3, threshold=0.25, intensity=0.2)
    u8, y = film.resolve(exposure=e, tonemap="reinhard", white=4.0, want_float=True, source=planes)
    den = film.denoise(p, sc.d_sph)
    e_den = film.auto_exposure(source=den, prev=e)
    planes_den = film.bloom(source=den, levels=3, threshold=0.25, intensity=0.2)
    u8_den = film.resolve(exposure=e_den, source=planes_den)
    _sync()
    apt.render.check_device_status()

    op = oracle_params(p)
    passes = [fr.render_pass(op, sc.sph, sc.mat, pass_index=k)[0] for k in range(K)]
    want_film, want_mom = dr.accumulate(passes)
    assert_bits_equal(film.buffer.cpu().numpy(), want_film)
    hist = pr.meter(want_film, K)
    assert int(hist.sum()) == w * h and np.count_nonzero(hist[:256]) > 8          # the room spans more than an octave
    w_e = pr.exposure(pr.METER_DEFAULTS, hist, 1.0)
    assert F(e) == w_e and 2.0 ** -12 < e < 2.0 ** 12
    assert F(e_slow) == pr.exposure(dict(pr.METER_DEFAULTS, adapt=0.25, key=0.3), hist, 0.5)
    brec = dict(pr.BLOOM_DEFAULTS, levels=3, threshold=0.25, intensity=0.2)
    w_planes, B, _ = pr.bloom(brec, want_film, w, h, passes=K, detail=True)
    pr.assert_same(planes.cpu().numpy(), w_planes)
    assert B.max() > 0                                                            # the lamp is above the threshold: there is a glare
    w_y, w_u8 = fr.resolve(w_planes, 1, float(w_e), fr.TONEMAP_REINHARD, 1.0 / 16.0, apt.gen_data.film_curve("srgb"))
    assert_bits_equal(y.cpu().numpy(), w_y)
    assert np.array_equal(u8.cpu().numpy(), w_u8)

    feat = ft.planes(cr.default_record(w, h), w, h, p.samples, p.seed, sc.sph, sc.ns, p.eps)
    w_den = dr.denoise(apt._lib.film_denoise_record(K), want_film, want_mom, feat, w, h)
    dr.assert_same(den.cpu().numpy(), w_den)
    w_e_den = pr.exposure(pr.METER_DEFAULTS, pr.meter(w_den, 1), w_e)
    assert F(e_den) == w_e_den
    w_planes_den = pr.bloom(brec, w_den, w, h, passes=1)
    pr.assert_same(planes_den.cpu().numpy(), w_planes_den)
    _, w_u8_den = fr.resolve(w_planes_den, 1, float(w_e_den), fr.TONEMAP_CLIP, 0.0, apt.gen_data.film_curve("srgb"))
    assert np.array_equal(u8_den.cpu().numpy(), w_u8_den)
