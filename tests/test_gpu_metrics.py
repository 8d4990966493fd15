"""GPU: film comparison metrics (libmetrics_mi355x.so, include/render_mi355x_metrics.h) through the C-ABI, render.film_compare /
film_ssim and Film.compare, bit for bit against the CPU twins and the NumPy restatement tests/metrics_ref.py.

  compare     apt_film_compare_device against apt_film_compare_host on the CPU test's sizes (they hold 1023, 1024 and 1025: both sides
              of a workgroup's chunk of 1024 pixels), on 70 001 pixels (69 rows) and on both sides of the fold's 4096 rows (4096 * 1024
              pixels and one more: the second fold launch); the films at a 16-byte boundary (16-byte loads where n is a multiple of 4) and
              4 bytes past it; work and result inside guard words, pre-filled with garbage; err_map NULL and not.
  ssim        apt_film_ssim_device against apt_film_ssim_host on the CPU test's sizes and at the tile's 16 x 64 windows +-1 in each axis;
              the map in work and the caller's (aligned and 4 bytes past), inside guards.
  refusals    the device entries'.
  end to end  the 32 x 24 lamp room (diff8-lamp): Film.compare of a 2-pass film against a 64-pass film of another seed equals the
              restatement of the films read back, field by field; more passes lower the clipped error.

Every case asserts bad == 0 unless it chose bad pixels itself.  On the parent every test here fails: the library does not exist."""
import ctypes

import numpy as np
import pytest

import metrics_ref as xr
from gpu_harness import apt, dev, scene  # noqa: F401

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
GUARD = xr.GUARD
GUARD64 = 0x5A5A5A5A5A5A5A5A
JUNK64 = 0x7BADF00D7BADF00D
FOLD_EDGE = xr.FOLD_ROWS * xr.CHUNK


def _sync():
    import torch
    torch.cuda.synchronize()


def _shifted(host, offset):
    """host float32 array -> a device tensor of its shape whose first float lies `offset` floats past a 16-byte boundary."""
    import torch
    flat = torch.empty(host.size + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    t = flat[offset:offset + host.size].view(*host.shape)
    t.copy_(torch.from_numpy(host))
    return t


def _words(n, fill=JUNK64):
    """n 64-bit words of garbage inside guard words -> (block int64, view)."""
    import torch
    to_i64 = lambda v: v - (1 << 64) if v >= 1 << 63 else v
    block = torch.full((n + 2 * GUARD,), to_i64(GUARD64), dtype=torch.int64, device="cuda")
    block[GUARD:GUARD + n] = to_i64(fill)
    return block, block[GUARD:GUARD + n]


def _words_intact(block, n):
    b = block.cpu().numpy().view(np.uint64)
    return bool(np.all(b[:GUARD] == GUARD64) and np.all(b[GUARD + n:] == GUARD64))


def _floats(n, offset=0):
    """n NaN floats inside guard floats, the first one `offset` floats past a 16-byte boundary -> (block, view)."""
    import torch
    block = torch.full((n + 2 * GUARD + 4,), -7.0, dtype=torch.float32, device="cuda")
    view = block[GUARD + offset:GUARD + offset + n]
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == 4 * offset
    return block, view


def _floats_intact(block, n, offset=0):
    b = block.cpu().numpy()
    return bool(np.all(b[:GUARD + offset] == -7.0) and np.all(b[GUARD + offset + n:] == -7.0))


def _compare_device(apt, rec, a, b, offset=0, want_map=True):
    """render.film_compare with work and result inside guards -> (result uint64 [8], err_map or None, guards intact)."""
    import torch
    n = a.shape[1]
    doubles = apt._lib.metrics_lib().apt_film_compare_work_doubles(n)
    wb, work = _words(doubles)
    rb, res = _words(xr.COMPARE_WORDS)
    mb, emap = _floats(n, offset) if want_map else (None, None)
    apt.render.film_compare(rec, _shifted(a, offset), _shifted(b, offset), work.view(torch.float64), res, emap)
    _sync()
    ok = _words_intact(wb, doubles) and _words_intact(rb, xr.COMPARE_WORDS) and (mb is None or _floats_intact(mb, n, offset))
    return res.cpu().numpy().view(np.uint64), None if emap is None else emap.cpu().numpy(), ok


@pytest.mark.parametrize("n", xr.COMPARE_SIZES + [70001])
def test_compare_device_equals_the_twin(apt, n):
    for k, (pa, pb) in enumerate(xr.COMPARE_PASSES):
        a, b = xr.compare_films(n, seed=10 * n + k)
        rec = xr.record(apt, pa, pb)
        rc, want, want_map, guards, _ = xr.compare_host(apt, rec, a, b)
        assert rc == 0 and guards and want[5] == 0 and want[6] == n
        for offset in (0, 1):
            for want_err in (True, False):
                got, got_map, ok = _compare_device(apt, rec, a, b, offset, want_err)
                assert ok
                assert np.array_equal(got, want), (n, pa, pb, offset, want_err, got, want)
                if want_err:
                    xr.assert_same(got_map, want_map)
    # around the display range with bad pixels the test chooses: every 5th from the second, NaN, inf and 2^60 in turn
    a, b = xr.display_films(n, seed=n)
    chosen = np.arange(1, n, 5)
    for j, i in enumerate(chosen):
        (a if j % 2 else b)[j % 3, i] = (np.nan, np.inf, -np.inf, 2.0 ** 60)[j % 4]
    rec = xr.record(apt, 1, 1, exposure=0.75, eps=1e-3)
    rc, want, want_map, _, _ = xr.compare_host(apt, rec, a, b)
    assert rc == 0 and want[5] == chosen.size and np.array_equal(want, xr.compare(a, b, 1, 1, 0.75, 1e-3)[0])
    for offset in (0, 1):
        got, got_map, ok = _compare_device(apt, rec, a, b, offset)
        assert ok and np.array_equal(got, want)
        xr.assert_same(got_map, want_map)
    apt.render.check_device_status()


def test_compare_device_tiny_values(apt):
    """Subnormal means (2^-145 .. 2^-105 over up to 2^24 passes): the device's quotients, by a division or by the exact multiply with
    2^-m, are the twin's and the restatement's."""
    a, b = xr.tiny_films(1025)
    for pa, pb in xr.TINY_PASSES:
        rec = xr.record(apt, pa, pb)
        rc, want, want_map, _, _ = xr.compare_host(apt, rec, a, b)
        assert rc == 0 and want[5] == 0 and np.array_equal(want, xr.compare(a, b, pa, pb)[0])
        for offset in (0, 1):
            got, got_map, ok = _compare_device(apt, rec, a, b, offset)
            assert ok and np.array_equal(got, want), (pa, pb, offset, got, want)
            xr.assert_same(got_map, want_map)
    apt.render.check_device_status()


@pytest.mark.parametrize("n", [FOLD_EDGE, FOLD_EDGE + 1])
def test_compare_device_at_the_fold_limit(apt, n):
    """4096 rows: one fold launch; 4097: a first fold to 2 rows, then the last one.  One film pair, tiled from 2^16 pixels (the sums'
    bits still depend on the order at every level: the test asserts it on the restatement of a slice)."""
    L = apt._lib.metrics_lib()
    assert L.apt_film_compare_work_doubles(FOLD_EDGE) == 6 * 4096 and L.apt_film_compare_work_doubles(FOLD_EDGE + 1) == 6 * (4097 + 2)
    sa, sb = xr.compare_films(1 << 16, seed=77)
    assert (xr.compare(sa, sb, wrong="sequential")[0][:4] != xr.compare(sa, sb)[0][:4]).any()
    reps = (n + (1 << 16) - 1) >> 16
    a = np.ascontiguousarray(np.tile(sa, (1, reps))[:, :n])
    b = np.ascontiguousarray(np.tile(sb, (1, reps))[:, :n])
    a[:, ::3] *= F(0.5)                                                  # so that the slices are not copies of one another
    rec = xr.record(apt)
    rc, want, want_map, guards, _ = xr.compare_host(apt, rec, a, b)
    assert rc == 0 and guards and want[5] == 0 and want[6] == n
    got, got_map, ok = _compare_device(apt, rec, a, b)
    assert ok and np.array_equal(got, want), (got, want)
    xr.assert_same(got_map, want_map)
    apt.render.check_device_status()


def _ssim_device(apt, rec, a, b, W, H, map_offset=None):
    """render.film_ssim with work and result inside guards; map_offset None: the map in work -> (result, map or None, guards intact)."""
    import torch
    windows = (W - 10) * (H - 10)
    doubles = (apt._lib.metrics_lib().apt_film_ssim_work_bytes(W, H) + 7) // 8
    wb, work = _words(doubles)
    rb, res = _words(xr.SSIM_WORDS)
    mb, smap = (None, None) if map_offset is None else _floats(windows, map_offset)
    apt.render.film_ssim(rec, dev(a), dev(b), W, H, work.view(torch.float64), res, smap)
    _sync()
    ok = _words_intact(wb, doubles) and _words_intact(rb, xr.SSIM_WORDS) and (mb is None or _floats_intact(mb, windows, map_offset))
    return res.cpu().numpy().view(np.uint64), None if smap is None else smap.cpu().numpy(), ok


TILE_SIZES = [(xr.TILE_X + 10 + dx, xr.TILE_Y + 10 + dy) for dx, dy in ((-1, -1), (0, 0), (1, 1), (1, -1), (-1, 1))]


@pytest.mark.parametrize("shape", xr.SSIM_SIZES + TILE_SIZES + [(60, 150)], ids=lambda s: "%dx%d" % s)
def test_ssim_device_equals_the_twin(apt, shape):
    W, H = shape
    for k, (pa, pb, ex) in enumerate(((1, 1, 1.0), (3, 64, 0.8))):
        a, b = xr.ssim_films(W, H, seed=k)
        a, b = a * F(pa), b * F(pb)
        rec = xr.record(apt, pa, pb, exposure=ex)
        rc, want, want_map, guards, _ = xr.ssim_host(apt, rec, a, b, W, H)
        assert rc == 0 and guards and want[1] == (W - 10) * (H - 10)
        assert xr.compare_host(apt, rec, a, b)[1][5] == 0
        for map_offset in (None, 0, 1):
            got, got_map, ok = _ssim_device(apt, rec, a, b, W, H, map_offset)
            assert ok
            assert np.array_equal(got, want), (shape, map_offset, got, want)
            if got_map is not None:
                xr.assert_same(got_map, want_map)
    # an image against itself: 1 in every window, on the device too
    got, got_map, ok = _ssim_device(apt, xr.record(apt), a, a.copy(), W, H, 0)
    assert ok and np.all(got_map == F(1)) and got[0:1].view(D)[0] == float((W - 10) * (H - 10))
    apt.render.check_device_status()


def test_device_refusals(apt):
    import torch
    L = apt._lib.metrics_lib()
    nan, inf = float("nan"), float("inf")
    p = lambda t, shift=0: None if t is None else ctypes.c_void_p(t.data_ptr() + shift)
    n = 65
    ha, hb = xr.display_films(n, seed=1)
    a, b = dev(ha), dev(hb)
    work = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    res = torch.full((8,), 7, dtype=torch.int64, device="cuda")
    emap = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    good = lambda **kw: xr.record(apt, 2, 3, **kw)

    def compare(rec, fa=a, fb=b, count=n, w=work, r=res, m=emap, shift=0):
        rc = L.apt_film_compare_device(None if rec is None else ctypes.byref(rec), None, p(fa), p(fb), count, p(w, shift), p(r), p(m))
        assert rc != 0 and L.apt_film_metrics_last_error() != b""
        return rc

    assert compare(None) == APT_ERR_ARG and compare(good(), fa=None) == APT_ERR_ARG and compare(good(), fb=None) == APT_ERR_ARG
    assert compare(good(), w=None) == APT_ERR_ARG and compare(good(), r=None) == APT_ERR_ARG
    assert compare(good(), count=0) == APT_ERR_ARG and compare(good(), count=(1 << 28) + 1) == APT_ERR_ARG
    assert compare(good(), shift=4) == APT_ERR_ARG
    assert compare(good(), r=a) == APT_ERR_ARG and compare(good(), m=b) == APT_ERR_ARG and compare(good(), w=a) == APT_ERR_ARG
    assert compare(good(), m=res) == APT_ERR_ARG and compare(good(), w=res) == APT_ERR_ARG
    for kw in (dict(exposure=0.0), dict(exposure=nan), dict(exposure=inf), dict(eps=0.0), dict(eps=-1.0), dict(eps=nan)):
        assert compare(good(**kw)) == APT_ERR_ARG, kw
    rec = good()
    rec.passes_a = (1 << 24) + 1
    assert compare(rec) == APT_ERR_ARG
    rec = good()
    rec.struct_size = 28
    assert compare(rec) == APT_ERR_STRUCT
    with pytest.raises(apt.AptError, match="eps"):
        apt.render.film_compare(good(eps=0.0), a, b)
    with pytest.raises(apt.AptError, match="work"):
        apt.render.film_compare(good(), dev(np.zeros((3, 5000), F)), dev(np.zeros((3, 5000), F)), work=work[:6])

    W, H = 12, 11
    hsa, hsb = xr.ssim_films(W, H)
    sa, sb = dev(hsa), dev(hsb)
    swork = torch.full((8,), 7.0, dtype=torch.float64, device="cuda")
    sres = torch.full((2,), 7, dtype=torch.int64, device="cuda")
    smap = torch.full((4,), -7.0, dtype=torch.float32, device="cuda")

    def ssim(rec, fa=sa, fb=sb, w=W, h=H, wk=swork, r=sres, m=smap, shift=0):
        rc = L.apt_film_ssim_device(None if rec is None else ctypes.byref(rec), None, p(fa), p(fb), w, h, p(wk, shift), p(r), p(m))
        assert rc != 0 and L.apt_film_metrics_last_error() != b""
        return rc

    assert ssim(None) == APT_ERR_ARG and ssim(good(), fa=None) == APT_ERR_ARG and ssim(good(), fb=None) == APT_ERR_ARG
    assert ssim(good(), wk=None) == APT_ERR_ARG and ssim(good(), r=None) == APT_ERR_ARG
    for w, h in ((10, 11), (11, 10), (0, 11), (1 << 14, (1 << 14) + 1)):
        assert ssim(good(), w=w, h=h) == APT_ERR_ARG, (w, h)
    assert ssim(good(), shift=8) == APT_ERR_ARG
    assert ssim(good(), r=sa) == APT_ERR_ARG and ssim(good(), m=sb) == APT_ERR_ARG and ssim(good(), wk=sb) == APT_ERR_ARG
    assert ssim(good(exposure=-1.0)) == APT_ERR_ARG and ssim(good(eps=nan)) == APT_ERR_ARG
    rec = good()
    rec.struct_size = 20
    assert ssim(rec) == APT_ERR_STRUCT
    with pytest.raises(apt.AptError, match="at least 11"):
        apt.render.film_ssim(good(), dev(np.zeros((3, 100), F)), dev(np.zeros((3, 100), F)), 10, 10)
    band = apt.render.Film(W, H, pixel_begin=H)
    with pytest.raises(apt.AptError, match="band"):
        band.compare(torch.zeros((3, band.pixel_count), device="cuda"))
    with pytest.raises(apt.AptError, match="no pass"):
        apt.render.Film(W, H).compare(torch.zeros((3, W * H), device="cuda"))
    _sync()
    assert all(bool((t == 7).all()) for t in (work, res, swork, sres)) and all(bool((t == -7.0).all()) for t in (emap, smap))
    for t, h in ((a, ha), (b, hb), (sa, hsa), (sb, hsb)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), h.view(np.uint32))


def test_metrics_end_to_end(apt):
    """diff8-lamp (the closed room under smallpt's small lamp), 32 x 24, NEE passes of 1 sample and depth 4.  Film.compare of a 2-pass
    film against a 64-pass film of another seed: every field is the restatement's of the two films read back (psnr by the same Python
    expression on both sides); so is a band with ssim=False, and a `source`.  16 passes are closer to the reference than 1."""
    sc = scene(apt, "diff8-lamp")
    w, h = 32, 24
    p = sc.params(w, h, 1, 4, mode="nee", seed=33)
    p_ref = sc.params(w, h, 1, 4, mode="nee", seed=1234)
    ref = apt.render.Film(w, h)
    for _ in range(64):
        ref.add_pass(p_ref, sc.d_sph, sc.d_mat)
    film = apt.render.Film(w, h)
    got = {}
    for k in range(16):
        film.add_pass(p, sc.d_sph, sc.d_mat)
        if k + 1 in (1, 2, 16):
            got[k + 1] = (film.compare(ref, exposure=1.5, eps=1e-3), film.buffer.cpu().numpy().copy())
    mean2 = got[2][1] / F(2)
    via_source = film.compare(ref.mean(), exposure=1.5, eps=1e-3, source=dev(mean2))
    apt.render.check_device_status()

    hb = ref.buffer.cpu().numpy()
    for K in (1, 2, 16):
        d, ha = got[K]
        want = xr.summary(xr.compare(ha, hb, K, 64, 1.5, 1e-3)[0], xr.ssim(ha, hb, w, h, K, 64, 1.5)[0])
        assert set(d) == set(want) == {"mse", "clipped_mse", "rel_mse", "mae", "psnr", "max_abs", "max_index", "bad", "ssim"}
        assert d == want, (K, d, want)
        assert d["bad"] == 0 and 0 < d["clipped_mse"] < 1 and 0 < d["ssim"] < 1 and 0 <= d["max_index"] < w * h
    assert got[16][0]["clipped_mse"] < got[1][0]["clipped_mse"] and got[16][0]["ssim"] > got[1][0]["ssim"]
    hm = hb / F(64)
    assert via_source == xr.summary(xr.compare(mean2, hm, 1, 1, 1.5, 1e-3)[0], xr.ssim(mean2, hm, w, h, 1, 1, 1.5)[0])
    assert via_source == got[2][0]                                       # x / 2 and x / 64 are what the entries compute themselves
    # a band: compare takes it, SSIM refuses it
    n0, cnt = 5 * h, 9 * h
    band, band_ref = apt.render.Film(w, h, pixel_begin=n0, pixel_count=cnt), apt.render.Film(w, h, pixel_begin=n0, pixel_count=cnt)
    for _ in range(2):
        band.add_pass(p, sc.d_sph, sc.d_mat)
        band_ref.add_pass(p_ref, sc.d_sph, sc.d_mat)
    d = band.compare(band_ref, ssim=False)
    want = xr.summary(xr.compare(band.buffer.cpu().numpy(), band_ref.buffer.cpu().numpy(), 2, 2)[0])
    assert d == want and d["ssim"] is None and d["bad"] == 0
    with pytest.raises(apt.AptError, match="band"):
        band.compare(band_ref)
    with pytest.raises(apt.AptError, match="other pixels"):
        band.compare(ref, ssim=False)
