"""CPU-only: metering and bloom (libpost_mi355x.so, include/render_mi355x_post.h) -- the binding against the header and the exports,
the CPU twins of the histogram and the bloom bit for bit against the restatement tests/post_ref.py, the exposure against it, what the
exposure and the bloom MEAN (the scaling law, the half-bin bound, the untouched film below the threshold, the geometric series on a
constant film, the support of one bright pixel), every refusal, and, on the restatement, that three wrong implementations are told
from the right one.

Without the feature nothing here passes: the library, the header, the binding and the restatement do not exist."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import materials_ref as mr
import post_ref as pr

F, D = np.float32, np.float64
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
NAMES = ["apt_film_meter_default_host", "apt_film_meter_work_words", "apt_film_meter_device", "apt_film_meter_host", "apt_film_exposure_host",
         "apt_film_bloom_default_host", "apt_film_bloom_work_floats", "apt_film_bloom_device", "apt_film_bloom_host", "apt_film_post_last_error"]


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data, render
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def _header_prototypes(name):
    """include/<name> -> {symbol: (restype, [argtypes])} in the header's order, by the binding's type rules."""
    scalars = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int, "float": ctypes.c_float}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(mr.ROOT, "include", name)).read(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = {}
    for statement in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(apt_[a-z0-9_]+)\s*\(([^()]*)\)\s*", statement)
        if m is None:
            continue
        ret, sym, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        args = [] if params == "void" else [ctypes.c_void_p if "*" in a else scalars[[w for w in a.split() if w != "const"][0]]
                                            for a in params.split(",")]
        assert sym not in found
        found[sym] = (ctypes.c_char_p if ret == "const char *" else scalars[ret], args)
    return found


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_symbols_records_and_defaults(apt):
    """A fifth library with a header of its own: the binding's table is that header's, entry by entry and in its order, the library
    exports those names and nothing else, and the other four libraries and their headers know none of them and export what they did."""
    from ascendpathtracing_amd._lib import ApFilmBloom, ApFilmMeter
    L = apt._lib.post_lib()
    assert ctypes.sizeof(ApFilmMeter) == 32 and ApFilmMeter.key.offset == 16 and ApFilmMeter.adapt.offset == 28
    assert ctypes.sizeof(ApFilmBloom) == 32 and ApFilmBloom.threshold.offset == 16 and ApFilmBloom.intensity.offset == 28
    header = _header_prototypes("render_mi355x_post.h")
    assert list(header) == NAMES
    table = apt._lib.POST_PROTOTYPES
    assert list(table) == list(header)
    for name, proto in header.items():
        assert (table[name][0], list(table[name][1])) == proto, name
        fn = getattr(L, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == list(table[name][1]), name
    assert _exports(apt._lib.POST_LIB_PATH) == set(header)
    new = set(header) | {"apt_film_meter", "apt_film_bloom"}
    others = (set(apt._lib.ABI_SYMBOLS) | set(apt._lib.DENOISE_PROTOTYPES) | set(apt._lib.ADAPTIVE_PROTOTYPES)
              | set(apt._lib.HISTORY_PROTOTYPES))
    assert not new & others
    assert _exports(apt._lib.LIB_PATH) == set(apt._lib.PROTOTYPES)
    assert _exports(apt._lib.DENOISE_LIB_PATH) == set(apt._lib.DENOISE_PROTOTYPES)
    assert _exports(apt._lib.ADAPTIVE_LIB_PATH) == set(apt._lib.ADAPTIVE_PROTOTYPES)
    assert _exports(apt._lib.HISTORY_LIB_PATH) == set(apt._lib.HISTORY_PROTOTYPES)
    for h in ("render_mi355x.h", "render_mi355x_denoise.h", "render_mi355x_adaptive.h", "render_mi355x_history.h"):
        assert not re.search(r"\b(%s)\b" % "|".join(sorted(new)), open(os.path.join(mr.ROOT, "include", h)).read()), h
    assert apt._lib.lib().apt_abi_version() == 3
    assert (apt._lib.APT_METER_BINS, apt._lib.APT_METER_WORDS) == (pr.BINS, pr.WORDS) == (256, 257)

    m = apt._lib.film_meter_record(7)
    assert (m.struct_size, m.passes, m.low_q, m.high_q) == (32, 7, 6554, 58982)
    assert (m.key, m.min_exposure, m.max_exposure, m.adapt) == (F(0.18), F(2.0 ** -12), F(2.0 ** 12), F(1))
    assert {k: getattr(m, k) for k in pr.METER_DEFAULTS} == {k: (v if isinstance(v, int) else F(v)) for k, v in pr.METER_DEFAULTS.items()}
    b = apt._lib.film_bloom_record(3)
    assert (b.struct_size, b.passes, b.levels, b.reserved) == (32, 3, 5, 0)
    assert (b.threshold, b.cap, b.spread, b.intensity) == (F(1), F(2.0 ** 16), F(1), F(0.05))
    for fn, rec in ((L.apt_film_meter_default_host, m), (L.apt_film_bloom_default_host, b)):
        assert fn(None, 1) == APT_ERR_ARG and b"null" in L.apt_film_post_last_error()
        assert fn(ctypes.byref(rec), 0) == APT_ERR_ARG and fn(ctypes.byref(rec), (1 << 24) + 1) == APT_ERR_ARG
        assert fn(ctypes.byref(rec), 1 << 24) == 0 and L.apt_film_post_last_error() == b"" and rec.passes == 1 << 24
    assert apt._lib.film_meter_record(2, key=0.5, low_q=1).key == F(0.5)
    assert apt._lib.film_bloom_record(2, levels=3).levels == 3
    with pytest.raises(apt.AptError):
        apt._lib.film_meter_record(2, sigma=1.0)
    with pytest.raises(apt.AptError):
        apt._lib.film_bloom_record(2, key=1.0)
    for name in ("film_meter", "film_exposure", "film_bloom"):
        assert hasattr(apt.render, name)
    for name in ("auto_exposure", "bloom"):
        assert hasattr(apt.render.Film, name)
    # (build_id() hashes public_headers(): tests/test_film_stage_cpu.py holds it to the hand-written list)
    assert os.path.join(mr.ROOT, "include", "render_mi355x_post.h") in apt._lib.public_headers()
    # the work sizes: one row per 1024 pixels, at most 512; four floats per pyramid pixel
    W = L.apt_film_meter_work_words
    assert [W(n) for n in (0, 1, 1024, 1025, 512 * 1024, 1 << 28, (1 << 28) + 1)] == [0, 257, 257, 514, 512 * 257, 512 * 257, 0]
    Wf = L.apt_film_bloom_work_floats
    assert Wf(33, 17, 6) == 4 * sum(w * h for w, h in pr.level_sizes(33, 17, 6)) == 4 * (17 * 9 + 9 * 5 + 5 * 3 + 3 * 2 + 2 * 1 + 1 * 1)
    assert Wf(1, 1, 1) == 4 and Wf(1920, 1080, 5) == 4 * sum(w * h for w, h in pr.level_sizes(1920, 1080, 5))
    assert Wf(0, 4, 1) == 0 and Wf(4, 0, 1) == 0 and Wf(4, 4, 0) == 0 and Wf(4, 4, 7) == 0 and Wf(1 << 15, (1 << 13) + 1, 1) == 0


# ---- the meter's twin against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pr.METER_SIZES)
def test_meter_twin_equals_the_restatement(apt, n):
    for passes, seed in ((1, n), (3, n + 1), (1 << 24, n + 2)):
        film = pr.meter_film(n, seed=seed)
        rc, hist, intact, _ = pr.meter_host(apt, apt._lib.film_meter_record(passes), film)
        assert rc == 0 and intact
        idx = pr.meter_index(film, passes)
        assert np.array_equal(hist, np.bincount(idx, minlength=pr.WORDS))
        assert np.array_equal(hist, pr.meter(film, passes)) and int(hist.sum()) == n
    if n >= 64:                                                        # every edge pixel is among the first ten (a film of 1 pixel: one)
        film = pr.meter_film(n, seed=0)
        idx = pr.meter_index(film, 1)
        # 2^-16 | its predecessor | 2^16 | its predecessor | a subnormal | +0 | -0 | negative | +inf | NaN
        assert list(idx[:10]) == [0, 0, 255, 255, 0, 256, 256, 256, 255, 256]
        rc, hist, intact, _ = pr.meter_host(apt, apt._lib.film_meter_record(1), film)
        assert rc == 0 and np.array_equal(hist, pr.meter(film, 1)) and hist[256] >= 4


def test_meter_edges_one_value_per_bin_and_bands(apt):
    rec = apt._lib.film_meter_record(1)
    # the ten edge pixels alone
    rc, hist, intact, _ = pr.meter_host(apt, rec, pr.edge_pixels())
    assert rc == 0 and intact and (hist[0], hist[255], hist[256]) == (3, 3, 4) and hist.sum() == 10
    # the bins next to the edges: the successor of 2^-16's bin end, and the last value of bin 254
    first_of_1 = pr.bin_value(2)
    assert pr.meter_index(np.array(pr.with_lum(first_of_1), dtype=F).reshape(3, 1), 1)[0] == 1
    assert pr.meter_index(np.array(pr.with_lum(np.nextafter(first_of_1, F(0))), dtype=F).reshape(3, 1), 1)[0] == 0
    # one value per bin
    film = pr.bin_film()
    rc, hist, intact, _ = pr.meter_host(apt, rec, film)
    assert rc == 0 and intact and np.all(hist[:256] == 1) and hist[256] == 0
    assert np.array_equal(pr.meter_index(film, 1), np.arange(256))
    # no pixels: all zero, film not read
    rc, hist, intact, _ = pr.meter_host(apt, rec, None, n=0)
    assert rc == 0 and intact and not hist.any()
    # two bands add to the whole image
    film = pr.meter_film(1001, seed=5)
    whole = pr.meter_host(apt, rec, film)[1]
    for cut in (1, 64, 500, 1000):
        a = pr.meter_host(apt, rec, np.ascontiguousarray(film[:, :cut]))[1]
        b = pr.meter_host(apt, rec, np.ascontiguousarray(film[:, cut:]))[1]
        assert np.array_equal(a + b, whole)


# ---- the exposure ------------------------------------------------------------------------------------------------------------------------------
def _exposure_host(apt, rec, hist, prev=1.0):
    out = (ctypes.c_float * 3)(-7.0, -7.0, -7.0)
    hist = np.ascontiguousarray(hist, dtype=np.uint32)
    rc = apt._lib.post_lib().apt_film_exposure_host(ctypes.byref(rec), pr.ptr(hist), prev, ctypes.byref(out, 4))
    assert out[0] == -7.0 and out[2] == -7.0
    return rc, F(out[1])


def _hist(**bins):
    h = np.zeros(pr.WORDS, dtype=np.uint32)
    for b, c in bins.items():
        h[int(b[1:])] = c
    return h


def test_exposure_equals_the_restatement(apt):
    rng = np.random.default_rng(3)
    cases = [_hist(b100=5), _hist(b0=1), _hist(b255=9), _hist(b100=5, b256=1000),            # one bin
             _hist(b100=1, b131=1), _hist(b100=3, b101=1), _hist(b107=1000, b180=1),          # two bins
             _hist(b256=77), _hist(),                                                      # nothing metered
             pr.meter(pr.meter_film(1001, seed=2), 1), pr.meter(pr.bin_film(), 1),
             rng.integers(0, 1 << 20, pr.WORDS).astype(np.uint32), np.full(pr.WORDS, 0xFFFFFFFF, dtype=np.uint32)]
    fields = [{}, dict(low_q=1, high_q=65536), dict(low_q=32768, high_q=32768), dict(low_q=1, high_q=1), dict(low_q=65536, high_q=65536),
              dict(adapt=0.25), dict(adapt=0.0), dict(key=1.0, min_exposure=0.5, max_exposure=2.0), dict(min_exposure=3.0, max_exposure=3.0)]
    for h in cases:
        for kw in fields:
            rec = apt._lib.film_meter_record(1, **kw)
            for prev in (1.0, 0.0, 37.5):
                rc, got = _exposure_host(apt, rec, h, prev)
                want = pr.exposure(dict(pr.METER_DEFAULTS, **kw), h, prev)
                assert rc == 0 and got.view(np.uint32) == F(want).view(np.uint32), (kw, prev, got, want)
    # what the cases mean
    d = apt._lib.film_meter_record
    assert _exposure_host(apt, d(1), _hist(b256=77), 2.5) == (0, F(2.5))                     # all excluded: the exposure stays
    assert _exposure_host(apt, d(1), _hist(b100=5))[1] == F(0.18) / pr.bin_value(201)        # one bin: its middle
    assert _exposure_host(apt, d(1, low_q=1, high_q=65536), _hist(b100=1, b131=1))[1] == F(0.18) / pr.bin_value(232)   # (201 + 263) / 2
    assert _exposure_host(apt, d(1, low_q=1, high_q=65536), _hist(b100=3, b101=1))[1] == F(0.18) / pr.bin_value(201)   # floor(806 / 4)
    assert _exposure_host(apt, d(1), _hist(b107=1000, b180=1))[1] == F(0.18) / pr.bin_value(215)                         # the outlier is cut
    assert _exposure_host(apt, d(1, low_q=65536, high_q=65536), _hist(b107=1000, b180=1))[1] == F(0.18) / pr.bin_value(361)
    # the clamps at both ends
    assert _exposure_host(apt, d(1), _hist(b0=1))[1] == F(2.0 ** 12) and F(0.18) / pr.bin_value(1) > 2.0 ** 12
    assert _exposure_host(apt, d(1), _hist(b255=1))[1] == F(2.0 ** -12) and F(0.18) / pr.bin_value(511) < 2.0 ** -12
    # adapt: none of the way, a quarter of it, all of it
    t = F(0.18) / pr.bin_value(201)
    assert _exposure_host(apt, d(1, adapt=0.0), _hist(b100=5), 2.0)[1] == F(2.0)
    assert _exposure_host(apt, d(1, adapt=0.25), _hist(b100=5), 2.0)[1] == F(F(2.0) + F(t - F(2.0)) * F(0.25))
    assert _exposure_host(apt, d(1, adapt=1.0), _hist(b100=5), 2.0)[1] == t
    e, trail = F(2.0), []
    for _ in range(40):                                                # frame after frame the exposure approaches the metered one
        e = _exposure_host(apt, d(1, adapt=0.25), _hist(b100=5), float(e))[1]
        trail.append(abs(float(e) - float(t)))
    assert all(b <= a for a, b in zip(trail, trail[1:])) and trail[-1] < 1e-4 * float(t)


def test_exposure_scaling_law_and_the_half_bin_bound(apt):
    """Scaling a film by 2^k is exact in every operation of lum (no subnormal, no overflow here), so every luminance's bit pattern moves
    by k << 23 = 8 k bins: the histogram is the old one shifted, and while neither the range ends nor the clamps are reached the metered
    L scales by 2^k exactly and key / L by 2^-k exactly.

    The half-bin bound.  A film of constant luminance L0 fills one bin b, so m2 = 2 b + 1 and L is the value in the MIDDLE of bin b in
    its mantissa: with L0 = 2^e (1 + (t + f) / 8), t = 0 .. 7 the bin of its octave and 0 <= f < 1, L = 2^e (1 + (t + 1/2) / 8), and
    L0 / L = (8 + t + f) / (8.5 + t) lies in [(8 + t) / (8.5 + t), (9 + t) / (8.5 + t)), widest at t = 0: [16/17, 18/17).  The exposure
    is key / L rounded once, so exposure * L0 / key = L0 / L up to 2^-24, which matters only for an L0 within 2^-24 of a bin's end:
    the values below keep more than 1e-4 of a bin away from them, which the test asserts last."""
    rec = apt._lib.film_meter_record(1)
    rng = np.random.default_rng(11)
    film = (np.exp2(rng.uniform(-4, 4, (1, 1001))) * rng.uniform(0.5, 1.5, (3, 1001))).astype(F)
    base = pr.meter_host(apt, rec, film)[1]
    e0 = _exposure_host(apt, rec, base)[1]
    assert base[256] == 0 and base[:48].sum() == 0 and base[208:256].sum() == 0
    for k in (-5, -1, 1, 3, 5):
        h = pr.meter_host(apt, rec, np.ascontiguousarray(film * F(2.0 ** k)))[1]
        assert np.array_equal(np.roll(base[:256], 8 * k), h[:256]) and h[256] == 0
        ek = _exposure_host(apt, rec, h)[1]
        assert ek == F(e0 * F(2.0 ** -k)) and float(ek) == float(e0) * 2.0 ** -k
    nearest = 1.0
    for j in range(200):
        c = F(1e-4 * 1.137 ** j)                                      # 1e-4 .. 1.2e7: inside [2^-16, 2^16) until j = 158, beyond it after
        grey = np.full((3, 65), c, dtype=F)
        L0 = float(pr.lum(c, c, c))
        h = pr.meter_host(apt, rec, grey)[1]
        for key in (0.18, 1.0):
            r = apt._lib.film_meter_record(1, key=key, min_exposure=2.0 ** -40, max_exposure=2.0 ** 40)
            rc, e = _exposure_host(apt, r, h)
            assert rc == 0 and e == pr.exposure(dict(pr.METER_DEFAULTS, key=key, min_exposure=2.0 ** -40, max_exposure=2.0 ** 40), h, 1.0)
            if 2.0 ** -16 <= L0 < 2.0 ** 16:
                ratio = float(e) * L0 / float(F(key))
                assert 16 / 17 <= ratio <= 18 / 17, (j, c, ratio)
                frac = (np.array([L0], dtype=F).view(np.uint32)[0] & 0xFFFFF) / float(1 << 20)
                nearest = min(nearest, frac, 1 - frac)
    assert nearest > 1e-4


# ---- the bloom's twin against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", pr.BLOOM_LEVELS)
@pytest.mark.parametrize("shape", pr.BLOOM_SIZES, ids=lambda s: "%dx%d" % s)
def test_bloom_twin_equals_the_restatement(apt, shape, levels):
    """The output, every record of the work buffer, and B >= 0; with a NaN, a +inf and negative pixels in the film too."""
    W, H = shape
    for bad in (False, True):
        for passes, kw in ((1, {}), (3, dict(threshold=0.5, cap=12.0, spread=0.75, intensity=0.3))):
            film = pr.bloom_film(W, H, seed=levels, bad=bad)
            rec = apt._lib.film_bloom_record(passes, levels=levels, **kw)
            rc, out, intact, _, work = pr.bloom_host(apt, rec, film, W, H, detail=True)
            assert rc == 0 and intact
            want, B, U = pr.bloom(rec, film, W, H, detail=True)
            pr.assert_same(out, want)
            got_levels, pads = pr.work_levels(work, W, H, levels)
            assert [l.shape[1:] for l in got_levels] == pr.level_sizes(W, H, levels)
            for g, u, p in zip(got_levels, U, pads):
                pr.assert_same(g, u)
                assert not p.any()
            assert (B >= 0).all() and np.isfinite(B).all()
            bad_px = ~np.isfinite(film).all(0)
            assert bad_px.any() == bad
            nan_in = np.isnan(film / F(passes))
            assert np.array_equal(np.isnan(out), nan_in)               # a NaN stays in its own pixel (and channel) and reaches no other
    if shape == (33, 17) and levels == 6:
        assert pr.level_sizes(W, H, levels) == [(17, 9), (9, 5), (5, 3), (3, 2), (2, 1), (1, 1)]


def test_bloom_below_the_threshold_is_the_mean(apt):
    W, H = 33, 17
    rng = np.random.default_rng(2)
    film = (rng.random((3, W * H)) * 2.9).astype(F)                      # the sum of 3 passes: the mean's luminance stays below 1
    film[:, 5] = 0.0
    for levels in pr.BLOOM_LEVELS:
        rc, out, intact, _ = pr.bloom_host(apt, apt._lib.film_bloom_record(3, levels=levels, intensity=4.0), film, W, H)
        assert rc == 0 and intact
        assert float(pr.lum(*(film / F(3))).max()) < 1.0
        assert not pr.bits_differ(out, film / F(3))


def test_bloom_of_a_constant_film_is_the_geometric_series(apt):
    """A film of (c, c, c) with lum above the threshold: every pixel's bright value is v = x (l - thr) / l, every level of the pyramid
    is v again, and out = m + intensity * v * (1 + spread + .. + spread^(L-1)) =: T.

    The rounding bound, from the operation count, u = 2^-24, all terms positive so that relative errors of summands bound the sum's.
    The bright-pass: m (1), lum (5: the error of l is at most 3 u l since the partial sums are below l), l - thr (1, and the error of l
    enters amplified by l / (l - thr) = 4 / 3 for c = 4, thr = 1: 4 u + 1 u), the divisor's l (3), the divide (1), x * g (1): below
    12 u.  A down step: 16 products, 16 adds, a divide: 33 u.  An up step: 4 products, 4 adds: 8 u.  A combine or the composite: 2 u.  The
    longest chain to the output passes L downs, L ups and L combines/composite: (12 + 43 L) u relative to T, first order; the second
    order is below 1e-3 of it for L <= 6."""
    W, H, c, thr = 33, 17, 4.0, 1.0
    film = np.full((3, W * H), c, dtype=F)
    u = 2.0 ** -24
    for levels in pr.BLOOM_LEVELS:
        for spread, intensity in ((1.0, 0.05), (0.5, 0.3)):
            rec = apt._lib.film_bloom_record(1, levels=levels, threshold=thr, spread=spread, intensity=intensity)
            rc, out, intact, _ = pr.bloom_host(apt, rec, film, W, H)
            assert rc == 0 and intact
            l = float(F(0.2126)) * c + float(F(0.7152)) * c + float(F(0.0722)) * c
            v = c * (l - thr) / l
            T = c + float(F(intensity)) * v * sum(float(F(spread)) ** j for j in range(levels))
            err = np.abs(out.astype(D) - T).max()
            assert err <= (12 + 43 * levels) * u * T * 1.001, (levels, err / (u * T))
            assert err < 1e-4 * T and T > c * 1.03


def _support(p, size, levels):
    """The full-resolution indices along one axis that a bright pixel at index p can reach, from the two filters alone -> (lo, hi).
    Down: destination x reads the sources 2x - 1 .. 2x + 2, so a source interval [a, b] reaches x in [ceil((a - 2) / 2), floor((b + 1) / 2)].
    Up: a fine i reads the coarse (i - 1) >> 1 and the one after it, so a coarse interval [a, b] reaches i in [2a - 1, 2b + 2] (a clamped
    read lands on the edge pixel from an i that this interval holds already).  U_j = D_j + spread * up(U_(j+1)) unites the two."""
    sizes = [size]
    for _ in range(levels):
        sizes.append((sizes[-1] + 1) >> 1)
    a = b = p
    reach = []
    for j in range(levels):                                            # D_j
        a, b = max(0, -((2 - a) // 2)), min(sizes[j + 1] - 1, (b + 1) // 2)
        reach.append((a, b))
    lo, hi = reach[-1]
    for j in range(levels - 1, -1, -1):                                # up into level j - 1 (j = 0: the image), united with D_(j-1)
        lo, hi = max(0, 2 * lo - 1), min(sizes[j] - 1, 2 * hi + 2)
        if j:
            lo, hi = min(lo, reach[j - 1][0]), max(hi, reach[j - 1][1])
    return lo, hi


def test_bloom_of_one_bright_pixel_stays_within_its_support(apt):
    W, H = 64, 48
    rng = np.random.default_rng(4)
    for levels, (px, py) in ((1, (31, 20)), (2, (30, 21)), (3, (33, 23)), (6, (31, 20))):
        film = (rng.random((3, W * H)) * 0.5).astype(F)                  # dark: below the threshold
        film[:, px * H + py] = (300.0, 200.0, 100.0)
        rc, out, intact, _ = pr.bloom_host(apt, apt._lib.film_bloom_record(1, levels=levels), film, W, H)
        assert rc == 0 and intact
        (x0, x1), (y0, y1) = _support(px, W, levels), _support(py, H, levels)
        radius = max(px - x0, x1 - px, py - y0, y1 - py)
        X, Y = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
        beyond = (np.maximum(np.abs(X - px), np.abs(Y - py)) > radius).ravel()
        changed = (out.view(np.uint32) != film.view(np.uint32)).any(0)
        assert not changed[beyond].any()
        outside = ~((X >= x0) & (X <= x1) & (Y >= y0) & (Y <= y1)).ravel()
        assert not changed[outside].any()                                # the sharper statement: the rectangle itself
        assert changed.sum() > 1 and changed.reshape(W, H)[px, py]
        if levels < 6:
            assert beyond.any() and radius < 24
        _, B, _ = pr.bloom(pr.BLOOM_DEFAULTS | {"levels": levels}, film, W, H, detail=True)
        assert (B >= 0).all()


def test_three_wrong_implementations_change_the_result():
    """On the restatement: the taps summed in reverse, the border clamped instead of renormalised in `down`, the cap dropped under an inf."""
    W, H = 33, 17
    film = pr.bloom_film(W, H, seed=1)
    rec = dict(pr.BLOOM_DEFAULTS, levels=3)
    right = pr.bloom(rec, film, W, H)
    out = pr.bloom(rec, film, W, H, wrong="reverse_taps")
    assert pr.bits_differ(out, right) and np.abs(out - right).max() < 1e-4 * np.abs(right).max()     # rounding alone
    out = pr.bloom(rec, film, W, H, wrong="clamp")
    d = (out.view(np.uint32) != right.view(np.uint32)).any(0).reshape(W, H)
    assert d.any() and np.abs(out - right).max() > 1e-4                # a border pixel counted more than once
    assert not pr.bits_differ(pr.bloom(rec, film, W, H, wrong="no_cap"), right)       # (no value reaches the cap: the same)
    film[1, 7 * H + 5] = np.inf
    right = pr.bloom(rec, film, W, H)
    out = pr.bloom(rec, film, W, H, wrong="no_cap")
    assert np.isfinite(right[:, np.arange(W * H) != 7 * H + 5]).all() and np.isnan(out).sum() > 3
    assert pr.bits_differ(out, right)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(apt):
    L = apt._lib.post_lib()
    nan, inf = float("nan"), float("inf")
    film = pr.meter_film(65, seed=1)

    def meter(**kw):
        r = apt._lib.film_meter_record(2)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad_meter = [(meter(struct_size=28), APT_ERR_STRUCT), (meter(passes=0), APT_ERR_ARG), (meter(passes=(1 << 24) + 1), APT_ERR_ARG),
                 (meter(low_q=0), APT_ERR_ARG), (meter(low_q=60000), APT_ERR_ARG), (meter(high_q=65537), APT_ERR_ARG),
                 (meter(key=0.0), APT_ERR_ARG), (meter(key=nan), APT_ERR_ARG), (meter(key=inf), APT_ERR_ARG), (meter(min_exposure=0.0), APT_ERR_ARG),
                 (meter(min_exposure=-1.0), APT_ERR_ARG), (meter(max_exposure=inf), APT_ERR_ARG), (meter(max_exposure=nan), APT_ERR_ARG),
                 (meter(min_exposure=8.0, max_exposure=4.0), APT_ERR_ARG), (meter(adapt=-0.1), APT_ERR_ARG), (meter(adapt=1.5), APT_ERR_ARG),
                 (meter(adapt=nan), APT_ERR_ARG)]
    good_hist = pr.meter(film, 2)
    for r, code in bad_meter:
        rc, _, intact, untouched = pr.meter_host(apt, r, film)
        assert rc == code and intact and untouched and L.apt_film_post_last_error() != b""
        rc, e = _exposure_host(apt, r, good_hist)
        assert rc == code and e == F(-7.0)
    for prev in (nan, inf, -inf, -0.5):
        rc, e = _exposure_host(apt, meter(), good_hist, prev)
        assert rc == APT_ERR_ARG and e == F(-7.0) and b"prev" in L.apt_film_post_last_error()
    hist = np.full(pr.WORDS, pr.GARBAGE, dtype=np.uint32)
    good, out = meter(), ctypes.c_float(-7.0)
    for a in ([None, pr.ptr(film), 65, pr.ptr(hist)], [ctypes.byref(good), None, 65, pr.ptr(hist)], [ctypes.byref(good), pr.ptr(film), 65, None],
              [ctypes.byref(good), pr.ptr(film), (1 << 28) + 1, pr.ptr(hist)]):
        assert L.apt_film_meter_host(*a) == APT_ERR_ARG
    assert np.all(hist == pr.GARBAGE)
    for a in ([None, pr.ptr(good_hist), 1.0, ctypes.byref(out)], [ctypes.byref(good), None, 1.0, ctypes.byref(out)],
              [ctypes.byref(good), pr.ptr(good_hist), 1.0, None]):
        assert L.apt_film_exposure_host(*a) == APT_ERR_ARG
    assert out.value == -7.0
    assert L.apt_film_meter_host(ctypes.byref(good), pr.ptr(film), 65, pr.ptr(hist)) == 0 and L.apt_film_post_last_error() == b""
    assert np.array_equal(hist, good_hist)

    W, H = 5, 3
    N = W * H
    bfilm = pr.bloom_film(W, H)

    def bloom(**kw):
        r = apt._lib.film_bloom_record(2, levels=2)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad_bloom = [(bloom(struct_size=28), APT_ERR_STRUCT), (bloom(passes=0), APT_ERR_ARG), (bloom(passes=(1 << 24) + 1), APT_ERR_ARG),
                 (bloom(levels=0), APT_ERR_ARG), (bloom(levels=7), APT_ERR_ARG), (bloom(threshold=-1.0), APT_ERR_ARG), (bloom(threshold=nan), APT_ERR_ARG),
                 (bloom(threshold=inf), APT_ERR_ARG), (bloom(cap=0.0), APT_ERR_ARG), (bloom(cap=inf), APT_ERR_ARG), (bloom(cap=nan), APT_ERR_ARG),
                 (bloom(spread=-0.5), APT_ERR_ARG), (bloom(spread=nan), APT_ERR_ARG), (bloom(intensity=-1.0), APT_ERR_ARG),
                 (bloom(intensity=inf), APT_ERR_ARG)]
    for r, code in bad_bloom:
        rc, _, intact, untouched = pr.bloom_host(apt, r, bfilm, W, H)
        assert rc == code and intact and untouched and L.apt_film_post_last_error() != b"", (code, rc)
    good = bloom()
    floats = L.apt_film_bloom_work_floats(W, H, 2)
    wb, work = pr._guarded(floats, F, np.nan)
    ob, out = pr._guarded(3 * N, F, np.nan)
    args = [ctypes.byref(good), pr.ptr(bfilm), W, H, pr.ptr(work), pr.ptr(out)]
    for i in (0, 1, 4, 5):
        a = list(args)
        a[i] = None
        assert L.apt_film_bloom_host(*a) == APT_ERR_ARG, i
    for i, v in ((2, 0), (3, 0)):
        a = list(args)
        a[i] = v
        assert L.apt_film_bloom_host(*a) == APT_ERR_ARG
    a = list(args)
    a[2], a[3] = 1 << 15, (1 << 13) + 1                                # N > 2^28
    assert L.apt_film_bloom_host(*a) == APT_ERR_ARG
    a = list(args)
    a[4] = pr.ptr(work) + 4                                            # a misaligned work
    assert L.apt_film_bloom_host(*a) == APT_ERR_ARG and b"aligned" in L.apt_film_post_last_error()
    a = list(args)
    a[5] = a[1]                                                        # out == film
    before = bfilm.copy()
    assert L.apt_film_bloom_host(*a) == APT_ERR_ARG and not pr.bits_differ(bfilm, before)
    assert np.isnan(out).all() and np.isnan(work).all() and pr._intact(wb, floats) and pr._intact(ob, 3 * N)
    assert L.apt_film_bloom_host(*args) == 0 and L.apt_film_post_last_error() == b"" and not np.isnan(out).any()
    pr.assert_same(out.reshape(3, N), pr.bloom(good, bfilm, W, H))
