"""CPU-only: film comparison metrics (libmetrics_mi355x.so, include/render_mi355x_metrics.h) -- the binding against the header and the
exports, the CPU twins of compare and SSIM bit for bit against the restatement tests/metrics_ref.py, what the results MEAN (bad pixels,
the tie of the maximum, a film against itself, the scaling law, identical and constant images), every refusal, and, on the restatement,
that three wrong implementations are told from the right one.

Every test that does not choose its bad pixels asserts bad == 0: no case hides behind the exclusion.

Without the feature nothing here passes: the library, the header, the binding and the restatement do not exist."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import materials_ref as mr
import metrics_ref as xr

F, D = np.float32, np.float64
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
NAMES = ["apt_film_compare_default_host", "apt_film_compare_work_doubles", "apt_film_compare_device", "apt_film_compare_host",
         "apt_film_ssim_weights_host", "apt_film_ssim_work_bytes", "apt_film_ssim_device", "apt_film_ssim_host",
         "apt_film_metrics_last_error"]


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


def test_symbols_record_and_defaults(apt):
    """A sixth library with a header of its own: the binding's table is that header's, entry by entry and in its order, the library
    exports those names and nothing else, and the other five libraries export exactly their tables and know none of the new names."""
    from ascendpathtracing_amd._lib import ApFilmCompare
    L = apt._lib.metrics_lib()
    assert ctypes.sizeof(ApFilmCompare) == 24 and ApFilmCompare.exposure.offset == 16 and ApFilmCompare.eps.offset == 20
    header = _header_prototypes("render_mi355x_metrics.h")
    assert list(header) == NAMES
    table = apt._lib.METRICS_PROTOTYPES
    assert list(table) == list(header)
    for name, proto in header.items():
        assert (table[name][0], list(table[name][1])) == proto, name
        fn = getattr(L, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == list(table[name][1]), name
    assert _exports(apt._lib.METRICS_LIB_PATH) == set(header)
    new = set(header) | {"apt_film_compare"}
    others = (set(apt._lib.ABI_SYMBOLS) | set(apt._lib.DENOISE_PROTOTYPES) | set(apt._lib.ADAPTIVE_PROTOTYPES)
              | set(apt._lib.HISTORY_PROTOTYPES) | set(apt._lib.POST_PROTOTYPES))
    assert not new & others
    assert _exports(apt._lib.LIB_PATH) == set(apt._lib.PROTOTYPES)
    assert _exports(apt._lib.DENOISE_LIB_PATH) == set(apt._lib.DENOISE_PROTOTYPES)
    assert _exports(apt._lib.ADAPTIVE_LIB_PATH) == set(apt._lib.ADAPTIVE_PROTOTYPES)
    assert _exports(apt._lib.HISTORY_LIB_PATH) == set(apt._lib.HISTORY_PROTOTYPES)
    assert _exports(apt._lib.POST_LIB_PATH) == set(apt._lib.POST_PROTOTYPES)
    for h in ("render_mi355x.h", "render_mi355x_denoise.h", "render_mi355x_adaptive.h", "render_mi355x_history.h", "render_mi355x_post.h"):
        assert not re.search(r"\b(%s)\b" % "|".join(sorted(new)), open(os.path.join(mr.ROOT, "include", h)).read()), h
    assert apt._lib.lib().apt_abi_version() == 3
    assert (apt._lib.APT_COMPARE_WORDS, apt._lib.APT_SSIM_WORDS, apt._lib.APT_SSIM_TAPS) == (xr.COMPARE_WORDS, xr.SSIM_WORDS, xr.TAPS) == (8, 2, 11)

    c = apt._lib.film_compare_record(7, 3)
    assert (c.struct_size, c.passes_a, c.passes_b, c.reserved) == (24, 7, 3, 0)
    assert (c.exposure, c.eps) == (F(1), F(1e-2)) == tuple(F(xr.DEFAULTS[k]) for k in ("exposure", "eps"))
    fn = L.apt_film_compare_default_host
    assert fn(None, 1, 1) == APT_ERR_ARG and b"null" in L.apt_film_metrics_last_error()
    for pa, pb in ((0, 1), (1, 0), ((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
        assert fn(ctypes.byref(c), pa, pb) == APT_ERR_ARG
    assert fn(ctypes.byref(c), 1 << 24, 1 << 24) == 0 and L.apt_film_metrics_last_error() == b"" and c.passes_b == 1 << 24
    assert apt._lib.film_compare_record(2, exposure=0.5).exposure == F(0.5) and apt._lib.film_compare_record(2).passes_b == 1
    with pytest.raises(apt.AptError):
        apt._lib.film_compare_record(2, 2, key=1.0)
    for name in ("film_compare", "film_ssim", "compare_summary"):
        assert hasattr(apt.render, name)
    assert hasattr(apt.render.Film, "compare")
    # (build_id() hashes public_headers(): tests/test_film_stage_cpu.py holds it to the hand-written list)
    assert os.path.join(mr.ROOT, "include", "render_mi355x_metrics.h") in apt._lib.public_headers()
    # the work sizes, functions of the size alone: a row of 6 words per 1024 pixels, and a row per 4096 of those beyond 4096
    Wd = L.apt_film_compare_work_doubles
    assert [Wd(n) for n in (0, 1, 1024, 1025, 1 << 22, (1 << 22) + 1, 1 << 28, (1 << 28) + 1)] == [
        0, 6, 6, 12, 6 * 4096, 6 * (4097 + 2), 6 * ((1 << 18) + 64), 0]
    Wb = L.apt_film_ssim_work_bytes
    assert Wb(11, 11) == 16 + 16 and Wb(75, 70) == 8 * 4 + 4 * 65 * 60 and Wb(1920, 1080) == 8 * 1996 + 4 * 1910 * 1070
    assert Wb(10, 11) == 0 and Wb(11, 10) == 0 and Wb(1 << 14, (1 << 14) + 1) == 0


def test_the_weights_are_the_restatements(apt):
    w = np.full(13, -7.0, dtype=F)
    assert apt._lib.metrics_lib().apt_film_ssim_weights_host(w[1:].ctypes.data) == 0
    assert w[0] == -7.0 and w[12] == -7.0
    want = xr.weights()
    assert np.array_equal(w[1:12].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, want[::-1]) and abs(float(want.astype(D).sum()) - 1.0) < 1e-7 and want.argmax() == 5
    assert apt._lib.metrics_lib().apt_film_ssim_weights_host(None) == APT_ERR_ARG


# ---- compare's twin against the restatement ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", xr.COMPARE_SIZES)
def test_compare_twin_equals_the_restatement(apt, n):
    """Channels spanning 2^-20 .. 2^20.  From 64 pixels on the pin is first shown to be sensitive to the order: a left-to-right float64
    sum of the same terms has other bits than the tree in at least one of the four sums.  (Up to 3 terms the two orders are the same
    expression; a few dozen terms of 24 significant bits mostly still add exactly in 53, whatever the order: nothing can be asked
    there.)"""
    for k, (pa, pb) in enumerate(xr.COMPARE_PASSES):
        a, b = xr.compare_films(n, seed=10 * n + k)
        want, want_map = xr.compare(a, b, pa, pb)
        if n >= 64:
            assert (xr.compare(a, b, pa, pb, wrong="sequential")[0][:4] != want[:4]).any()
        rc, got, got_map, guards, _ = xr.compare_host(apt, xr.record(apt, pa, pb), a, b)
        assert rc == 0 and guards
        assert np.array_equal(got, want), (n, pa, pb, got, want)
        assert got[5] == 0 and got[6] == n and got[7] == 0
        xr.assert_same(got_map, want_map)
        rc, got2, _, guards, _ = xr.compare_host(apt, xr.record(apt, pa, pb), a, b, want_map=False)        # err_map NULL
        assert rc == 0 and guards and np.array_equal(got2, want)
    a, b = xr.display_films(n, seed=n)                                   # around the display range, another exposure and eps
    rec = xr.record(apt, 2, 5, exposure=0.75, eps=1e-3)
    rc, got, got_map, guards, _ = xr.compare_host(apt, rec, a, b)
    want, want_map = xr.compare(a, b, 2, 5, 0.75, 1e-3)
    assert rc == 0 and guards and np.array_equal(got, want) and got[5] == 0
    xr.assert_same(got_map, want_map)
    s = xr.summary(got)
    assert 0 <= s["clipped_mse"] <= 1 and s["clipped_mse"] <= s["mse"] * 0.75 ** 2 * 1.0001 and s["ssim"] is None


BAD_VALUES = [np.nan, np.inf, -np.inf, 2.0 ** 60]


def test_bad_pixels(apt):
    """The test chooses them: NaN, +inf, -inf and exactly 2^60 in each of the six positions (24 bad pixels), the predecessor of 2^60
    in each (6 good ones).  An all-bad image: sums of +0, a key of 0, bad = n."""
    n = 101
    a, b = xr.display_films(n, seed=4)
    chosen = []
    at = 3
    for film in (a, b):
        for ch in range(3):
            for v in BAD_VALUES:
                film[ch, at] = v
                chosen.append(at)
                at += 1
            film[ch, at] = np.nextafter(F(2.0 ** 60), F(0))               # the largest good value
            at += 1
    assert at == 33 and len(set(chosen)) == 24
    rc, got, got_map, guards, _ = xr.compare_host(apt, xr.record(apt), a, b)
    want, want_map = xr.compare(a, b)
    assert rc == 0 and guards and np.array_equal(got, want)
    assert got[5] == 24 and got[6] == n
    xr.assert_same(got_map, want_map)
    assert not got_map[chosen].any() and np.isfinite(got_map).all()
    assert np.isfinite(got[:4].view(D)).all()
    # the largest difference is one of the 2^60-predecessor pixels, never a bad one
    s = xr.summary(got)
    assert s["bad"] == 24 and s["max_index"] not in chosen and s["max_abs"] >= 2.0 ** 59
    # with passes = 2 the value 2^61 is the first bad one
    a2, b2 = xr.display_films(7, seed=5)
    a2[1, 2] = 2.0 ** 61
    a2[1, 3] = np.nextafter(F(2.0 ** 61), F(0))
    rc, got, _, _, _ = xr.compare_host(apt, xr.record(apt, 2, 1), a2, b2)
    assert rc == 0 and got[5] == 1 and np.array_equal(got, xr.compare(a2, b2, 2, 1)[0])
    # all bad
    for n in (1, 5, 1025):
        a, b = xr.display_films(n, seed=6)
        a[n % 3, :] = np.nan
        rc, got, got_map, guards, _ = xr.compare_host(apt, xr.record(apt), a, b)
        assert rc == 0 and guards and list(got) == [0, 0, 0, 0, 0, n, n, 0] and not got_map.view(np.uint32).any()
        assert np.array_equal(got, xr.compare(a, b)[0])
        s = xr.summary(got)
        assert s["bad"] == n and s["max_index"] == -1 and all(np.isnan(s[k]) for k in ("mse", "clipped_mse", "rel_mse", "mae", "psnr", "max_abs"))


def test_compare_meaning(apt):
    # a tie of the maximum at two indices reports the lower one
    n = 300
    a, b = xr.display_films(n, seed=7)
    b[1, 211], b[2, 77] = 0.5, 0.25                                     # so that the two differences are exactly 8
    a[:, :] = b
    a[1, 211] = b[1, 211] + F(8.0)
    a[2, 77] = b[2, 77] - F(8.0)
    d211, d77 = abs(F(a[1, 211] - b[1, 211])), abs(F(a[2, 77] - b[2, 77]))
    assert d211 == d77 == F(8.0)
    rc, got, _, _, _ = xr.compare_host(apt, xr.record(apt), a, b)
    s = xr.summary(got)
    assert rc == 0 and got[5] == 0 and s["max_index"] == 77 and s["max_abs"] == 8.0
    assert np.array_equal(got, xr.compare(a, b)[0])
    # a film against itself (the same pointer): four zero sums, the key of difference 0 at pixel 0
    for n in (1, 64, 1001):
        a, _ = xr.compare_films(n, seed=8)
        rc, got, got_map, guards, _ = xr.compare_host(apt, xr.record(apt, 3, 3), a, a)
        assert rc == 0 and guards and list(got) == [0, 0, 0, 0, 0xFFFFFFFF, 0, n, 0] and not got_map.view(np.uint32).any()
    # the scaling law: both films times 2^k -> the sum of the squared error times exactly 4^k (and the absolute error times 2^k)
    a, b = xr.compare_films(777, seed=9)
    base = xr.compare_host(apt, xr.record(apt), a, b)[1]
    assert base[5] == 0
    for k in (3, -2, 10):
        got = xr.compare_host(apt, xr.record(apt), a * F(2.0 ** k), b * F(2.0 ** k))[1]
        assert got[5] == 0
        assert got[0:1].view(D)[0] == base[0:1].view(D)[0] * 4.0 ** k and got[3:4].view(D)[0] == base[3:4].view(D)[0] * 2.0 ** k
        assert int(got[4]) >> 32 == (int(base[4]) >> 32) + (k << 23)     # the largest difference: its exponent moved
        assert int(got[4]) & 0xFFFFFFFF == int(base[4]) & 0xFFFFFFFF
    # passes: a film of sums over K frames against the same means
    a, b = xr.display_films(500, seed=10)
    one = xr.compare_host(apt, xr.record(apt), a, b)[1]
    assert np.array_equal(xr.compare_host(apt, xr.record(apt, 4, 8), a * F(4), b * F(8))[1], one)
    # tiny values: where K is a power of two the library may multiply by 2^-m instead of dividing; the quotients -- subnormal ones
    # too -- are the restatement's divisions bit for bit
    a, b = xr.tiny_films(257)
    for pa, pb in xr.TINY_PASSES:
        rc, got, got_map, _, _ = xr.compare_host(apt, xr.record(apt, pa, pb), a, b)
        want, want_map = xr.compare(a, b, pa, pb)
        assert rc == 0 and got[5] == 0 and np.array_equal(got, want), (pa, pb)
        xr.assert_same(got_map, want_map)
    m = a / F(1 << 24)
    assert (m < 2.0 ** -126).all() and (m > 0).any() and (xr.compare_terms(a, b, 1 << 24, 4)[3] > 0).any()    # subnormal means, errors above 0


# ---- SSIM's twin against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", xr.SSIM_SIZES, ids=lambda s: "%dx%d" % s)
def test_ssim_twin_equals_the_restatement(apt, shape):
    W, H = shape
    for k, (pa, pb, ex) in enumerate(((1, 1, 1.0), (3, 64, 0.8), (1 << 24, 1, 1.7))):
        a, b = xr.ssim_films(W, H, seed=k)
        a, b = a * F(pa), b * F(pb)
        rc, got, got_map, guards, _ = xr.ssim_host(apt, xr.record(apt, pa, pb, exposure=ex), a, b, W, H)
        want, want_map = xr.ssim(a, b, W, H, pa, pb, ex)
        assert rc == 0 and guards
        assert np.array_equal(got, want), (shape, got, want)
        assert got[1] == (W - 10) * (H - 10)
        xr.assert_same(got_map, want_map)
        assert np.isfinite(got_map).all() and got_map.max() <= 1.0 and got_map.min() > -1.0
        rc, got2, _, guards, _ = xr.ssim_host(apt, xr.record(apt, pa, pb, exposure=ex), a, b, W, H, want_map=False)
        assert rc == 0 and guards and np.array_equal(got2, want)
        # SSIM reads the films as compare does: no bad pixel hides in them
        assert xr.compare_host(apt, xr.record(apt, pa, pb, exposure=ex), a, b)[1][5] == 0


def _closed_form(A, B):
    """A window of two CONSTANT luminance planes A and B, in scalar float32: a plane of the constant c filters to g(g(c)), g one pass."""
    w = xr.weights()

    def g(c):
        acc = F(0)
        for k in range(xr.TAPS):
            acc = F(acc + F(w[k] * c))
        return acc

    A, B = F(A), F(B)
    ma, mb, eaa, ebb, eab = (g(g(c)) for c in (A, B, F(A * A), F(B * B), F(A * B)))
    maa, mbb, mab = F(ma * ma), F(mb * mb), F(ma * mb)
    saa, sbb, sab = F(eaa - maa), F(ebb - mbb), F(eab - mab)
    num = F(F(F(F(2) * mab) + xr.C1) * F(F(F(2) * sab) + xr.C2))
    den = F(F(F(maa + mbb) + xr.C1) * F(F(saa + sbb) + xr.C2))
    return F(num / den)


def test_ssim_meaning(apt):
    """Identical images give s == 1.0f EXACTLY in every window.  Why: with Ya == Yb the five planes collapse to m = ma = mb and
    E = Eaa = Ebb = Eab, so maa = mbb = mab = m * m and saa = sbb = sab.  The numerator holds 2 * (m * m), the denominator m * m + m * m:
    doubling a binary float and adding it to itself are both the exact value 2 (m * m) (only the exponent moves; nothing here is near
    overflow), hence the same float; likewise 2 * sab and saa + sbb.  Numerator and denominator are then the same operations on the same
    floats, the same finite positive number (at least C1 * (C2 - rounding)), and x / x is exactly 1."""
    W, H = 43, 27
    a, _ = xr.ssim_films(W, H, seed=3)
    for pa, pb in ((1, 1), (4, 4)):
        rc, got, got_map, _, _ = xr.ssim_host(apt, xr.record(apt, pa, pb), a, a.copy(), W, H)
        assert rc == 0 and np.all(got_map.view(np.uint32) == F(1).view(np.uint32))
        assert got[0:1].view(D)[0] == float((W - 10) * (H - 10)) and xr.summary(np.zeros(8, np.uint64), got)["ssim"] == 1.0
    # the same film through the same pointer
    rc, got, got_map, _, _ = xr.ssim_host(apt, xr.record(apt), a, a, W, H)
    assert rc == 0 and np.all(got_map == F(1))
    # a constant image against another constant: the closed form, in every window
    N = W * H
    for va, vb in ((0.25, 0.75), (0.6, 0.6), (0.0, 1.0), (2.5, 0.4)):
        a = np.full((3, N), va, dtype=F)
        b = np.full((3, N), vb, dtype=F)
        A, B = (xr.lum(*([xr.clip01(np.array([v], dtype=F))] * 3))[0] for v in (va, vb))
        want = _closed_form(A, B)
        rc, got, got_map, _, _ = xr.ssim_host(apt, xr.record(apt), a, b, W, H)
        assert rc == 0 and np.all(got_map.view(np.uint32) == want.view(np.uint32)), (va, vb, got_map[0], want)
        assert abs(float(want) - (2 * A * B + 1e-4) / (A * A + B * B + 1e-4)) < 2e-3          # the luminance term alone is left
    # exposure: it scales what is clipped
    a, b = xr.ssim_films(W, H, seed=4)
    lo = xr.ssim_host(apt, xr.record(apt, exposure=0.5), a, b, W, H)[1]
    assert np.array_equal(lo, xr.ssim(a, b, W, H, exposure=0.5)[0]) and not np.array_equal(lo, xr.ssim(a, b, W, H)[0])


def test_wrong_implementations_are_told(apt):
    """A sequential sum, the taps in reverse order and border-clamped windows each change the bits on the test's input."""
    W, H = 43, 27
    a, b = xr.ssim_films(W, H, seed=5)
    rc, got, got_map, _, _ = xr.ssim_host(apt, xr.record(apt), a, b, W, H)
    right, right_map = xr.ssim(a, b, W, H)
    assert rc == 0 and np.array_equal(got, right)
    # (a sequential sum of THESE terms would not show: a few hundred s of 24 bits within a few binades add exactly in float64 in any
    # order.  The sum's order is told on compare's input, below.)
    rev, rev_map = xr.ssim(a, b, W, H, wrong="reverse")
    assert rev[0] != right[0] and (rev_map.view(np.uint32) != right_map.view(np.uint32)).any()
    assert np.abs(rev_map - right_map).max() < 1e-4                       # the same filter, another rounding
    cl, cl_map = xr.ssim(a, b, W, H, wrong="clamp")
    assert cl[1] == W * H != right[1] and cl[0] != right[0]
    inner = cl_map.reshape(W, H)[5:W - 5, 5:H - 5]                        # away from the border the clamped windows ARE the valid ones
    assert np.array_equal(np.ascontiguousarray(inner).ravel().view(np.uint32), right_map.view(np.uint32))
    assert float(cl[0:1].view(D)[0]) / W / H != float(right[0:1].view(D)[0]) / int(right[1])
    # and for compare: the sequential sum (the other two have no counterpart there)
    a, b = xr.compare_films(4097, seed=11)
    got = xr.compare_host(apt, xr.record(apt), a, b)[1]
    assert np.array_equal(got, xr.compare(a, b)[0]) and (xr.compare(a, b, wrong="sequential")[0][:4] != got[:4]).any()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(apt):
    L = apt._lib.metrics_lib()
    nan, inf = float("nan"), float("inf")
    n = 65
    a, b = xr.display_films(n, seed=12)
    good = lambda **kw: xr.record(apt, 2, 3, **kw)

    def compare(rec, fa=a, fb=b, count=n, res=True, alias=None):
        rb, r = xr.guarded(xr.COMPARE_WORDS, np.uint64, xr.GARBAGE64)
        mb, m = xr.guarded(n, F, np.nan)
        r_ptr = {None: xr.ptr(r), "result=a": xr.ptr(fa), "result=b": xr.ptr(fb)}.get(alias, xr.ptr(r)) if res else None
        m_ptr = {"map=a": xr.ptr(fa), "map=b": xr.ptr(fb), "map=result": xr.ptr(r)}.get(alias, xr.ptr(m))
        before = (fa.copy(), fb.copy()) if fa is not None and fb is not None else None
        rc = L.apt_film_compare_host(None if rec is None else ctypes.byref(rec), xr.ptr(fa), xr.ptr(fb), count, r_ptr, m_ptr)
        assert rc != 0 and L.apt_film_metrics_last_error() != b""
        assert xr.intact(rb, xr.COMPARE_WORDS) and xr.intact(mb, n) and np.all(r == xr.GARBAGE64) and np.isnan(m).all()
        if before is not None:
            assert np.array_equal(before[0], fa) and np.array_equal(before[1], fb)
        return rc

    assert compare(None) == APT_ERR_ARG and compare(good(), fa=None) == APT_ERR_ARG and compare(good(), fb=None) == APT_ERR_ARG
    assert compare(good(), res=False) == APT_ERR_ARG
    assert compare(good(), count=0) == APT_ERR_ARG and compare(good(), count=(1 << 28) + 1) == APT_ERR_ARG
    for kw in (dict(exposure=0.0), dict(exposure=-1.0), dict(exposure=nan), dict(exposure=inf), dict(eps=0.0), dict(eps=-1e-2), dict(eps=nan),
               dict(eps=inf)):
        assert compare(good(**kw)) == APT_ERR_ARG, kw
    for field, v in (("passes_a", 0), ("passes_b", 0), ("passes_a", (1 << 24) + 1), ("passes_b", (1 << 24) + 1)):
        rec = good()
        setattr(rec, field, v)
        assert compare(rec) == APT_ERR_ARG
    for size in (20, 28):
        rec = good()
        rec.struct_size = size
        assert compare(rec) == APT_ERR_STRUCT
    for alias in ("result=a", "result=b", "map=a", "map=b", "map=result"):
        assert compare(good(), alias=alias) == APT_ERR_ARG, alias
    assert L.apt_film_compare_host(ctypes.byref(good()), xr.ptr(a), xr.ptr(a), n, xr.ptr(np.zeros(8, np.uint64)), None) == 0   # a == b is allowed
    assert L.apt_film_metrics_last_error() == b""

    W, H = 12, 11
    sa, sb = xr.ssim_films(W, H)

    def ssim(rec, fa=sa, fb=sb, w=W, h=H, res=True, alias=None):
        rb, r = xr.guarded(xr.SSIM_WORDS, np.uint64, xr.GARBAGE64)
        mb, m = xr.guarded(4, F, np.nan)
        r_ptr = {"result=a": xr.ptr(fa), "result=b": xr.ptr(fb)}.get(alias, xr.ptr(r)) if res else None
        m_ptr = {"map=a": xr.ptr(fa), "map=b": xr.ptr(fb), "map=result": xr.ptr(r)}.get(alias, xr.ptr(m))
        rc = L.apt_film_ssim_host(None if rec is None else ctypes.byref(rec), xr.ptr(fa), xr.ptr(fb), w, h, r_ptr, m_ptr)
        assert rc != 0 and L.apt_film_metrics_last_error() != b""
        assert xr.intact(rb, xr.SSIM_WORDS) and xr.intact(mb, 4) and np.all(r == xr.GARBAGE64) and np.isnan(m).all()
        return rc

    assert ssim(None) == APT_ERR_ARG and ssim(good(), fa=None) == APT_ERR_ARG and ssim(good(), fb=None) == APT_ERR_ARG
    assert ssim(good(), res=False) == APT_ERR_ARG
    for w, h in ((10, 11), (11, 10), (0, 11), (11, 0), (1 << 14, (1 << 14) + 1)):
        assert ssim(good(), w=w, h=h) == APT_ERR_ARG, (w, h)
    for kw in (dict(exposure=0.0), dict(exposure=nan), dict(eps=0.0), dict(eps=inf)):
        assert ssim(good(**kw)) == APT_ERR_ARG, kw
    rec = good()
    rec.passes_b = 0
    assert ssim(rec) == APT_ERR_ARG
    rec = good()
    rec.struct_size = 32
    assert ssim(rec) == APT_ERR_STRUCT
    for alias in ("result=a", "result=b", "map=a", "map=b", "map=result"):
        assert ssim(good(), alias=alias) == APT_ERR_ARG, alias
    assert np.array_equal(sa, xr.ssim_films(W, H)[0]) and np.array_equal(sb, xr.ssim_films(W, H)[1])
