"""include/render_mi355x_metrics.h restated in NumPy: the compare terms and the SSIM windows, every fp32 step one float32 ufunc in the
header's order (NumPy rounds each operation on its own and fuses nothing), and THE SUM: pad to a power of two with +0.0, then repeated
reshape(-1, 2) pair adds in float64.  tests/test_metrics_cpu.py holds libmetrics_mi355x.so's CPU twins to it bit for bit,
tests/test_gpu_metrics.py the device entries to the twins.  Also what those two files share: the films, the summary of the result
words, and the calls of the host entries into garbage-filled outputs inside guard words.

`wrong=` builds three WRONG implementations (a left-to-right sum, the taps in reverse order, border-clamped windows) that the CPU test
must tell from the right one."""
import ctypes
import math

import numpy as np

F, D = np.float32, np.float64
COMPARE_WORDS, SSIM_WORDS, TAPS = 8, 2, 11
DEFAULTS = dict(exposure=1.0, eps=1e-2)
C1, C2 = F(1e-4), F(9e-4)
COMPARE_SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
COMPARE_PASSES = [(1, 1), (3, 64), (1 << 24, 1)]
SSIM_SIZES = [(11, 11), (11, 12), (12, 11), (16, 16), (43, 27), (75, 70)]      # (W, H)
CHUNK, FOLD_ROWS = 1024, 4096                                                   # metrics_ops.h: pixels a workgroup, rows a fold workgroup
TILE_X, TILE_Y = 16, 64                                                         # metrics.hip: windows a workgroup of the SSIM kernel
GUARD = 16
GARBAGE64 = 0xDEADBEEFCAFEF00D


# ---- the sum -------------------------------------------------------------------------------------------------------------------------------
def tree_sum(terms):
    """float32 terms [n], n >= 1 -> the float64 T(0, L) of the header."""
    t = np.ascontiguousarray(terms, dtype=F).astype(D)
    size = 1
    while size < t.size:
        size *= 2
    v = np.zeros(size, dtype=D)                                                 # +0.0
    v[:t.size] = t
    while v.size > 1:
        p = v.reshape(-1, 2)
        v = p[:, 0] + p[:, 1]
    return v[0]


def sequential_sum(terms):
    """WRONG on purpose: the same terms, left to right."""
    return np.add.accumulate(np.ascontiguousarray(terms, dtype=F).astype(D))[-1]


def bits64(x):
    return int(np.array([x], dtype=D).view(np.uint64)[0])


# ---- the arithmetic ------------------------------------------------------------------------------------------------------------------------
def lum(r, g, b):
    l = F(0.2126) * r
    l = l + F(0.7152) * g
    return l + F(0.0722) * b


def fmax(a, b):
    return np.where(a > b, a, b)


def clip01(e):
    t = np.where(e > 0, e, F(0))
    return np.where(t < 1, t, F(1)).astype(F)


def is_bad(v):
    return ((np.ascontiguousarray(v, dtype=F).view(np.uint32) >> 23) & 255) >= 187


def compare_terms(a, b, passes_a=1, passes_b=1, exposure=1.0, eps=1e-2):
    """a, b [3][n] -> (se, cse, rse, ae, ad float32 [n], bad bool [n]); the terms of a bad pixel are +0."""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    with np.errstate(all="ignore"):
        x, y = a / F(passes_a), b / F(passes_b)
        bad = is_bad(x).any(axis=0) | is_bad(y).any(axis=0)
        d = x - y
        dd = d * d
        ad3 = np.abs(d)
        se = (dd[0] + dd[1]) + dd[2]
        ae = (ad3[0] + ad3[1]) + ad3[2]
        r = dd / (y * y + F(eps))
        rse = (r[0] + r[1]) + r[2]
        c = clip01(x * F(exposure)) - clip01(y * F(exposure))
        cc = c * c
        cse = (cc[0] + cc[1]) + cc[2]
        ad = fmax(fmax(ad3[0], ad3[1]), ad3[2])
    zero = F(0)
    out = [np.where(bad, zero, v).astype(F) for v in (se, cse, rse, ae, ad)]
    return (*out, bad)


def compare(a, b, passes_a=1, passes_b=1, exposure=1.0, eps=1e-2, wrong=None):
    """-> (result uint64 [8], err_map float32 [n])."""
    se, cse, rse, ae, ad, bad = compare_terms(a, b, passes_a, passes_b, exposure, eps)
    n = se.size
    total = sequential_sum if wrong == "sequential" else tree_sum
    res = np.zeros(COMPARE_WORDS, dtype=np.uint64)
    for k, t in enumerate((se, cse, rse, ae)):
        res[k] = bits64(total(t))
    key = (np.ascontiguousarray(ad, dtype=F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (
        np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))
    good = ~bad
    res[4] = key[good].max() if good.any() else 0
    res[5] = int(bad.sum())
    res[6] = n
    return res, se


def weights():
    """exp(-(k - 5)^2 / 4.5) normalised in float64, rounded once."""
    k = np.arange(TAPS, dtype=D)
    g = np.exp(-(k - 5.0) ** 2 / 4.5)
    return (g / g.sum()).astype(F)


def display_lum(film, passes, exposure, W, H):
    film = np.ascontiguousarray(film, dtype=F)
    with np.errstate(all="ignore"):
        m = film / F(passes)
        c = clip01(m * F(exposure))
        return np.ascontiguousarray(lum(c[0], c[1], c[2]), dtype=F).reshape(W, H)


def _filter(P, w, order, axis):
    n = P.shape[axis] - 10
    acc = np.zeros(P.shape[:axis] + (n,) + P.shape[axis + 1:], dtype=F)
    for k in order:
        sl = [slice(None)] * P.ndim
        sl[axis] = slice(k, k + n)
        acc = acc + w[k] * P[tuple(sl)]
    return acc


def ssim(a, b, W, H, passes_a=1, passes_b=1, exposure=1.0, wrong=None):
    """-> (result uint64 [2], map float32 [(W - 10) * (H - 10)])  (wrong="clamp": one window per PIXEL, the images edge-replicated)."""
    ya, yb = display_lum(a, passes_a, exposure, W, H), display_lum(b, passes_b, exposure, W, H)
    if wrong == "clamp":
        ya, yb = np.pad(ya, 5, mode="edge"), np.pad(yb, 5, mode="edge")
    w = weights()
    order = range(TAPS - 1, -1, -1) if wrong == "reverse" else range(TAPS)
    with np.errstate(all="ignore"):
        planes = (ya, yb, ya * ya, yb * yb, ya * yb)
        ma, mb, eaa, ebb, eab = (_filter(_filter(p, w, order, 0), w, order, 1) for p in planes)
        maa, mbb, mab = ma * ma, mb * mb, ma * mb
        saa, sbb, sab = eaa - maa, ebb - mbb, eab - mab
        s = ((F(2) * mab + C1) * (F(2) * sab + C2)) / (((maa + mbb) + C1) * ((saa + sbb) + C2))
    s = np.ascontiguousarray(s, dtype=F).ravel()
    total = sequential_sum if wrong == "sequential" else tree_sum
    return np.array([bits64(total(s)), s.size], dtype=np.uint64), s


def summary(result, ssim_result=None):
    """The restatement of render.compare_summary: the result words as numbers."""
    r = np.ascontiguousarray(result).view(np.uint64)
    sums = r[:4].view(D)
    key, bad, n = int(r[4]), int(r[5]), int(r[6])
    good = n - bad
    mean = [float(s) / (3 * good) if good else float("nan") for s in sums]
    out = dict(mse=mean[0], clipped_mse=mean[1], rel_mse=mean[2], mae=mean[3])
    out["psnr"] = (10.0 * math.log10(1.0 / mean[1]) if mean[1] > 0 else float("inf")) if good else float("nan")
    out["max_abs"] = float(np.array([key >> 32], dtype=np.uint32).view(F)[0]) if good else float("nan")
    out["max_index"] = 0xFFFFFFFF - (key & 0xFFFFFFFF) if good else -1
    out["bad"] = bad
    out["ssim"] = None
    if ssim_result is not None:
        s = np.ascontiguousarray(ssim_result).view(np.uint64)
        out["ssim"] = float(s[:1].view(D)[0]) / int(s[1])
    return out


# ---- the films -----------------------------------------------------------------------------------------------------------------------------
def compare_films(n, seed=0):
    """a, b [3][n]: every channel log-uniform over 2^-20 .. 2^20 on its own, b within a factor of two of a.  No bad pixel."""
    rng = np.random.default_rng(1000 + seed)
    a = np.exp2(rng.uniform(-20, 20, (3, n))).astype(F)
    b = (a * rng.uniform(0.5, 2.0, (3, n)).astype(F)).astype(F)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def display_films(n, seed=0):
    """a, b [3][n] around the display range: a reference in [0, 1.5) and a noisy copy of it."""
    rng = np.random.default_rng(2000 + seed)
    b = (rng.random((3, n)) * 1.5).astype(F)
    a = (b + rng.normal(0, 0.2, (3, n)).astype(F)).astype(F)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


TINY_PASSES = [(1 << 24, 4), (2, 1 << 10), (3, 1 << 24), (1, 1)]


def tiny_films(n, seed=0):
    """compare_films scaled by 2^-125: 2^-145 .. 2^-105, subnormal and tiny normal values whose means over 2^24 passes are all subnormal."""
    a, b = compare_films(n, seed=4000 + seed)
    return np.ascontiguousarray(a * F(2.0 ** -125)), np.ascontiguousarray(b * F(2.0 ** -125))


def ssim_films(W, H, seed=0):
    """A smooth image plus texture, and a noisy, slightly darker copy: windows from near 1 down to well below it."""
    rng = np.random.default_rng(3000 + seed + 31 * W + H)
    x, y = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    base = 0.5 + 0.4 * np.sin(x / 3.0) * np.cos(y / 4.0)
    b = np.stack([base * s for s in (1.0, 0.8, 1.3)]).reshape(3, W * H) + 0.05 * rng.random((3, W * H))
    a = 0.9 * b + rng.normal(0, 0.15, (3, W * H))
    return np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)


# ---- the host entries inside guards ----------------------------------------------------------------------------------------------------------
def ptr(a):
    return None if a is None else a.ctypes.data


def guarded(n, dtype, fill):
    """An n-element array of `fill` inside GUARD elements of another pattern on either side -> (block, view)."""
    block = np.empty(n + 2 * GUARD, dtype=dtype)
    g = np.array([0x5A5A5A5A], dtype=np.uint32).view(F)[0] if dtype == F else 0x5A5A5A5A5A5A5A5A
    block[:] = g
    block[GUARD:GUARD + n] = fill
    return block, block[GUARD:GUARD + n]


def intact(block, n):
    ref = guarded(0, block.dtype.type, 0)[0]
    return bool(np.array_equal(block[:GUARD].view(np.uint8), ref[:GUARD].view(np.uint8))
                and np.array_equal(block[GUARD + n:].view(np.uint8), ref[GUARD:].view(np.uint8)))


def record(apt, passes_a=1, passes_b=1, **kw):
    return apt._lib.film_compare_record(passes_a, passes_b, **kw)


def compare_host(apt, rec, a, b, n=None, want_map=True):
    """apt_film_compare_host into garbage inside guards -> (rc, result uint64 [8], err_map or None, guards intact, untouched)."""
    n = a.shape[1] if n is None else n
    rb, res = guarded(COMPARE_WORDS, np.uint64, GARBAGE64)
    mb, emap = guarded(a.shape[1], F, np.nan) if want_map else (None, None)
    rc = apt._lib.metrics_lib().apt_film_compare_host(ctypes.byref(rec), ptr(a), ptr(b), n, ptr(res), ptr(emap))
    ok = intact(rb, COMPARE_WORDS) and (mb is None or intact(mb, a.shape[1]))
    untouched = bool(np.all(res == GARBAGE64)) and (emap is None or bool(np.isnan(emap).all()))
    return rc, res.copy(), None if emap is None else emap.copy(), ok, untouched


def ssim_host(apt, rec, a, b, W, H, want_map=True):
    """apt_film_ssim_host into garbage inside guards -> (rc, result uint64 [2], ssim_map or None, guards intact, untouched)."""
    windows = max(W - 10, 0) * max(H - 10, 0)
    rb, res = guarded(SSIM_WORDS, np.uint64, GARBAGE64)
    mb, smap = guarded(max(windows, 1), F, np.nan) if want_map else (None, None)
    rc = apt._lib.metrics_lib().apt_film_ssim_host(ctypes.byref(rec), ptr(a), ptr(b), W, H, ptr(res), ptr(smap))
    ok = intact(rb, SSIM_WORDS) and (mb is None or intact(mb, max(windows, 1)))
    untouched = bool(np.all(res == GARBAGE64)) and (smap is None or bool(np.isnan(smap).all()))
    return rc, res.copy(), None if smap is None else smap[:windows].copy(), ok, untouched


def assert_same(got, want):
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])
