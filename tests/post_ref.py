"""include/render_mi355x_post.h restated in NumPy: the luminance histogram, the exposure derived from it, and the bloom (bright-pass,
pyramid, composite), every arithmetic step one fp32 operation in the header's order -- NumPy's float32 ufuncs round each operation on
its own and fuse nothing.  tests/test_post_cpu.py holds libpost_mi355x.so's CPU twins to it bit for bit, tests/test_gpu_post.py the
device entries to the twins.  Also what those two files share: the comparisons, the films, and the calls of the host entries into
NaN-filled outputs inside guard words."""
import ctypes

import numpy as np

F, D = np.float32, np.float64
BINS, WORDS = 256, 257
METER_DEFAULTS = dict(low_q=6554, high_q=58982, key=0.18, min_exposure=2.0 ** -12, max_exposure=2.0 ** 12, adapt=1.0)
BLOOM_DEFAULTS = dict(levels=5, threshold=1.0, cap=2.0 ** 16, spread=1.0, intensity=0.05)
METER_SIZES = [1, 63, 64, 65, 257, 1001]
BLOOM_SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17)]                # (W, H) of the CPU test; the GPU test adds the wave boundaries
BLOOM_GPU_SIZES = BLOOM_SIZES + [(3, 64), (3, 65), (2, 130), (9, 5), (64, 48)]
BLOOM_LEVELS = (1, 2, 6)
GUARD = 16                                                              # words: a multiple of 4, so that alignment survives it


def lum(r, g, b):
    l = F(0.2126) * r
    l = l + F(0.7152) * g
    return l + F(0.0722) * b


def fmax(a, b):
    return np.where(a > b, a, b)                                        # the header's select: a NaN in `a` gives b


# ---- metering ------------------------------------------------------------------------------------------------------------------------------
def meter_index(film, passes):
    """film [3][n] -> the histogram word of every pixel, int64 [n]."""
    film = np.ascontiguousarray(film, dtype=F)
    with np.errstate(all="ignore"):
        c = film / F(passes)
        l = np.ascontiguousarray(lum(c[0], c[1], c[2]), dtype=F)
        e = (l.view(np.uint32) >> 20).astype(np.int64) - 888
        return np.where(l > 0, np.clip(e, 0, 255), 256)


def meter(film, passes):
    return np.bincount(meter_index(film, passes), minlength=WORDS).astype(np.uint32)


def bin_value(half_bins):
    """The float whose bits are (888 << 20) + (half_bins << 19)."""
    return np.array([(888 << 20) + (int(half_bins) << 19)], dtype=np.uint32).view(F)[0]


def exposure(rec, hist, prev):
    """rec: a dict of METER_DEFAULTS' keys (or a record with those attributes).  Python integers for the selection, fp32 for the rest."""
    get = (lambda k: rec[k]) if isinstance(rec, dict) else (lambda k: getattr(rec, k))
    h = [int(v) for v in np.asarray(hist).ravel()[:BINS]]
    prev = F(prev)
    n = sum(h)
    if n == 0:
        return prev

    def percentile(q):
        cum = 0
        for b in range(BINS):
            cum += h[b]
            if cum * 65536 >= q * n:
                return b
        raise AssertionError("unreachable: cum(255) = n")

    b_lo, b_hi = percentile(int(get("low_q"))), percentile(int(get("high_q")))
    C = sum(h[b] for b in range(b_lo, b_hi + 1))
    S = sum(h[b] * (2 * b + 1) for b in range(b_lo, b_hi + 1))
    L = bin_value(S // C)
    key, lo, hi, adapt = F(get("key")), F(get("min_exposure")), F(get("max_exposure")), F(get("adapt"))
    t = key / L
    t = t if t < hi else hi
    t = t if t > lo else lo
    if adapt >= 1:
        return F(t)
    d = F(t - prev)
    return F(prev + F(d * adapt))


# ---- bloom ---------------------------------------------------------------------------------------------------------------------------------
def bright(film, W, H, passes, cap, threshold, wrong=None):
    """film [3][N] -> the bright image [3][W][H]."""
    with np.errstate(all="ignore"):
        m = np.ascontiguousarray(film, dtype=F).reshape(3, W, H) / F(passes)
        x = np.where(m > 0, m, F(0))
        if wrong != "no_cap":
            x = np.where(x < F(cap), x, F(cap))
        l = lum(x[0], x[1], x[2])
        g = fmax(l - F(threshold), F(0)) / fmax(l, F(1e-6))
        return (x * g).astype(F)


def _taps(lo, hi, wrong):
    order = [(a, b) for a in range(lo, hi + 1) for b in range(lo, hi + 1)]
    return order[::-1] if wrong == "reverse_taps" else order


def down(src, wrong=None):
    """[3][ws][hs] -> [3][(ws + 1) >> 1][(hs + 1) >> 1]."""
    _, ws, hs = src.shape
    wd, hd = (ws + 1) >> 1, (hs + 1) >> 1
    X, Y = np.meshgrid(np.arange(wd), np.arange(hd), indexing="ij")
    Wt, S = np.zeros((wd, hd), dtype=F), np.zeros((3, wd, hd), dtype=F)
    k = {-1: 1.0, 0: 3.0, 1: 3.0, 2: 1.0}
    with np.errstate(all="ignore"):
        for dx, dy in _taps(-1, 2, wrong):
            qx, qy = 2 * X + dx, 2 * Y + dy
            inside = (qx >= 0) & (qx < ws) & (qy >= 0) & (qy < hs)
            v = src[:, np.clip(qx, 0, ws - 1), np.clip(qy, 0, hs - 1)]
            if wrong == "clamp":
                inside = np.ones_like(inside)
            w = F(k[dx] * k[dy])
            Wt = np.where(inside, Wt + w, Wt)
            S = np.where(inside[None], S + w * v, S)
        return (S / Wt).astype(F)


def up(c, wf, hf, wrong=None):
    """The coarse level c [3][wc][hc] at every pixel of a wf x hf image -> [3][wf][hf]."""
    _, wc, hc = c.shape
    X, Y = np.meshgrid(np.arange(wf), np.arange(hf), indexing="ij")
    x0, y0 = (X - 1) >> 1, (Y - 1) >> 1
    wx0, wy0 = np.where(X & 1, F(0.75), F(0.25)).astype(F), np.where(Y & 1, F(0.75), F(0.25)).astype(F)
    u = np.zeros((3, wf, hf), dtype=F)
    with np.errstate(all="ignore"):
        for tx, ty in _taps(0, 1, wrong):
            qx, qy = np.clip(x0 + tx, 0, wc - 1), np.clip(y0 + ty, 0, hc - 1)
            w = (F(1) - wx0 if tx else wx0) * (F(1) - wy0 if ty else wy0)
            u = u + w * c[:, qx, qy]
    return u.astype(F)


def bloom(rec, film, W, H, passes=1, wrong=None, detail=False):
    """rec: a dict of BLOOM_DEFAULTS' keys (or a record with those attributes and `passes`) -> out [3][N], or (out, B [3][N], the
    levels U_j as the work buffer holds them: a list of [3][w_j][h_j])."""
    if not isinstance(rec, dict):
        passes = rec.passes
        rec = {k: getattr(rec, k) for k in BLOOM_DEFAULTS}
    levels, spread, intensity = int(rec["levels"]), F(rec["spread"]), F(rec["intensity"])
    film = np.ascontiguousarray(film, dtype=F)
    Dl = [down(bright(film, W, H, passes, rec["cap"], rec["threshold"], wrong), wrong)]
    for _ in range(1, levels):
        Dl.append(down(Dl[-1], wrong))
    U = [None] * levels
    U[-1] = Dl[-1]
    with np.errstate(all="ignore"):
        for j in range(levels - 2, -1, -1):
            U[j] = Dl[j] + spread * up(U[j + 1], Dl[j].shape[1], Dl[j].shape[2], wrong)
        B = up(U[0], W, H, wrong)
        out = (film.reshape(3, W, H) / F(passes) + intensity * B).astype(F).reshape(3, W * H)
    return (out, B.reshape(3, W * H), U) if detail else out


def level_sizes(W, H, levels):
    out = []
    for _ in range(levels):
        W, H = (W + 1) >> 1, (H + 1) >> 1
        out.append((W, H))
    return out


# ---- what the CPU and the GPU tests share -----------------------------------------------------------------------------------------------
def assert_same(got, want):
    """Bit for bit, NaN positions included (IEEE leaves a NaN's sign and payload to the implementation)."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), ("NaN positions", np.argwhere(gn != wn)[:5])
    diff = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~gn)
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ptr(a):
    return None if a is None else a.ctypes.data


EDGES = np.array([2.0 ** -16, np.nextafter(F(2.0 ** -16), F(0)), 2.0 ** 16, np.nextafter(F(2.0 ** 16), F(0)), 1e-40, 0.0, -0.0, -3.0, np.inf,
                  np.nan], dtype=F)


def with_lum(T):
    """A pixel (r, 0, b) whose lum is EXACTLY the normal float T: red brings the luminance to a few ulps below T, blue -- whose term is
    then far finer than T's ulp -- the rest."""
    T = F(T)
    r = F(T / F(0.2126))
    while F(F(0.2126) * r) >= T:
        r = np.nextafter(r, F(0))
    q = F(T - F(F(0.2126) * r))                                         # exact: both are within a few ulps of T
    b = F(q / F(0.0722))
    for _ in range(8):
        if lum(r, F(0), b) == T:
            return (r, F(0), b)
        b = np.nextafter(b, F(np.inf) if lum(r, F(0), b) < T else F(0))
    raise AssertionError("no pixel of luminance %r" % T)


def edge_pixels():
    """[3][10]: 2^-16 and its predecessor, 2^16 and its predecessor as exact luminances; a subnormal, +0, -0, a negative value, +inf
    and NaN as grey pixels."""
    cols = [with_lum(v) for v in EDGES[:4]] + [(v, v, v) for v in EDGES[4:]]
    px = np.ascontiguousarray(np.array(cols, dtype=F).T)
    l = lum(px[0], px[1], px[2])
    assert np.array_equal(l[:4].view(np.uint32), EDGES[:4].view(np.uint32)) and 0 < l[4] < 2.0 ** -126
    return px


def meter_film(n, seed=0, edges=True):
    """[3][n]: pixels whose luminance is log-uniform over about 2^-20 .. 2^20, and (edges) edge_pixels() in the first ten places,
    rotated by the seed so that a film of fewer pixels sees other ones."""
    rng = np.random.default_rng(seed)
    film = np.exp2(rng.uniform(-20, 20, (1, n))).astype(F) * rng.uniform(0.5, 1.5, (3, n)).astype(F)
    if edges:
        k = min(n, EDGES.size)
        film[:, :k] = edge_pixels()[:, (np.arange(k) + seed) % EDGES.size]
    return np.ascontiguousarray(film)


def bin_film():
    """[3][256]: one pixel per bin, (v, v, v) with v the middle of the bin; lum(v, v, v) stays inside it."""
    v = np.array([bin_value(2 * b + 1) for b in range(BINS)], dtype=F)
    return np.ascontiguousarray(np.stack([v, v, v]))


def bloom_film(W, H, seed=0, bad=False):
    """[3][W*H]: mostly below the default threshold, a few pixels far above it; bad: a NaN, a +inf and a negative pixel among them."""
    rng = np.random.default_rng(seed + 17 * W + H)
    N = W * H
    film = (rng.random((3, N)) * 0.9).astype(F)
    hot = rng.random(N) < 0.15
    film[:, hot] *= F(40.0)
    if bad:
        film[0, (3 * N) // 7] = np.nan
        film[1, (5 * N) // 7] = np.inf
        film[2, N // 2] = -4.0
        film[:, N - 1] = (-1.0, np.inf, np.nan)
    return np.ascontiguousarray(film)


def _guarded(n, dtype, fill):
    """An n-element array inside GUARD words on either side, its first element 16-byte aligned -> (block, view)."""
    raw = np.empty(n + 2 * GUARD + 4, dtype=dtype)
    off = (-(raw.ctypes.data // 4 + GUARD)) % 4
    block = raw[off:off + n + 2 * GUARD]
    block[:GUARD] = 0x5A5A5A5A if dtype == np.uint32 else -7.0
    block[GUARD + n:] = 0x5A5A5A5A if dtype == np.uint32 else -7.0
    block[GUARD:GUARD + n] = fill
    assert block[GUARD:].ctypes.data % 16 == 0
    return block, block[GUARD:GUARD + n]


def _intact(block, n):
    g = 0x5A5A5A5A if block.dtype == np.uint32 else -7.0
    return bool(np.all(block[:GUARD] == g) and np.all(block[GUARD + n:] == g))


GARBAGE = 0xDEADBEEF


def meter_host(apt, rec, film, n=None):
    """apt_film_meter_host into garbage-filled words inside guards -> (rc, hist, guards intact, untouched)."""
    n = film.shape[1] if n is None else n
    block, hist = _guarded(WORDS, np.uint32, GARBAGE)
    rc = apt._lib.post_lib().apt_film_meter_host(ctypes.byref(rec), ptr(film), n, ptr(hist))
    return rc, hist.copy(), _intact(block, WORDS), bool(np.all(hist == GARBAGE))


def bloom_host(apt, rec, film, W, H, detail=False):
    """apt_film_bloom_host into NaN-filled out and work inside guards -> (rc, out [3][N], guards intact, untouched[, work])."""
    N = W * H
    floats = 4 * sum(w * h for w, h in level_sizes(W, H, max(1, min(6, int(rec.levels)))))
    ob, out = _guarded(3 * N, F, np.nan)
    wb, work = _guarded(floats, F, np.nan)
    rc = apt._lib.post_lib().apt_film_bloom_host(ctypes.byref(rec), ptr(film), W, H, ptr(work), ptr(out))
    res = (rc, out.reshape(3, N).copy(), _intact(ob, 3 * N) and _intact(wb, floats), bool(np.isnan(out).all() and np.isnan(work).all()))
    return res + (work.copy(),) if detail else res


def work_levels(work, W, H, levels):
    """The work buffer's records -> the levels as [3][w_j][h_j] arrays (and the records' fourth words, which must be 0)."""
    out, pads, at = [], [], 0
    for w, h in level_sizes(W, H, levels):
        rec = work[at:at + 4 * w * h].reshape(w, h, 4)
        out.append(np.ascontiguousarray(rec[:, :, :3].transpose(2, 0, 1)))
        pads.append(rec[:, :, 3])
        at += 4 * w * h
    return out, pads
