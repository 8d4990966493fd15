"""NumPy restatement of guided film upscaling (include/render_mi355x_upscale.h), for the tests only, written from the header's contract:
the coordinates in float64 NumPy, one separately rounded operation per step in the header's order (f64() fails on a float32
intermediate there), prepare, the guided sum, the decision and the patch in float32 (f32() fails on a float64 one), the four taps as
gathers whose accumulators keep their values where a tap does not enter (np.where, not a zero weight).  Images are flat x-major
arrays: pixel (x, y) sits at x * H + y.

`wrong=` makes the wrong implementations the tests hold the right one against: "reverse_taps" (the taps summed in the reverse order),
"lo_albedo" (re-modulation with the bilinearly interpolated low-res albedo in place of the full-size pixel's own), "no_g" (g dropped:
plain bilinear interpolation of the demodulated illumination).  plain=True is the baseline of the quality condition: g dropped AND
no demodulation (bilinear interpolation of the radiance itself).

Below the restatement: what the CPU and the GPU tests share -- the comparison, the seeded inputs, the closed-form cases and the CPU
twins' calls."""
import ctypes

import numpy as np

from history_ref import f64
from materials_ref import F, f32

D = np.float64
U32 = np.uint32
COVERAGE, DEPTH, NORMAL, ALBEDO, PLANES = 0, 1, 2, 5, 8
DEFAULTS = dict(sigma_n=32.0, sigma_z=10.0, sigma_c=8.0, sigma_a=8.0, albedo_floor=1.0 / 32, min_weight=2.0 ** -6)
# (lo_w, lo_h, w, h): the CPU test's sizes; 7x5 -> 33x17 is a non-integer ratio, two are equal sizes
SIZES = [(1, 1, 1, 1), (1, 1, 3, 2), (1, 4, 1, 7), (4, 1, 7, 1), (3, 2, 5, 3), (4, 4, 8, 8), (7, 5, 33, 17), (5, 3, 5, 3), (8, 8, 8, 8)]
# the GPU test adds full sizes from halves on both sides of a wave's 64 lanes in the contiguous axis
GPU_SIZES = SIZES + [(2, 32, 3, 64), (2, 33, 3, 65), (1, 65, 2, 130), (5, 3, 9, 5)]


def big_size():
    """One case of 70 001 full pixels from an odd low size.  70 001 is prime, so the image is one column: 1 x 70 001 from 1 x 35 001,
    274 workgroups along the contiguous axis with a ragged last one."""
    return (1, 35001, 1, 70001)


def fmax(a, b):
    """a > b ? a : b: a NaN a falls to b."""
    return f32(np.where(a > b, a, b))


def _get(rec):
    return (lambda k: rec[k]) if isinstance(rec, dict) else (lambda k: getattr(rec, k))


def albedo_of(feat, floor):
    """A = max(albedo + (1 - cov), floor) per channel -> [3] float32 arrays."""
    u = f32(F(1) - feat[COVERAGE])
    return [fmax(f32(feat[ALBEDO + ch] + u), F(floor)) for ch in range(3)]


def prepare(rec, lo, lo_feat):
    """-> work float32 [3][Nl][4]: (i.rgb, cov), (n.xyz, z), (A.rgb, 0)."""
    get = _get(rec)
    lf = f32(np.ascontiguousarray(lo_feat).reshape(PLANES, -1))
    nl = lf.shape[1]
    lo = f32(np.ascontiguousarray(lo).reshape(3, nl))
    with np.errstate(all="ignore"):
        A = albedo_of(lf, get("albedo_floor"))
        il = [f32(lo[ch] / A[ch]) for ch in range(3)]
    work = np.zeros((3, nl, 4), dtype=F)
    for ch in range(3):
        work[0, :, ch] = il[ch]
        work[1, :, ch] = lf[NORMAL + ch]
        work[2, :, ch] = A[ch]
    work[0, :, 3] = lf[COVERAGE]
    work[1, :, 3] = lf[DEPTH]
    return work


def axis(k, low, full):
    """One axis of the coordinates: float64 arrays (k0, f)."""
    k = np.asarray(k).astype(D)
    c = k + D(0.5)
    s = c * D(low)
    u = s / D(full) - D(0.5)
    k0 = np.floor(u)
    return f64(k0, u - k0)


def upscale(rec, lo, lo_feat, lw, lh, hi_feat, W, H, wrong=None, plain=False):
    """apt_film_upscale_* -> (out float32 [3][N], resolved uint32 [N], work float32 [3][Nl][4])."""
    get = _get(rec)
    N, nl = W * H, lw * lh
    hf = f32(np.ascontiguousarray(hi_feat).reshape(PLANES, N))
    work = prepare(rec, lo, lo_feat)
    assert work.shape[1] == nl
    lo = f32(np.ascontiguousarray(lo).reshape(3, nl))
    ci, gn, ga = work[0], work[1], work[2]
    sn, sz, sc, sa = (F(get(k)) for k in ("sigma_n", "sigma_z", "sigma_c", "sigma_a"))
    idx = np.arange(N)
    x0, fx = axis(idx // H, lw, W)
    y0, fy = axis(idx % H, lh, H)
    taps = [(0, 0), (0, 1), (1, 0), (1, 1)]
    if wrong == "reverse_taps":
        taps = taps[::-1]
    with np.errstate(all="ignore"):
        cov_p, z_p = hf[COVERAGE], hf[DEPTH]
        n_p = [hf[NORMAL + k] for k in range(3)]
        A_p = albedo_of(hf, get("albedo_floor"))
        iz = f32(F(1) / f32(z_p + F(1e-6)))
        zero = lambda: np.zeros(N, dtype=F)
        Wg, Sg, Wf, Sf = zero(), [zero() for _ in range(3)], zero(), [zero() for _ in range(3)]
        Al = [zero() for _ in range(3)]                              # (wrong="lo_albedo": the fallback-weighted low-res albedo)
        for ex, ey in taps:
            qx, qy = x0 + D(ex), y0 + D(ey)
            b = f64((fx if ex else D(1) - fx) * (fy if ey else D(1) - fy)).astype(F)
            inside = (qx >= 0) & (qx <= D(lw) - D(1)) & (qy >= 0) & (qy <= D(lh) - D(1))
            q = np.where(inside, qx, 0).astype(np.int64) * lh + np.where(inside, qy, 0).astype(np.int64)
            c_q, n_q, a_q = ci[q], gn[q], ga[q]
            val = [lo[ch][q] for ch in range(3)] if plain else [c_q[:, ch] for ch in range(3)]
            cc = f32(cov_p * c_q[:, 3])
            dt = f32(F(0) + f32(n_p[0] * n_q[:, 0]))
            dt = f32(dt + f32(n_p[1] * n_q[:, 1]))
            dt = f32(dt + f32(n_p[2] * n_q[:, 2]))
            xn = f32(sn * fmax(f32(cc - dt), F(0)))
            xz = f32(f32(sz * np.abs(f32(z_p - n_q[:, 3]))) * iz)
            xc = f32(sc * np.abs(f32(cov_p - c_q[:, 3])))
            da = f32(np.abs(f32(A_p[0] - a_q[:, 0])) + np.abs(f32(A_p[1] - a_q[:, 1])))
            da = f32(da + np.abs(f32(A_p[2] - a_q[:, 2])))
            xa = f32(sa * da)
            xs = f32(f32(f32(xn + xz) + xc) + xa)
            t = fmax(f32(F(1) - f32(xs * F(0.125))), F(0))
            t = f32(t * t)
            t = f32(t * t)
            g = np.ones(N, dtype=F) if (wrong == "no_g" or plain) else f32(t * t)
            w = f32(b * g)
            enter = inside & (w > 0)
            Wg = f32(np.where(enter, Wg + w, Wg))
            Sg = [f32(np.where(enter, Sg[ch] + f32(w * val[ch]), Sg[ch])) for ch in range(3)]
            fall = inside & (b > 0)
            Wf = f32(np.where(fall, Wf + b, Wf))
            Sf = [f32(np.where(fall, Sf[ch] + f32(b * val[ch]), Sf[ch])) for ch in range(3)]
            Al = [f32(np.where(fall, Al[ch] + f32(b * a_q[:, ch]), Al[ch])) for ch in range(3)]
        ok = Wg >= F(get("min_weight"))
        Wt = f32(np.where(ok, Wg, Wf))
        out = np.empty((3, N), dtype=F)
        for ch in range(3):
            ip = f32(f32(np.where(ok, Sg[ch], Sf[ch])) / Wt)
            if plain:
                out[ch] = ip
            elif wrong == "lo_albedo":
                out[ch] = f32(ip * f32(Al[ch] / Wf))
            else:
                out[ch] = f32(ip * A_p[ch])
    return out, ok.astype(U32), work


def patch(sums, lst, passes, out):
    """apt_film_upscale_patch_* on a copy of out [3][N] -> out; lst without repeats among its entries inside the image."""
    out = f32(np.array(out, dtype=F, copy=True))
    lst = np.asarray(lst, dtype=U32)
    sums = f32(np.asarray(sums, dtype=F).reshape(3, lst.size))
    assert 1 <= passes <= 1 << 24
    keep = lst < out.shape[1]
    p = lst[keep].astype(np.int64)
    assert np.unique(p).size == p.size
    with np.errstate(all="ignore"):
        out[:, p] = f32(sums[:, keep] / F(passes))
    return out


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
def assert_same(got, want):
    """Bit for bit, NaN positions included (IEEE leaves a NaN's sign and payload to the implementation)."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), ("NaN positions", np.argwhere(gn != wn)[:5])
    diff = np.argwhere((got.view(U32) != want.view(U32)) & ~gn)
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape != b.shape or not np.array_equal(a.view(U32), b.view(U32))


def random_planes(w, h, seed):
    """Feature planes [8][N] of a few random flat patches: a coverage in (0.5, 1] (a quarter exactly 1, a tenth 0 with every plane 0,
    as a miss leaves them), unit normals and a depth per patch with a little noise, a random albedo, all times the coverage."""
    rng = np.random.default_rng(seed)
    n = w * h
    idx = np.arange(n)
    patch_of = ((idx // h) * 3 // max(w, 1)) * 2 + ((idx % h) * 2 // max(h, 1))            # 3 x 2 patches
    nrm = rng.standard_normal((6, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    depth = 50.0 + 100.0 * rng.random(6)
    alb = rng.random((6, 3))
    cov = 0.5 + 0.5 * rng.random(n)
    cov[rng.random(n) < 0.25] = 1.0
    cov[rng.random(n) < 0.1] = 0.0
    feat = np.zeros((PLANES, n), dtype=F)
    feat[COVERAGE] = cov
    feat[DEPTH] = depth[patch_of] * (1.0 + 0.01 * rng.standard_normal(n)) * cov
    feat[NORMAL:NORMAL + 3] = nrm[patch_of].T * cov
    feat[ALBEDO:ALBEDO + 3] = (alb[patch_of].T * (0.9 + 0.1 * rng.random((3, n)))) * cov
    return feat


def case(lw, lh, w, h, seed=0):
    """-> (lo [3][Nl], lo_feat, hi_feat): random patches at both sizes (the same patch layout and values: the seeds of the patch
    tables agree, the per-pixel noise does not) and a random low radiance."""
    rng = np.random.default_rng(seed + 1000)
    lo_feat, hi_feat = random_planes(lw, lh, seed), random_planes(w, h, seed)
    lo = (rng.random((3, lw * lh)) * 2).astype(F)
    return lo, lo_feat, hi_feat


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def record(apt, **fields):
    return apt._lib.film_upscale_record(**fields)


GUARD = 8               # guard words on both sides of every output (8 floats = 32 bytes: work stays 16-byte aligned)


def guarded(count, dtype, fill):
    """-> (block, body view, pointer to the body) with GUARD words of the guard value on both sides; the block is 16-byte aligned."""
    raw = np.empty(count + 2 * GUARD + 4, dtype=dtype)
    off = (-raw.ctypes.data // 4) % 4
    block = raw[off:off + count + 2 * GUARD]
    assert block.ctypes.data % 16 == 0
    block[:] = fill
    block[:GUARD] = block[GUARD + count:] = np.array(-7 if dtype == F else 0xDEADBEEF, dtype=dtype)
    return block, block[GUARD:GUARD + count], ctypes.c_void_p(block.ctypes.data + 4 * GUARD)


def guards_intact(block, count):
    g = np.array(-7 if block.dtype == F else 0xDEADBEEF, dtype=block.dtype)
    return bool(np.all(block[:GUARD] == g) and np.all(block[GUARD + count:] == g))


def upscale_host(apt, rec, lo, lo_feat, lw, lh, hi_feat, W, H):
    """apt_film_upscale_host into NaN-filled out, 0xFFFFFFFF-filled resolved and garbage-filled work inside guard words
    -> (rc, out [3][N], resolved [N], work [3][Nl][4], guards intact, outputs untouched)."""
    L = apt._lib.upscale_lib()
    N, nl = W * H, lw * lh
    c = lambda a: np.ascontiguousarray(a, dtype=F)
    lo, lo_feat, hi_feat = c(lo), c(lo_feat), c(hi_feat)
    ob, out, op = guarded(3 * N, F, np.nan)
    rb, res, rp = guarded(N, U32, 0xFFFFFFFF)
    wb, work, wp = guarded(12 * nl, F, F(-3.5))
    rc = L.apt_film_upscale_host(ctypes.byref(rec), ptr(lo), ptr(lo_feat), lw, lh, ptr(hi_feat), W, H, wp, op, rp)
    intact = guards_intact(ob, 3 * N) and guards_intact(rb, N) and guards_intact(wb, 12 * nl)
    untouched = bool(np.isnan(out).all() and np.all(res == 0xFFFFFFFF) and np.all(work == F(-3.5)))
    return rc, out.reshape(3, N).copy(), res.copy(), work.reshape(3, nl, 4).copy(), intact, untouched


def patch_host(apt, sums, lst, passes, out, n=None):
    """apt_film_upscale_patch_host on a copy of out inside guard floats -> (rc, out, guards intact)."""
    L = apt._lib.upscale_lib()
    out = np.ascontiguousarray(out, dtype=F)
    n = out.shape[1] if n is None else n
    lst, sums = np.ascontiguousarray(lst, dtype=U32), np.ascontiguousarray(sums, dtype=F)
    ob, body, op = guarded(out.size, F, np.nan)
    body[:] = out.ravel()
    one = np.zeros(1, dtype=F)                                        # (an empty array's pointer may be anything: list_count = 0)
    rc = L.apt_film_upscale_patch_host(ptr(sums if sums.size else one), ptr(lst if lst.size else one.view(U32)), lst.size, passes, n, op)
    return rc, body.reshape(out.shape).copy(), guards_intact(ob, out.size)


def unresolved_host(apt, resolved):
    """The list of the pixels with resolved == 0 through the UNCHANGED apt_film_select_host, as the header says -> uint32 list."""
    import adaptive_ref as ar
    n = resolved.size
    rec = apt._lib.film_select_record(2, min_passes=3, max_passes=3)
    rc, lst, count, untouched = ar.select_host(apt, np.zeros((2, n), dtype=F), np.ascontiguousarray(resolved, dtype=U32), rec)
    assert rc == 0 and untouched and count == lst.size
    return lst
