"""NumPy restatement of the film's moments and its filter (include/render_mi355x_denoise.h: per-pixel luminance moments collected
pass by pass, and the albedo-demodulated, variance-guided, edge-avoiding a-trous filter), for the tests only.

Written from the header's contract: float32 NumPy, one separately rounded operation per step in the header's order, the taps in the
header's order with a pixel outside the image skipped (its accumulators keep their values: np.where, not a zero weight).  As in the
other restatements f32() fails on a float64 intermediate.  Images are handled as [W][H] arrays: pixel (x, y) sits at x * H + y.

Below the restatement: what the CPU and the GPU tests share -- the comparison, the seeded synthetic inputs and the calls of the CPU twins."""
import ctypes

import numpy as np

from materials_ref import F, f32

SIGMAS = ("sigma_n", "sigma_z", "sigma_c", "sigma_a", "sigma_l")
COVERAGE, DEPTH, NORMAL, ALBEDO, PLANES = 0, 1, 2, 5, 8
B3 = (F(1), F(2), F(1))
H5 = (F(1 / 16), F(4 / 16), F(6 / 16), F(4 / 16), F(1 / 16))


def lum(r, g, b):
    l = F(0.2126) * r
    l = l + F(0.7152) * g
    return f32(l + F(0.0722) * b)


def fmax(a, b):
    """The header's max: a > b ? a : b, so a NaN `a` falls to b."""
    return f32(np.where(a > b, a, F(b)).astype(F, copy=False))


def accumulate(passes):
    """apt_film_accumulate_* over the passes (float32 [3][n] each, in order) -> (film [3][n], moments [2][n])."""
    film = mom = None
    with np.errstate(all="ignore"):
        for k, p in enumerate(passes):
            p = f32(np.asarray(p))
            l = lum(p[0], p[1], p[2])
            l2 = f32(l * l)
            if k == 0:
                film, mom = p.copy(), np.stack([l, l2])
            else:
                film = f32(film + p)
                mom = f32(np.stack([mom[0] + l, mom[1] + l2]))
    return film, mom


def prepare(film, moments, features, passes, albedo_floor):
    """-> (n [3], z, A [3], cov, i [3], vi), each float32 of the planes' shape."""
    film, moments, features = f32(np.asarray(film), np.asarray(moments), np.asarray(features))
    K, K1 = F(passes), F(passes - 1)
    with np.errstate(all="ignore"):
        cov = features[COVERAGE]
        u = f32(F(1) - cov)
        A = [fmax(f32(features[ALBEDO + c] + u), albedo_floor) for c in range(3)]
        i = [f32(f32(film[c] / K) / A[c]) for c in range(3)]
        lm, q = f32(moments[0] / K), f32(moments[1] / K)
        v = f32(fmax(f32(q - f32(lm * lm)), 0) / K1)
        LA = lum(*A)
        vi = f32(v / f32(LA * LA))
    return [features[NORMAL + c] for c in range(3)], features[DEPTH], A, cov, i, vi


def _taps(W, H, reach, step):
    """(dx, dy, inside mask, clipped qx, clipped qy) over dx (outer), dy (inner) in -reach..reach, in the header's order."""
    X, Y = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
    for dx in range(-reach, reach + 1):
        for dy in range(-reach, reach + 1):
            qx, qy = X + dx * step, Y + dy * step
            inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            yield dx, dy, inside, np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)


def iterate(sig, n, z, A, cov, i, vi, step):
    """One a-trous iteration with step `step` on [W][H] arrays -> (i' [3], vi')."""
    W, H = vi.shape
    zero = np.zeros((W, H), dtype=F)
    with np.errstate(all="ignore"):
        sv, sw = zero, zero
        for ex, ey, inside, qx, qy in _taps(W, H, 1, 1):
            b = f32(B3[ex + 1] * B3[ey + 1])
            sv = np.where(inside, sv + b * vi[qx, qy], sv)
            sw = np.where(inside, sw + b, sw)
        gv = f32(f32(sv) / f32(sw))
        e = f32(np.sqrt(gv) * F(sig["sigma_l"]))
        e = f32(e + F(1e-6))
        isd = f32(F(1) / e)
        iz = f32(F(1) / f32(z + F(1e-6)))
        lp = lum(*i)
        Wt, S, V = zero, [zero, zero, zero], zero
        for dx, dy, inside, qx, qy in _taps(W, H, 2, step):
            cc = f32(cov * cov[qx, qy])
            dt = F(0) + n[0] * n[0][qx, qy]
            dt = dt + n[1] * n[1][qx, qy]
            dt = f32(dt + n[2] * n[2][qx, qy])
            xn = f32(F(sig["sigma_n"]) * fmax(f32(cc - dt), 0))
            xz = f32(f32(F(sig["sigma_z"]) * np.abs(f32(z - z[qx, qy]))) * iz)
            xc = f32(F(sig["sigma_c"]) * np.abs(f32(cov - cov[qx, qy])))
            da = f32(np.abs(f32(A[0] - A[0][qx, qy])) + np.abs(f32(A[1] - A[1][qx, qy])))
            da = f32(da + np.abs(f32(A[2] - A[2][qx, qy])))
            xa = f32(F(sig["sigma_a"]) * da)
            lq = lum(i[0][qx, qy], i[1][qx, qy], i[2][qx, qy])
            xl = f32(np.abs(f32(lp - lq)) * isd)
            x = f32(xn + xz)
            x = f32(x + xc)
            x = f32(x + xa)
            x = f32(x + xl)
            t = fmax(f32(F(1) - f32(x * F(0.125))), 0)
            t = f32(t * t)
            t = f32(t * t)
            g = f32(t * t) if (dx, dy) != (0, 0) else np.ones((W, H), dtype=F)      # the centre tap: x = 0 by definition
            w = f32(f32(H5[dx + 2] * H5[dy + 2]) * g)
            Wt = f32(np.where(inside, Wt + w, Wt))
            S = [f32(np.where(inside, S[c] + f32(w * i[c][qx, qy]), S[c])) for c in range(3)]
            V = f32(np.where(inside, V + f32(f32(w * w) * vi[qx, qy]), V))
        return [f32(S[c] / Wt) for c in range(3)], f32(V / f32(Wt * Wt))


def denoise(rec, film, moments, features, W, H, history=False):
    """apt_film_denoise_* for the record `rec` (an ApFilmDenoise, or anything with its fields) -> out float32 [3][W * H]; with history
    also the list of (i, vi) images: after prepare and after every iteration."""
    assert 2 <= rec.passes <= 1 << 24 and 1 <= rec.iterations <= 5
    sig = {k: getattr(rec, k) for k in SIGMAS}
    n, z, A, cov, i, vi = prepare(film, moments, features, rec.passes, rec.albedo_floor)
    sh = lambda a: a.reshape(W, H)
    n, A, i, z, cov, vi = [sh(a) for a in n], [sh(a) for a in A], [sh(a) for a in i], sh(z), sh(cov), sh(vi)
    steps = [(i, vi)]
    for j in range(rec.iterations):
        i, vi = iterate(sig, n, z, A, cov, i, vi, 1 << j)
        steps.append((i, vi))
    with np.errstate(all="ignore"):
        out = np.stack([f32(i[c] * A[c]).reshape(-1) for c in range(3)])
    return (out, steps) if history else out


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17), (40, 70)]         # (W, H): all but the last inside the 32-pixel reach of step 16


def assert_same(got, want):
    """Bit for bit, NaN positions included: a NaN where and only where the other has one (IEEE leaves a NaN's sign and payload to
    the implementation), every other value with the same bits."""
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), ("NaN positions", np.argwhere(gn != wn)[:5])
    diff = np.argwhere((got.view(np.uint32) != want.view(np.uint32)) & ~gn)
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def synthetic(W, H, passes=3, seed=0, nan=True):
    """Seeded planes of a W x H image -> (pass planes [passes][3][N], features [8][N]).  Columns of full, partial and zero coverage, an
    albedo-0 "emitter" block, pixels whose passes are all equal (zero variance) and, with nan, one NaN in pass 1."""
    rng = np.random.default_rng(1000 * W + H + seed)
    N = W * H
    x, y = np.divmod(np.arange(N), H)
    kind = (x * 3 // max(W, 1) + y // 5) % 3                          # 0 full, 1 partial, 2 zero coverage
    cov = np.where(kind == 0, 1.0, np.where(kind == 1, rng.random(N) * 0.9 + 0.05, 0.0)).astype(F)
    feat = np.zeros((PLANES, N), dtype=F)
    feat[COVERAGE] = cov
    feat[DEPTH] = (cov * (50 + 100 * rng.random(N))).astype(F)
    nrm = rng.normal(size=(3, N))
    feat[NORMAL:NORMAL + 3] = (nrm / np.linalg.norm(nrm, axis=0) * cov).astype(F)
    alb = rng.random((3, N)) * 0.9
    alb[:, (x % 4 == 1) & (y % 4 < 2)] = 0.0                          # the emitter block
    feat[ALBEDO:ALBEDO + 3] = (alb * cov).astype(F)
    base = (rng.random((3, N)) * 2).astype(F)
    ps = np.stack([(base * (0.25 + 1.5 * rng.random((3, N)))).astype(F) for _ in range(passes)])
    still = (x + 2 * y) % 7 == 3                                      # zero variance: every pass the same
    ps[:, :, still] = base[:, still]
    if nan:
        ps[min(1, passes - 1), 1, N // 2] = np.nan
    return ps, feat


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def accumulate_host(apt, passes):
    """apt_film_accumulate_host over the passes, into buffers that start as NaN -> (film, moments)."""
    L = apt._lib.denoise_lib()
    n = passes[0].shape[1]
    film, mom = np.full((3, n), np.nan, dtype=F), np.full((2, n), np.nan, dtype=F)
    for k, p in enumerate(passes):
        assert L.apt_film_accumulate_host(ptr(np.ascontiguousarray(p, dtype=F)), n, ptr(film), ptr(mom), k) == 0
    return film, mom


GUARD = 8   # floats on either side of work and out: a multiple of 4, so work stays 16-byte aligned


def denoise_host(apt, rec, film, moments, features, W, H):
    """apt_film_denoise_host -> (rc, out [3][N], work [16 N], guards intact)."""
    L = apt._lib.denoise_lib()
    N = W * H
    block = np.full(16 * N + 2 * GUARD + 4, -7.0, dtype=F)
    skew = (-block.ctypes.data // 4) % 4                               # floats to the next 16-byte boundary
    work = block[skew + GUARD: skew + GUARD + 16 * N]
    assert work.ctypes.data % 16 == 0
    outb = np.full(3 * N + 2 * GUARD, -7.0, dtype=F)
    out = outb[GUARD:GUARD + 3 * N]
    rc = L.apt_film_denoise_host(ctypes.byref(rec), ptr(np.ascontiguousarray(film, dtype=F)), ptr(np.ascontiguousarray(moments, dtype=F)),
                                 ptr(np.ascontiguousarray(features, dtype=F)), W, H, ctypes.c_void_p(work.ctypes.data),
                                 ctypes.c_void_p(out.ctypes.data))
    guards = (np.all(block[:skew + GUARD] == -7.0) and np.all(block[skew + GUARD + 16 * N:] == -7.0)
              and np.all(outb[:GUARD] == -7.0) and np.all(outb[GUARD + 3 * N:] == -7.0))
    return rc, out.reshape(3, N).copy(), work.copy(), guards
