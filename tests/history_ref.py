"""NumPy restatement of temporal accumulation (include/render_mi355x_history.h), for the tests only, written from the header's contract:
the geometry in float64 NumPy, one separately rounded operation per step in the header's order (f64() fails on a float32 intermediate
there), the blend and the export in float32 (f32() fails on a float64 one), the four taps as gathers whose accumulators keep their
values where a tap is rejected (np.where, not a zero weight).  Images are flat x-major arrays: pixel (x, y) sits at x * H + y.

`wrong=` makes three wrong implementations the tests hold the right one against: "cur_camera" (the current camera used in place of the
previous one), "no_plane" (the plane test dropped), "reverse_taps" (the taps summed in the reverse order).

Below the restatement: what the CPU and the GPU tests share -- the comparison, the cameras, the seeded inputs and the CPU twins' calls."""
import ctypes

import numpy as np

import camera_ref as cr
from materials_ref import F, f32

D = np.float64
COVERAGE, DEPTH, NORMAL, ALBEDO, PLANES = 0, 1, 2, 5, 8
HPLANES = 6
DEFAULTS = dict(max_history=32, tol_plane=0.01, tol_normal=0.9, min_weight=2.0 ** -10)
SIZES = [(1, 1), (1, 7), (7, 1), (5, 3), (33, 17)]                    # (W, H) of the CPU test; the GPU test adds the wave boundaries
GPU_SIZES = SIZES + [(3, 64), (3, 65), (2, 130), (9, 5)]


def f64(*arrays):
    """Every intermediate of the geometry is float64: fails loudly on a float32 one."""
    for a in arrays:
        assert np.asarray(a).dtype == np.float64, np.asarray(a).dtype
    return arrays[0] if len(arrays) == 1 else arrays


def lum(r, g, b):
    l = f32(F(0.2126) * r)
    l = f32(l + f32(F(0.7152) * g))
    return f32(l + f32(F(0.0722) * b))


def dot(p, q):
    return f64((p[0] * q[0] + p[1] * q[1]) + p[2] * q[2])


def cam_of(rec):
    """A camera_ref record (or anything with pos, g, cx, cy, offset) -> what the geometry reads, as float64."""
    get = (lambda k: rec[k]) if isinstance(rec, dict) else (lambda k: getattr(rec, k))
    c = {k: [D(v) for v in get(k)] for k in ("pos", "g", "cx", "cy")}
    c["offset"] = D(get("offset"))
    return c


def world(c, w, h, x, y, cov, depth):
    """The world points of pixels (x, y) (float64 arrays) of camera c with these planes' values (float64) -> [3] float64 arrays."""
    f64(w, h, x, y, cov, depth)
    a = (x + D(0.5)) / w - D(0.5)
    b = (y + D(0.5)) / h - D(0.5)
    d = [(c["cx"][k] * a + c["cy"][k] * b) + c["g"][k] for k in range(3)]
    nd = np.sqrt(dot(d, d))
    t = depth / cov
    return [f64((c["pos"][k] + d[k] * c["offset"]) + (d[k] / nd) * t) for k in range(3)]


def reproject(rec, cur_cam, prev_cam, cur, cur_feat, prev_feat, prev_hist, W, H, wrong=None, detail=False):
    """apt_film_history_* -> out float32 [6][N]; with detail also (valid bool [N], W float32 [N]).  rec: a dict of DEFAULTS' keys or an
    ApFilmHistory.  prev_hist None: the first frame."""
    get = (lambda k: rec[k]) if isinstance(rec, dict) else (lambda k: getattr(rec, k))
    assert 1 <= get("max_history") <= 1 << 24
    N = W * H
    cur = f32(np.ascontiguousarray(cur).reshape(3, N))
    l = lum(cur[0], cur[1], cur[2])
    new = [cur[0], cur[1], cur[2], l, f32(l * l)]
    out = np.empty((HPLANES, N), dtype=F)
    if prev_hist is None:
        for j in range(5):
            out[j] = new[j]
        out[5] = F(1)
        return (out, np.zeros(N, dtype=bool), np.zeros(N, dtype=F)) if detail else out
    cf = f32(np.ascontiguousarray(cur_feat).reshape(PLANES, N))
    pf = f32(np.ascontiguousarray(prev_feat).reshape(PLANES, N))
    ph = f32(np.ascontiguousarray(prev_hist).reshape(HPLANES, N))
    cc = cam_of(cur_cam)
    pc = cam_of(cur_cam if wrong == "cur_camera" else prev_cam)
    w, h = D(W), D(H)
    idx = np.arange(N)
    x, y = (idx // H).astype(D), (idx % H).astype(D)
    with np.errstate(all="ignore"):
        cov = cf[COVERAGE].astype(D)
        X = world(cc, w, h, x, y, cov, cf[DEPTH].astype(D))
        n_p = [f64(cf[NORMAL + k].astype(D) / cov) for k in range(3)]
        vp = [X[k] - cc["pos"][k] for k in range(3)]
        wv = [X[k] - pc["pos"][k] for k in range(3)]
        r = np.sqrt(dot(vp, vp))
        f = dot(wv, pc["g"]) / dot(pc["g"], pc["g"])
        ap = dot(wv, pc["cx"]) / (f * dot(pc["cx"], pc["cx"]))
        bp = dot(wv, pc["cy"]) / (f * dot(pc["cy"], pc["cy"]))
        u = (ap + D(0.5)) * w - D(0.5)
        v = (bp + D(0.5)) * h - D(0.5)
        x0, y0 = np.floor(u), np.floor(v)
        fx, fy = u - x0, v - y0
        bound = D(F(get("tol_plane"))) * r
        f64(r, f, ap, bp, u, v, x0, y0, fx, fy, bound)
        tol_normal = D(F(get("tol_normal")))
        taps = [(0, 0), (0, 1), (1, 0), (1, 1)]
        if wrong == "reverse_taps":
            taps = taps[::-1]
        Wt, S, Sh = np.zeros(N, dtype=F), [np.zeros(N, dtype=F) for _ in range(5)], np.zeros(N, dtype=F)
        for ex, ey in taps:
            qx, qy = x0 + D(ex), y0 + D(ey)
            wq = f64((fx if ex else D(1) - fx) * (fy if ey else D(1) - fy)).astype(F)
            inside = (qx >= 0) & (qx <= w - D(1)) & (qy >= 0) & (qy <= h - D(1))
            q = np.where(inside, qx, 0).astype(np.int64) * H + np.where(inside, qy, 0).astype(np.int64)
            covq = pf[COVERAGE][q].astype(D)
            hq = ph[5][q]
            Xq = world(pc, w, h, np.where(inside, qx, D(0)), np.where(inside, qy, D(0)), covq, pf[DEPTH][q].astype(D))
            nq = [f64(pf[NORMAL + k][q].astype(D) / covq) for k in range(3)]
            dist = np.abs(dot([Xq[k] - X[k] for k in range(3)], n_p))
            ok = (f > 0) & inside & (cov > 0) & (covq > 0) & (hq >= F(1)) & (dot(n_p, nq) >= tol_normal)
            if wrong != "no_plane":
                ok = ok & (dist <= bound)
            Wt = f32(np.where(ok, Wt + wq, Wt))
            S = [f32(np.where(ok, S[j] + f32(wq * ph[j][q]), S[j])) for j in range(5)]
            Sh = f32(np.where(ok, Sh + f32(wq * hq), Sh))
        valid = Wt >= F(get("min_weight"))
        hl = f32(Sh / Wt)
        t = f32(hl + F(1))
        mh = F(get("max_history"))
        assert int(mh) == get("max_history")
        hn = f32(np.where(t < mh, t, mh))
        alpha = f32(F(1) / hn)
        for j in range(5):
            Hj = f32(S[j] / Wt)
            out[j] = np.where(valid, f32(Hj + f32(alpha * f32(new[j] - Hj))), new[j])
        out[5] = np.where(valid, hn, F(1))
    return (out, valid, Wt) if detail else out


def export(hist):
    """apt_film_history_export_* -> (film [3][n], moments [2][n])."""
    hist = f32(np.ascontiguousarray(hist).reshape(HPLANES, -1))
    with np.errstate(all="ignore"):
        film = f32(hist[:3] + hist[:3])
        lm, q, h = hist[3], hist[4], hist[5]
        l2 = f32(lm * lm)
        hm = f32(h - F(1))
        d = f32(q - l2)
        var = np.where(hm >= F(1), f32(np.where(d > F(0), d, F(0)) / hm), q)
        qq = f32(l2 + f32(var))
        return film, np.stack([f32(lm + lm), f32(qq + qq)])


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------------------
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


def look_at(eye, target, up, vfov_deg, W, H, offset=0.0):
    """camera_ref.build_record for a look-at pinhole: the record apt_camera_build_host makes of the same inputs."""
    scale = 2.0 * np.tan(np.radians(D(vfov_deg)) / 2.0)
    return cr.build_record(eye, [D(t) - D(e) for t, e in zip(target, eye)], up, scale, offset, 0.0, 0.0, W, H)


EYE, EYE2, TARGET, UP, VFOV = (20.0, 60.0, 160.0), (50.0, 90.0, 130.0), (70.0, 20.0, 60.0), (0.1, 1.0, 0.05), 55.0


def cameras(W, H):
    """name -> (cur, prev) camera records for a W x H image, around a wall of points some 100 units in front of `base`:
    "same"; "translate" (the eye moved sideways and forward); "rotate" (the previous camera looked 25 degrees aside: part of the image
    is outside it); "behind" (the previous camera stood beyond the points and looked the same way: f <= 0)."""
    base = look_at(EYE, TARGET, UP, VFOV, W, H)
    moved = look_at((23.0, 61.0, 157.0), TARGET, UP, VFOV, W, H)
    aside = look_at(EYE, (110.0, 20.0, 95.0), UP, VFOV, W, H)
    g = base["g"]
    far = look_at([EYE[k] + 400.0 * g[k] for k in range(3)], [EYE[k] + 500.0 * g[k] for k in range(3)], UP, VFOV, W, H)
    return {"same": (base, base), "translate": (base, moved), "rotate": (base, aside), "behind": (base, far)}


def ctypes_camera(apt, rec):
    """A camera_ref record -> an ApCamera."""
    from ascendpathtracing_amd._lib import ApCamera
    return ApCamera.from_buffer_copy(cr.record_bytes(rec))


def wall(cam, W, H, seed, tilt=0.3, cov0=True, jitter=0.0):
    """Feature planes [8][N] of what `cam` sees of a slanted plane some 100 units in front of EYE: every pixel's depth is the distance
    from the pixel centre's ray origin to the plane, its normal the plane's, times a coverage in (0.5, 1] (cov0: a few pixels of
    coverage 0, all planes 0 there, as a miss leaves them); jitter: relative noise on the depth (pixels that fail the plane test)."""
    rng = np.random.default_rng(seed)
    N = W * H
    c = cam_of(cam)
    idx = np.arange(N)
    a = ((idx // H) + 0.5) / W - 0.5
    b = ((idx % H) + 0.5) / H - 0.5
    d = np.stack([(c["cx"][k] * a + c["cy"][k] * b) + c["g"][k] for k in range(3)])
    dn = d / np.linalg.norm(d, axis=0)
    o = np.stack([c["pos"][k] + d[k] * c["offset"] for k in range(3)])
    base = cam_of(look_at(EYE, TARGET, UP, VFOV, W, H))
    nrm = np.array(base["g"]) * -1.0 + tilt * np.array(base["cx"]) / np.linalg.norm(base["cx"])
    nrm /= np.linalg.norm(nrm)
    p0 = np.array(EYE) + 100.0 * np.array(base["g"])
    t = ((p0[:, None] - o) * nrm[:, None]).sum(0) / (dn * nrm[:, None]).sum(0)
    t = t * (1.0 + jitter * rng.standard_normal(N))
    cov = 0.5 + 0.5 * rng.random(N)
    cov[rng.random(N) < 0.25] = 1.0
    if cov0:
        cov[rng.random(N) < 0.1] = 0.0
    hit = (t > 0) & (cov > 0)
    cov = np.where(hit, cov, 0.0)
    feat = np.zeros((PLANES, N), dtype=F)
    feat[COVERAGE] = cov
    feat[DEPTH] = np.where(hit, t, 0.0) * cov
    feat[NORMAL:NORMAL + 3] = nrm[:, None] * cov
    feat[ALBEDO:ALBEDO + 3] = rng.random((3, N)) * cov
    return feat


def synthetic_history(W, H, seed, max_len=40.0):
    """A previous history [6][N] (lengths from 1 to max_len, a few below 1) and a current mean [3][N]."""
    rng = np.random.default_rng(seed + 77)
    N = W * H
    hist = np.empty((HPLANES, N), dtype=F)
    hist[:3] = rng.random((3, N)) * 2
    l = lum(hist[0], hist[1], hist[2])
    hist[3] = l
    hist[4] = l * l * (1 + rng.random(N)).astype(F)
    hist[5] = np.floor(1 + rng.random(N) * max_len)
    hist[5][rng.random(N) < 0.08] = F(0.5)
    hist[5][rng.random(N) < 0.05] = F(1.0)
    cur = (rng.random((3, N)) * 2).astype(F)
    return hist, cur


def case(W, H, name, seed=0, jitter=0.0):
    """The inputs of one named camera case -> (cur_cam, prev_cam, cur, cur_feat, prev_feat, prev_hist)."""
    cur_cam, prev_cam = cameras(W, H)[name]
    cur_feat = wall(cur_cam, W, H, seed + 1, jitter=jitter)
    prev_feat = wall(prev_cam, W, H, seed + 2)
    hist, cur = synthetic_history(W, H, seed)
    return cur_cam, prev_cam, cur, cur_feat, prev_feat, hist


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def record(apt, **fields):
    return apt._lib.film_history_record(**fields)


GUARD = 5


def history_host(apt, rec, cur_cam, prev_cam, cur, cur_feat, prev_feat, prev_hist, W, H):
    """apt_film_history_host into a NaN-filled output inside guard floats -> (rc, out [6][N], guards intact, output untouched)."""
    L = apt._lib.history_lib()
    N = W * H
    block = np.full(HPLANES * N + 2 * GUARD, np.nan, dtype=F)
    block[:GUARD] = block[-GUARD:] = F(-7)
    c = lambda a: None if a is None else np.ascontiguousarray(a, dtype=F)
    cur, cur_feat, prev_feat, prev_hist = c(cur), c(cur_feat), c(prev_feat), c(prev_hist)
    cc = ctypes_camera(apt, cur_cam) if isinstance(cur_cam, dict) else cur_cam
    pc = ctypes_camera(apt, prev_cam) if isinstance(prev_cam, dict) else prev_cam
    rc = L.apt_film_history_host(ctypes.byref(rec), ctypes.byref(cc), None if pc is None else ctypes.byref(pc), ptr(cur), ptr(cur_feat),
                                 ptr(prev_feat), ptr(prev_hist), W, H, ctypes.c_void_p(block.ctypes.data + 4 * GUARD))
    body = block[GUARD:GUARD + HPLANES * N]
    intact = bool(np.all(block[:GUARD] == F(-7)) and np.all(block[-GUARD:] == F(-7)))
    return rc, body.reshape(HPLANES, N).copy(), intact, bool(np.isnan(body).all())


def export_host(apt, hist):
    L = apt._lib.history_lib()
    hist = np.ascontiguousarray(hist, dtype=F)
    n = hist.size // HPLANES
    film, mom = np.full((3, n), np.nan, dtype=F), np.full((2, n), np.nan, dtype=F)
    rc = L.apt_film_history_export_host(ptr(hist), n, ptr(film), ptr(mom))
    return rc, film, mom


def export_case(n, seed=5):
    """A history buffer [6][n] for the export: lengths 1, 1.5, 2 and larger, q below lm^2 (the clamp), a NaN length and a NaN q."""
    rng = np.random.default_rng(seed + n)
    hist = np.empty((HPLANES, n), dtype=F)
    hist[:3] = rng.random((3, n)) * 3
    hist[3] = rng.random(n) + F(0.25)
    hist[4] = hist[3] * hist[3] * (0.9 + 0.6 * rng.random(n)).astype(F)
    hist[5] = np.array([1.0, 1.5, 2.0, 2.5, 7.0, 32.0], dtype=F)[np.arange(n) % 6]
    if n > 8:
        hist[5, 7] = np.nan
        hist[4, 8] = np.nan
    return hist
