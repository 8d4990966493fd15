"""CPU-only: temporal accumulation (libhistory_mi355x.so, include/render_mi355x_history.h) -- the binding against the header and the
exports, the CPU twins of the reprojection and the export bit for bit against the restatement tests/history_ref.py, every refusal, the
running mean under an unmoved camera, what the default tolerances do on the open 8-sphere scene under a float64 ray cast of the test's
own, and, on the restatement, that three wrong implementations are told from the right one.

Without the feature nothing here passes: the library, the header, the binding and the restatement do not exist."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import camera_ref as cr
import features_ref as ft
import history_ref as hr
import materials_ref as mr

F, D = np.float32, np.float64
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
NAMES = ["apt_film_history_default_host", "apt_film_history_device", "apt_film_history_host", "apt_film_history_export_device",
         "apt_film_history_export_host", "apt_film_history_last_error"]
CASES = ("same", "translate", "rotate", "behind")


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
    scalars = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
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
    """A fourth library with a header of its own: the binding's table is that header's, entry by entry and in its order, the library
    exports those names and nothing else, and the other three libraries and their headers know none of them and export what they did."""
    from ascendpathtracing_amd._lib import ApFilmHistory
    L = apt._lib.history_lib()
    assert ctypes.sizeof(ApFilmHistory) == 24 and ApFilmHistory.tol_plane.offset == 12 and ApFilmHistory.min_weight.offset == 20
    header = _header_prototypes("render_mi355x_history.h")
    assert list(header) == NAMES
    table = apt._lib.HISTORY_PROTOTYPES
    assert list(table) == list(header)
    for name, proto in header.items():
        assert (table[name][0], list(table[name][1])) == proto, name
        fn = getattr(L, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == list(table[name][1]), name
    assert _exports(apt._lib.HISTORY_LIB_PATH) == set(header)
    new = set(header) | {"apt_film_history"}
    others = set(apt._lib.ABI_SYMBOLS) | set(apt._lib.DENOISE_PROTOTYPES) | set(apt._lib.ADAPTIVE_PROTOTYPES)
    assert not new & others
    assert _exports(apt._lib.LIB_PATH) == set(apt._lib.PROTOTYPES)
    assert _exports(apt._lib.DENOISE_LIB_PATH) == set(apt._lib.DENOISE_PROTOTYPES) == set(_header_prototypes("render_mi355x_denoise.h"))
    assert _exports(apt._lib.ADAPTIVE_LIB_PATH) == set(apt._lib.ADAPTIVE_PROTOTYPES) == set(_header_prototypes("render_mi355x_adaptive.h"))
    for h in ("render_mi355x.h", "render_mi355x_denoise.h", "render_mi355x_adaptive.h"):
        assert not re.search(r"\b(%s)\b" % "|".join(sorted(new)), open(os.path.join(mr.ROOT, "include", h)).read()), h
    assert apt._lib.lib().apt_abi_version() == 3
    r = apt._lib.film_history_record()
    assert (r.struct_size, r.max_history, r.reserved) == (24, 32, 0)
    assert (r.tol_plane, r.tol_normal, r.min_weight) == (F(0.01), F(0.9), F(2.0 ** -10))
    assert L.apt_film_history_default_host(None) == APT_ERR_ARG and b"null" in L.apt_film_history_last_error()
    assert L.apt_film_history_default_host(ctypes.byref(r)) == 0 and L.apt_film_history_last_error() == b""
    assert apt._lib.film_history_record(max_history=4, tol_plane=0.5).max_history == 4
    with pytest.raises(apt.AptError):
        apt._lib.film_history_record(sigma=1.0)
    for name in ("film_history", "film_history_export", "History"):
        assert hasattr(apt.render, name)
    for name in ("push", "radiance", "length", "denoise_inputs", "reset"):
        assert hasattr(apt.render.History, name)
    # (build_id() hashes public_headers(): tests/test_film_stage_cpu.py holds it to the hand-written list)
    assert os.path.join(mr.ROOT, "include", "render_mi355x_history.h") in apt._lib.public_headers()


# ---- the twins against the restatement ----------------------------------------------------------------------------------------------------
def _twin_equals(apt, rec, args, W, H):
    want, valid, wt = hr.reproject(rec, *args, W, H, detail=True)
    rc, got, intact, _ = hr.history_host(apt, rec, *args, W, H)
    assert rc == 0 and intact
    hr.assert_same(got, want)
    return want, valid


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("shape", hr.SIZES, ids=lambda s: "%dx%d" % s)
def test_twin_equals_the_restatement(apt, shape, name):
    """Synthetic planes of a slanted wall (cov = 0 pixels among them), a history with lengths from below 1 to beyond the clamp."""
    W, H = shape
    args = hr.case(W, H, name)
    hist = args[5]
    for mh in (1, 2, 32):
        want, valid = _twin_equals(apt, hr.record(apt, max_history=mh), args, W, H)
        assert (want[5] >= 1).all() and (want[5] <= mh).all()
        if mh == 1:                                                   # alpha = 1: the current frame, up to H + (new - H)'s two roundings
            assert np.abs(want[:3] - args[2]).max() <= 2 * 2.0 ** -24 * 4  # (values below 2: |new - H| and |out| below 4)
    if name == "behind":
        assert not valid.any()
    if shape == (33, 17):
        assert (hist[5] < 1).any() and (hist[5] > 32).any() and (hist[5] == 1).any()
        if name in ("same", "translate"):
            assert valid.sum() > W * H // 2 and not valid.all()
            assert (want[5] == 32).any() and (want[5] == 2).any() and ((want[5] > 2) & (want[5] < 32)).any()
        if name == "rotate":                                          # part of the image lies outside the previous frame
            columns = valid.reshape(W, H).sum(1)
            assert (columns == 0).sum() >= 3 and (columns > H // 2).sum() >= 3
            # the lengths below 1 are rejected: with them raised to 1 other pixels come out
            raised = hist.copy()
            raised[5] = np.maximum(raised[5], 1)
            assert hr.bits_differ(hr.reproject(hr.DEFAULTS, *args[:5], raised, W, H), hr.reproject(hr.DEFAULTS, *args, W, H))
        cov = args[3][0]
        assert (cov == 0).any() and not valid[cov == 0].any()


@pytest.mark.parametrize("shape", [(5, 3), (33, 17)], ids=lambda s: "%dx%d" % s)
def test_first_frame_and_nan_in_each_input(apt, shape):
    W, H = shape
    N = W * H
    cc, pc, cur, cf, pf, hist = hr.case(W, H, "translate")
    rec = hr.record(apt)
    # the first frame: prev_hist NULL, prev_features and prev_cam not read
    rc, got, intact, _ = hr.history_host(apt, rec, cc, None, cur, cf, None, None, W, H)
    assert rc == 0 and intact
    hr.assert_same(got, hr.reproject(rec, cc, None, cur, cf, None, None, W, H))
    hr.assert_same(got[:3], cur)
    assert (got[5] == 1).all()
    clean = hr.reproject(rec, cc, pc, cur, cf, pf, hist, W, H)
    for which in range(4):
        arrays = [cur.copy(), cf.copy(), pf.copy(), hist.copy()]
        a = arrays[which]
        for p in range(a.shape[0]):
            a[p, (3 + 5 * p) % N] = np.nan
        args = (cc, pc, arrays[0], arrays[1], arrays[2], arrays[3])
        want, _ = _twin_equals(apt, rec, args, W, H)
        assert hr.bits_differ(want, clean)
        if which in (1, 2):                                           # a NaN guide rejects taps: it never reaches the output
            assert not np.isnan(want).any()
        else:
            assert np.isnan(want).any()


@pytest.fixture(scope="module")
def open_scene(apt):
    """gen_spheres_open at 48 x 32 from the two eyes: the camera records (the library's own build), their features_ref planes."""
    W, H = 48, 32
    sph, _ = apt.gen_data.gen_spheres_open()
    cams = [apt.gen_data.camera(width=W, height=H, eye=e, target=hr.TARGET, up=hr.UP, vfov_deg=hr.VFOV, offset=0.0) for e in (hr.EYE, hr.EYE2)]
    recs = [cr.from_ctypes(c) for c in cams]
    planes = [ft.planes(r, W, H, 1, 3, sph, 8, 1e-4) for r in recs]
    return W, H, sph, cams, recs, planes


def test_twin_equals_the_restatement_on_real_planes(apt, open_scene):
    W, H, _, cams, recs, planes = open_scene
    hist, cur = hr.synthetic_history(W, H, 9)
    for a, b in ((0, 1), (1, 0), (0, 0)):
        want, valid = _twin_equals(apt, hr.record(apt), (cams[a], cams[b], cur, planes[a], planes[b], hist), W, H)
        hr.assert_same(want, hr.reproject(hr.DEFAULTS, recs[a], recs[b], cur, planes[a], planes[b], hist, W, H))
        assert valid.sum() > W * H // 4


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1001])
def test_export_twin_equals_the_restatement(apt, n):
    hist = hr.export_case(n)
    rc, film, mom = hr.export_host(apt, hist)
    assert rc == 0
    wf, wm = hr.export(hist)
    hr.assert_same(film, wf)
    hr.assert_same(mom, wm)
    # what the denoiser's prepare makes of it with passes = 2: the mean exactly, and var up to one add and one subtract
    ok = ~np.isnan(hist[4]) & ~np.isnan(hist[5])
    assert np.array_equal((film / F(2))[:, ok], hist[:3][:, ok]) and np.array_equal((mom[0] / F(2))[ok], hist[3][ok])
    lm, q, h = hist[3].astype(D), hist[4].astype(D), hist[5].astype(D)
    var = np.where(h - 1 >= 1, np.maximum(q - lm * lm, 0) / np.where(h - 1 >= 1, h - 1, 1), q)
    lm_d = mom[0] / F(2)
    got = np.maximum(mom[1] / F(2) - lm_d * lm_d, F(0))                # the prepare's v, / (passes - 1) = 1
    # lm * lm, q - lm * lm, the divide, lm * lm + var and the prepare's subtract: 5 roundings (8 allowed) of values <= q + lm^2 + var
    assert np.all(np.abs(got.astype(D) - var)[ok] <= 8 * 2.0 ** -24 * (q + lm * lm + var)[ok])
    assert n < 6 or ((hist[5] == 1).any() and (hist[5] > 2).any())


def test_refusals_leave_the_outputs_untouched(apt):
    L = apt._lib.history_lib()
    W, H = 5, 3
    N = W * H
    cc, pc, cur, cf, pf, hist = hr.case(W, H, "translate")
    good = hr.record(apt)

    def rec(**kw):
        r = hr.record(apt)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def cam(base, **kw):
        c = hr.ctypes_camera(apt, base)
        for k, v in kw.items():
            setattr(c, k, (ctypes.c_double * 3)(*v) if isinstance(v, tuple) else v)
        return c

    nan, inf = float("nan"), float("inf")
    bad_recs = [(rec(struct_size=20), APT_ERR_STRUCT), (rec(max_history=0), APT_ERR_ARG), (rec(max_history=(1 << 24) + 1), APT_ERR_ARG),
                (rec(tol_plane=-0.5), APT_ERR_ARG), (rec(tol_plane=nan), APT_ERR_ARG), (rec(tol_normal=inf), APT_ERR_ARG),
                (rec(min_weight=0.0), APT_ERR_ARG), (rec(min_weight=1.5), APT_ERR_ARG), (rec(min_weight=nan), APT_ERR_ARG)]
    for r, code in bad_recs:
        rc, _, intact, untouched = hr.history_host(apt, r, cc, pc, cur, cf, pf, hist, W, H)
        assert rc == code and intact and untouched and L.apt_film_history_last_error() != b""
    bad_cams = [(cam(cc, struct_size=180), APT_ERR_STRUCT), (cam(cc, pos=(nan, 0.0, 0.0)), APT_ERR_ARG), (cam(cc, g=(0.0, 0.0, 0.0)), APT_ERR_ARG),
                (cam(cc, cx=(inf, 0.0, 0.0)), APT_ERR_ARG), (cam(cc, cy=(0.0, 0.0, 0.0)), APT_ERR_ARG), (cam(cc, offset=nan), APT_ERR_ARG)]
    for c, code in bad_cams:
        for args in ((c, pc), (cc, c)):
            rc, _, intact, untouched = hr.history_host(apt, good, args[0], args[1], cur, cf, pf, hist, W, H)
            assert rc == code and intact and untouched
    # (a bad previous camera is not read on the first frame)
    assert hr.history_host(apt, good, cc, bad_cams[1][0], cur, cf, None, None, W, H)[0] == 0

    p = hr.ptr
    out = np.full((6, N), np.nan, dtype=F)
    c1, c2 = hr.ctypes_camera(apt, cc), hr.ctypes_camera(apt, pc)
    args = [ctypes.byref(good), ctypes.byref(c1), ctypes.byref(c2), p(cur), p(cf), p(pf), p(hist), W, H, p(out)]
    for i in (0, 1, 2, 3, 4, 5, 9):                                     # (6 alone is the first-frame form)
        a = list(args)
        a[i] = None
        assert L.apt_film_history_host(*a) == APT_ERR_ARG, i
    for i, v in ((7, 0), (8, 0)):
        a = list(args)
        a[i] = v
        assert L.apt_film_history_host(*a) == APT_ERR_ARG
    a = list(args)
    a[7], a[8] = 1 << 15, (1 << 13) + 1                                # N > 2^28
    assert L.apt_film_history_host(*a) == APT_ERR_ARG
    a = list(args)
    a[9] = a[6]                                                        # out_hist == prev_hist
    before = hist.copy()
    assert L.apt_film_history_host(*a) == APT_ERR_ARG and not hr.bits_differ(hist, before)
    assert np.isnan(out).all()
    assert L.apt_film_history_host(*args) == 0 and L.apt_film_history_last_error() == b"" and not np.isnan(out[5]).any()

    film, mom = np.full((3, N), -7.0, dtype=F), np.full((2, N), -7.0, dtype=F)
    for a in ([None, N, p(film), p(mom)], [p(hist), N, None, p(mom)], [p(hist), N, p(film), None], [p(hist), 0, p(film), p(mom)],
              [p(hist), (1 << 28) + 1, p(film), p(mom)]):
        assert L.apt_film_history_export_host(*a) == APT_ERR_ARG
    assert np.all(film == F(-7)) and np.all(mom == F(-7))


# ---- the same camera: the running mean ---------------------------------------------------------------------------------------------------
def test_same_camera_gives_the_running_mean(apt):
    """K frames pushed from one camera onto a fully covered wall: every pixel's history is the mean of the K frames.

    The tolerance, from the contract.  Under an unmoved camera u = x up to the float64 geometry's rounding: some 50 operations of
    relative error 2^-53 on coordinates a few hundred units large against a pixel footprint of about a unit, so |u - x| < 2^-40 * W:
    the fp32 weights are (1, 0, 0, 0) up to e = 2^-34 (either x0 = x with fx <= e or x0 = x - 1 with fx >= 1 - e).  One push then
    computes H = S / W with S, W sums of four terms of which three are <= e * M (M = 2: the values lie in [0, 2)): at most 4 products,
    3 + 3 adds and a divide, then hl likewise, t, alpha (3 more) and the blend's 3 operations: 20 roundings of relative 2^-24 on values
    <= M, plus 3 * e * M from the neighbours.  The blend is a convex combination, so the errors of earlier pushes are not amplified:
    after K pushes |out - mean| <= K * (20 * 2^-24 + 3 * 2^-34) * M."""
    W, H, K, M = 33, 17, 6, 2.0
    N = W * H
    cam = hr.look_at(hr.EYE, hr.TARGET, hr.UP, hr.VFOV, W, H)
    feat = hr.wall(cam, W, H, 4, cov0=False)
    rng = np.random.default_rng(8)
    frames = [(rng.random((3, N)) * M).astype(F) for _ in range(K)]
    rec = hr.record(apt, max_history=1 << 24)
    twin = ref = None
    for k, fr_ in enumerate(frames):
        prev = (None, None, None) if k == 0 else (cam, feat, twin)
        rc, twin, intact, _ = hr.history_host(apt, rec, cam, prev[0], fr_, feat, prev[1], prev[2], W, H)
        assert rc == 0 and intact
        ref = hr.reproject(rec, cam, prev[0], fr_, feat, prev[1], ref, W, H)
        hr.assert_same(twin, ref)
        mean = np.mean(np.stack(frames[:k + 1]).astype(D), axis=0)
        tol = (k + 1) * (20 * 2.0 ** -24 + 3 * 2.0 ** -34) * M
        assert np.abs(twin[:3].astype(D) - mean).max() <= tol, (k, np.abs(twin[:3].astype(D) - mean).max(), tol)
        assert np.abs(twin[5].astype(D) - (k + 1)).max() <= (k + 1) * 4 * 2.0 ** -24 * (k + 1)


# ---- physics: the default tolerances on the open scene, under a ray cast of the test's own ---------------------------------------------
def _cast(rec, W, H, sph, px, py):
    """float64 ray cast through image positions (px, py) in pixel units (pixel (x, y) spans [x, x + 1) x [y, y + 1)) -> (the index of
    the nearest sphere hit or -1, the hit points [3][n])."""
    s = np.asarray(sph, dtype=D)[:80].reshape(10, 8)
    shape, px, py = px.shape, px.ravel(), py.ravel()
    a, b = px / W - 0.5, py / H - 0.5
    d = np.stack([rec["cx"][k] * a + rec["cy"][k] * b + rec["g"][k] for k in range(3)])
    d /= np.linalg.norm(d, axis=0)
    o = np.asarray(rec["pos"], dtype=D)[:, None]
    best, which = np.full(px.shape, np.inf), np.full(px.shape, -1)
    for k in range(8):
        oc = o - s[1:4, k][:, None]
        bq = (oc * d).sum(0)
        disc = bq * bq - ((oc * oc).sum(0) - s[0, k])                    # row 0 holds the squared radius
        t = -bq - np.sqrt(np.where(disc > 0, disc, np.nan))
        hit = (disc > 0) & (t > 1e-6) & (t < best)
        best, which = np.where(hit, t, best), np.where(hit, k, which)
    return which.reshape(shape), (o + d * best).reshape((3,) + shape)


def _covered(rec, W, H, sph, grid=7):
    """-> int [W][H]: the sphere every ray of a grid over [x - 0.25, x + 1.25] x [y - 0.25, y + 1.25] hits, or -1."""
    X, Y = np.meshgrid(np.arange(W, dtype=D), np.arange(H, dtype=D), indexing="ij")
    offs = np.linspace(-0.25, 1.25, grid)
    first = None
    same = np.ones((W, H), dtype=bool)
    for ox in offs:
        for oy in offs:
            k, _ = _cast(rec, W, H, sph, X + ox, Y + oy)
            first = k if first is None else first
            same &= (k == first) & (k >= 0)
    return np.where(same, first, -1)


def test_default_tolerances_on_the_open_scene(apt, open_scene):
    """gen_spheres_open() at 48 x 32, the previous camera at (20, 60, 160), the current one at (50, 90, 130) (history_ref.EYE, EYE2), both
    looking at (70, 20, 60).  The previous frame's albedo planes serve as the history.  A current pixel that is itself covered by one
    sphere and whose four taps are each covered by that sphere must be valid and carry the sphere's albedo; one whose four taps are
    all covered by one other sphere must be reset.  "Covered" is decided by a float64 ray cast of the test's own.  The conditions
    asserted first -- at least half the image of the first kind, at least 30 pixels of the second -- hold with 852 and 38 pixels; from
    (60, 70, 140) the second kind has only 18 under this classification, which is why the second eye stands where it does.

    The albedo tolerance: the sphere's albedo a is exact in every plane (a mean of equal values), so H = (sum of w a) / (sum of w)
    and out = H + alpha * (a - H) differ from a by at most 4 products, 3 + 3 adds, a divide and the blend's 3: 14 roundings of 2^-24."""
    W, H, sph, cams, recs, planes = open_scene
    cur_rec, prev_rec = recs[1], recs[0]
    cur_f, prev_f = planes[1], planes[0]
    cov_cur, cov_prev = _covered(cur_rec, W, H, sph), _covered(prev_rec, W, H, sph)
    # the taps of each current pixel, by the test's own projection of the pixel centre's hit point
    X, Y = np.meshgrid(np.arange(W, dtype=D), np.arange(H, dtype=D), indexing="ij")
    _, P = _cast(cur_rec, W, H, sph, X + 0.5, Y + 0.5)
    wv = P - np.asarray(prev_rec["pos"], dtype=D)[:, None, None]
    proj = lambda axis: np.tensordot(np.asarray(prev_rec[axis], dtype=D), wv, 1) / np.dot(prev_rec[axis], prev_rec[axis])
    f = proj("g")
    u, v = (proj("cx") / f + 0.5) * W - 0.5, (proj("cy") / f + 0.5) * H - 0.5
    x0, y0 = np.floor(u), np.floor(v)
    # (pixels whose projection falls within 1e-6 of a pixel centre line could take other taps by rounding: none of either kind below)
    inside = (f > 0) & (x0 >= 0) & (x0 + 1 <= W - 1) & (y0 >= 0) & (y0 + 1 <= H - 1) & (cov_cur >= 0)
    xi, yi = np.where(inside, x0, 0).astype(int), np.where(inside, y0, 0).astype(int)
    taps = np.stack([cov_prev[xi + ex, yi + ey] for ex in (0, 1) for ey in (0, 1)])
    safe = (np.abs(u - np.round(u)) > 1e-6) & (np.abs(v - np.round(v)) > 1e-6)
    own = inside & safe & (taps == cov_cur[None]).all(0)
    other = inside & safe & (taps >= 0).all(0) & (taps == taps[0][None]).all(0) & (taps[0] != cov_cur)
    assert own.sum() >= W * H // 2 and other.sum() >= 30, (own.sum(), other.sum())

    alb = lambda p: p[ft.ALBEDO:ft.ALBEDO + 3]
    l = hr.lum(*alb(prev_f))
    hist = np.concatenate([alb(prev_f), l[None], (l * l)[None], np.full((1, W * H), 5, dtype=F)])
    cur = alb(cur_f).copy()
    for how in ("restatement", "twin"):
        if how == "twin":
            rc, out, intact, _ = hr.history_host(apt, hr.record(apt), cams[1], cams[0], cur, cur_f, prev_f, hist, W, H)
            assert rc == 0 and intact
        else:
            out = hr.reproject(hr.DEFAULTS, cur_rec, prev_rec, cur, cur_f, prev_f, hist, W, H)
        length = out[5].reshape(W, H)
        assert (length[own] > 1).all(), (how, (length[own] <= 1).sum())
        assert (length[other] == 1).all(), (how, (length[other] != 1).sum())
        table = np.asarray(sph, dtype=F)[:80].reshape(10, 8)[7:10]
        want = table[:, cov_cur[own]].astype(D)
        got = out[:3].reshape(3, W, H)[:, own].astype(D)
        assert np.all(np.abs(got - want) <= 14 * 2.0 ** -24 * want), how
        assert not hr.bits_differ(out[:3].reshape(3, W, H)[:, other], cur.reshape(3, W, H)[:, other])


# ---- three wrong implementations ---------------------------------------------------------------------------------------------------------
def test_three_wrong_implementations_change_the_result():
    """On the restatement: the current camera in place of the previous one, the plane test dropped, the taps summed in reverse."""
    W, H = 33, 17
    args = hr.case(W, H, "translate", jitter=0.03)
    right, valid, _ = hr.reproject(hr.DEFAULTS, *args, W, H, detail=True)
    assert valid.any() and not valid.all()
    for wrong in ("cur_camera", "no_plane", "reverse_taps"):
        out, v, _ = hr.reproject(hr.DEFAULTS, *args, W, H, wrong=wrong, detail=True)
        assert hr.bits_differ(out, right), wrong
        if wrong == "no_plane":
            assert v.sum() > valid.sum()
        if wrong == "reverse_taps":                                  # rounding alone: the same pixels are valid, values move by ulps
            assert np.array_equal(v, valid) and np.nanmax(np.abs(out - right)) < 1e-4
