"""CPU-only: guided film upscaling (libupscale_mi355x.so, include/render_mi355x_upscale.h) -- the binding against the header and the
exports, the CPU twins of the upscale and the patch bit for bit against the restatement tests/upscale_ref.py (out, resolved and every
word of work), NaN, infinite and negative values in each input, four closed forms with their rounding counts, the unresolved list
through the unchanged apt_film_select_host, every refusal, a cap on the unresolved share on the open 8-sphere scene, and, on the
restatement, that three wrong implementations are told from the right one.

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
import upscale_ref as ur

F, D, U32 = np.float32, np.float64, np.uint32
E = 2.0 ** -24                                   # one fp32 rounding, relative
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
NAMES = ["apt_film_upscale_default_host", "apt_film_upscale_work_floats", "apt_film_upscale_device", "apt_film_upscale_host",
         "apt_film_upscale_patch_device", "apt_film_upscale_patch_host", "apt_film_upscale_last_error"]
OTHERS = [("LIB_PATH", "PROTOTYPES", None), ("DENOISE_LIB_PATH", "DENOISE_PROTOTYPES", "render_mi355x_denoise.h"),
          ("ADAPTIVE_LIB_PATH", "ADAPTIVE_PROTOTYPES", "render_mi355x_adaptive.h"), ("HISTORY_LIB_PATH", "HISTORY_PROTOTYPES", "render_mi355x_history.h"),
          ("POST_LIB_PATH", "POST_PROTOTYPES", "render_mi355x_post.h"), ("METRICS_LIB_PATH", "METRICS_PROTOTYPES", "render_mi355x_metrics.h")]


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
    """A seventh library with a header of its own: the binding's table is that header's, entry by entry and in its order, the library
    exports those names and nothing else, and the other six libraries and their headers know none of them and export what they did."""
    from ascendpathtracing_amd._lib import ApFilmUpscale
    L = apt._lib.upscale_lib()
    assert ctypes.sizeof(ApFilmUpscale) == 32 and ApFilmUpscale.sigma_n.offset == 8 and ApFilmUpscale.min_weight.offset == 28
    header = _header_prototypes("render_mi355x_upscale.h")
    assert list(header) == NAMES
    table = apt._lib.UPSCALE_PROTOTYPES
    assert list(table) == list(header)
    for name, proto in header.items():
        assert (table[name][0], list(table[name][1])) == proto, name
        fn = getattr(L, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == list(table[name][1]), name
    assert _exports(apt._lib.UPSCALE_LIB_PATH) == set(header)
    new = set(header) | {"apt_film_upscale"}
    for path, protos, hname in OTHERS:
        names = set(getattr(apt._lib, protos))
        assert not new & names, protos
        assert _exports(getattr(apt._lib, path)) == names, path
        if hname is not None:
            assert names == set(_header_prototypes(hname)), hname
    for h in ["render_mi355x.h"] + [o[2] for o in OTHERS[1:]]:
        assert not re.search(r"\b(%s)\b" % "|".join(sorted(new)), open(os.path.join(mr.ROOT, "include", h)).read()), h
    assert apt._lib.lib().apt_abi_version() == 3
    r = apt._lib.film_upscale_record()
    assert (r.struct_size, r.reserved) == (32, 0)
    assert (r.sigma_n, r.sigma_z, r.sigma_c, r.sigma_a, r.albedo_floor, r.min_weight) == (32.0, 10.0, 8.0, 8.0, 1.0 / 32, 2.0 ** -6)
    d = apt._lib.film_denoise_record(2)                               # the denoiser's values, as the header says
    assert (r.sigma_n, r.sigma_z, r.sigma_c, r.sigma_a, r.albedo_floor) == (d.sigma_n, d.sigma_z, d.sigma_c, d.sigma_a, d.albedo_floor)
    assert {k: getattr(r, k) for k in ur.DEFAULTS} == {k: F(v) for k, v in ur.DEFAULTS.items()}
    assert L.apt_film_upscale_default_host(None) == APT_ERR_ARG and b"null" in L.apt_film_upscale_last_error()
    assert L.apt_film_upscale_default_host(ctypes.byref(r)) == 0 and L.apt_film_upscale_last_error() == b""
    assert L.apt_film_upscale_work_floats(7, 5) == 12 * 35 and L.apt_film_upscale_work_floats(1 << 14, 1 << 14) == 12 << 28
    assert apt._lib.film_upscale_record(sigma_n=4.0, min_weight=0.5).min_weight == 0.5
    with pytest.raises(apt.AptError):
        apt._lib.film_upscale_record(sigma_l=1.0)
    for name in ("film_upscale", "film_upscale_patch", "Upscaler"):
        assert hasattr(apt.render, name)
    for name in ("upscale", "unresolved", "refine"):
        assert hasattr(apt.render.Upscaler, name)
    # (build_id() hashes public_headers(): tests/test_film_stage_cpu.py holds it to the hand-written list)
    assert os.path.join(mr.ROOT, "include", "render_mi355x_upscale.h") in apt._lib.public_headers()


# ---- the twins against the restatement ----------------------------------------------------------------------------------------------------
def _twin_equals(apt, rec, lo, lf, lw, lh, hf, W, H):
    want = ur.upscale(rec, lo, lf, lw, lh, hf, W, H)
    rc, out, res, work, intact, _ = ur.upscale_host(apt, rec, lo, lf, lw, lh, hf, W, H)
    assert rc == 0 and intact
    ur.assert_same(out, want[0])
    assert res.dtype == U32 and np.array_equal(res, want[1])
    ur.assert_same(work, want[2])
    return want


def test_coordinates_are_float64():
    """The restatement's coordinates fail on a float32 intermediate, and are what exact arithmetic gives at a ratio of 2 and of 1."""
    x0, fx = ur.axis(np.arange(8), 4, 8)
    assert x0.dtype == D and fx.dtype == D
    assert np.array_equal(x0, [-1, 0, 0, 1, 1, 2, 2, 3]) and np.array_equal(fx, [.75, .25] * 4)
    x0, fx = ur.axis(np.arange(5), 5, 5)
    assert np.array_equal(x0, np.arange(5)) and not fx.any()
    with pytest.raises(AssertionError):
        hr.f64(np.zeros(3, dtype=F))


@pytest.mark.parametrize("size", ur.SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_twin_equals_the_restatement(apt, size):
    """Random flat patches with noisy coverage: resolved and unresolved pixels both occur at the sizes that have room for them."""
    lw, lh, W, H = size
    for seed in (0, 1):
        lo, lf, hf = ur.case(*size, seed=seed)
        for fields in ({}, dict(min_weight=1.0), dict(sigma_c=0.0, sigma_z=0.5, albedo_floor=0.5)):
            out, res, _ = _twin_equals(apt, ur.record(apt, **fields), lo, lf, lw, lh, hf, W, H)
            assert set(np.unique(res)) <= {0, 1}
        if size == (7, 5, 33, 17):
            out, res, _ = _twin_equals(apt, ur.record(apt), lo, lf, lw, lh, hf, W, H)
            assert 0.2 < res.mean() < 0.8
            # the unresolved list through the UNCHANGED select: exactly the pixels with resolved == 0, ascending
            lst = ur.unresolved_host(apt, res)
            assert lst.dtype == U32 and np.array_equal(lst, np.flatnonzero(res == 0))


@pytest.fixture(scope="module")
def open_scene(apt):
    """gen_spheres_open from history_ref.EYE at 48 x 32 / 24 x 16 and at 64 x 48 / 32 x 24: features_ref planes (samples 1, seed 3)."""
    sph, _ = apt.gen_data.gen_spheres_open()
    planes = {}
    for W, H in ((48, 32), (24, 16), (64, 48), (32, 24)):
        cam = apt.gen_data.camera(width=W, height=H, eye=hr.EYE, target=hr.TARGET, up=hr.UP, vfov_deg=hr.VFOV, offset=0.0)
        planes[W, H] = ft.planes(cr.from_ctypes(cam), W, H, 1, 3, sph, 8, 1e-4)
    return planes


def test_twin_equals_the_restatement_on_rendered_planes(apt, open_scene):
    lf, hf = open_scene[24, 16], open_scene[48, 32]
    lo = (np.random.default_rng(5).random((3, 24 * 16)) * 2).astype(F)
    out, res, _ = _twin_equals(apt, ur.record(apt), lo, lf, 24, 16, hf, 48, 32)
    assert 0 < (res == 0).sum() < 48 * 32 // 4 and np.isfinite(out).all()
    ur.assert_same(out, ur.upscale(ur.DEFAULTS, lo, lf, 24, 16, hf, 48, 32)[0])


def test_nan_inf_and_negative_in_each_input(apt):
    """A NaN, +inf and a negative value in every plane of every input in turn: the twin follows the restatement, NaN positions
    included.  A NaN guide closes its taps (g = 0 by the max) and never reaches out by itself."""
    size = lw, lh, W, H = (7, 5, 33, 17)
    lo, lf, hf = ur.case(*size, seed=2)
    rec = ur.record(apt)
    clean = ur.upscale(rec, lo, lf, lw, lh, hf, W, H)[0]
    for value in (np.nan, np.inf, -1.5):
        for which in range(3):
            arrays = [lo.copy(), lf.copy(), hf.copy()]
            a = arrays[which]
            for p in range(a.shape[0]):
                a[p, (3 + 5 * p) % a.shape[1]] = value
            out, res, work = _twin_equals(apt, rec, arrays[0], arrays[1], lw, lh, arrays[2], W, H)
            assert ur.bits_differ(out, clean), (value, which)
            if which == 0 and value != -1.5:
                assert not np.isfinite(out).all()


def _halves(lw, lh, W, H, i_left=1.0, i_right=3.0):
    """Closed form (b): two half-images with orthogonal normals, albedo 0.5, coverage 1, one depth; illumination i_left / i_right."""
    def planes(w, h):
        f = np.zeros((ur.PLANES, w * h), dtype=F)
        left = (np.arange(w * h) // h) < w // 2
        f[ur.COVERAGE], f[ur.DEPTH] = 1, 100
        f[ur.NORMAL], f[ur.NORMAL + 1] = left, ~left
        f[ur.ALBEDO:ur.ALBEDO + 3] = 0.5
        return f, left
    lf, l_left = planes(lw, lh)
    hf, h_left = planes(W, H)
    lo = np.tile(np.where(l_left, F(0.5 * i_left), F(0.5 * i_right)).astype(F), (3, 1))
    return lo, lf, hf, l_left, h_left


def test_nan_under_a_zero_weight_tap_stays_out(apt):
    """A NaN illumination in the low pixels of the right half: every full pixel of the left half has taps there, all with g = 0
    exactly (x_n = 32), and none of them may meet the NaN -- a product w * i with w = 0 would be NaN."""
    lw, lh, W, H = 8, 6, 16, 12
    lo, lf, hf, l_left, h_left = _halves(lw, lh, W, H)
    lo[:, ~l_left] = np.nan
    out, res, _ = _twin_equals(apt, ur.record(apt), lo, lf, lw, lh, hf, W, H)
    assert res.all()
    assert np.all(out[:, h_left] == F(0.5)) and np.isnan(out[:, ~h_left]).all()
    boundary = h_left & ((np.arange(W * H) // H) == W // 2 - 1)       # these pixels do have taps in the NaN half
    x0, fx = ur.axis(np.arange(W * H) // H, lw, W)
    assert np.all(x0[boundary] + 1 == lw // 2) and np.all(fx[boundary] > 0)


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def test_closed_form_a_constant_illumination(apt, open_scene):
    """(a) lo = A_q * c gives out = A_p * c at EVERY pixel, resolved or not, on the rendered planes.

    Roundings, all relative 2^-24 on positive terms (weights, illuminations and albedos are positive, so nothing cancels): lo = A_q * c
    (1), i_q = lo / A_q (1): every i_q is c within 2.  A sum S = sum of w * i over up to four taps: a product (1) and up to 3 adds
    (the first onto 0 is exact) per term: 4; W: 3 adds; the divide 1; out = i_p * A_p: 1.  2 + 4 + 3 + 1 + 1 = 11; 12 allowed."""
    lf, hf = open_scene[24, 16], open_scene[48, 32]
    c = F(0.7)
    A_q = np.stack(ur.albedo_of(lf, ur.DEFAULTS["albedo_floor"]))
    A_p = np.stack(ur.albedo_of(hf, ur.DEFAULTS["albedo_floor"])).astype(D)
    lo = (A_q * c).astype(F)
    out, res, _ = _twin_equals(apt, ur.record(apt), lo, lf, 24, 16, hf, 48, 32)
    want = A_p * D(c)
    assert (res == 0).any() and (res == 1).any()
    assert np.all(np.abs(out.astype(D) - want) <= 12 * E * want)
    # the low-res albedo multiplied back instead (a wrong implementation) blurs every albedo edge: it misses this bound by far
    bad = ur.upscale(ur.DEFAULTS, lo, lf, 24, 16, hf, 48, 32, wrong="lo_albedo")[0]
    assert (np.abs(bad.astype(D) - want) > 1000 * E * want).sum() > 50


def test_closed_form_b_two_halves(apt):
    """(b) Two half-images with orthogonal normals and illuminations 1 and 3: a tap of the other side has x_n = 32 * max(1 - 0, 0) = 32,
    t = max(1 - 4, 0) = 0, g = 0 exactly, so every pixel gets its own side's value where plain bilinear interpolation blends.

    Roundings: albedo 0.5 makes lo, i_q = lo / 0.5 and out = i_p * 0.5 exact.  Left (i = 1): w * 1 = w, so S and W are the same sums
    and S / W = 1 exactly.  Right (i = 3): a product and up to 3 adds a term (4), W's 3 adds, the divide: 8."""
    lw, lh, W, H = 8, 6, 16, 12
    lo, lf, hf, _, h_left = _halves(lw, lh, W, H)
    out, res, _ = _twin_equals(apt, ur.record(apt), lo, lf, lw, lh, hf, W, H)
    assert res.all()
    assert np.all(out[:, h_left] == F(0.5))
    assert np.all(np.abs(out[:, ~h_left].astype(D) - 1.5) <= 8 * E * 1.5)
    # g dropped (a wrong implementation): the columns beside the edge blend
    bad = ur.upscale(ur.DEFAULTS, lo, lf, lw, lh, hf, W, H, wrong="no_g")[0]
    blended = (np.abs(bad[0].astype(D) - np.where(h_left, 0.5, 1.5)) > 0.1)
    assert blended.sum() == 2 * H and np.all(np.isin(np.flatnonzero(blended) // H, (W // 2 - 1, W // 2)))


def test_closed_form_c_a_block_of_coverage(apt):
    """(c) A block of full coverage over a low image of coverage 0: x_c = 8 * |1 - 0| = 8 alone gives t = max(1 - 8 * 0.125, 0) = 0,
    g = 0 for every tap of a block pixel: exactly the block is unresolved.  Elsewhere all planes are 0 at both sizes: x = 0, g = 1."""
    lw, lh, W, H = 6, 5, 12, 10
    lf = np.zeros((ur.PLANES, lw * lh), dtype=F)
    hf = np.zeros((ur.PLANES, W * H), dtype=F)
    idx = np.arange(W * H)
    block = ((idx // H >= 3) & (idx // H < 7)) & ((idx % H >= 2) & (idx % H < 9))
    hf[ur.COVERAGE, block], hf[ur.DEPTH, block], hf[ur.NORMAL + 2, block] = 1, 80, 1
    hf[ur.ALBEDO:ur.ALBEDO + 3, block] = 0.25
    lo = np.full((3, lw * lh), 2.0, dtype=F)
    for fields in ({}, dict(sigma_n=0.0, sigma_z=0.0, sigma_a=0.0)):                   # the second: x_c alone
        out, res, _ = _twin_equals(apt, ur.record(apt, **fields), lo, lf, lw, lh, hf, W, H)
        assert np.array_equal(res == 0, block)
        assert np.all(out[:, ~block] == F(2.0))                       # A = 1 on both sides, equal values: S = 2 W exactly
        assert np.all(np.abs(out[:, block].astype(D) - 0.5) <= 8 * E)  # the fallback: illumination 2 (up to (b)'s 8), times A_p = 0.25
        assert np.array_equal(ur.unresolved_host(apt, res), np.flatnonzero(block))


def test_closed_form_d_equal_sizes(apt):
    """(d) Equal sizes with equal features return lo: u = ((x + 0.5) * w) / w - 0.5 = x exactly, so the first tap is the pixel itself
    with b = 1 and the other three have b = 0 and never enter.  Roundings: i = lo / A (1); guided: w = g, S = w * i (1), S / W (1) --
    or the fallback with w = 1: none --; out = i_p * A (1): at most 4, relative to lo."""
    for size in ((5, 3, 5, 3), (8, 8, 8, 8), (33, 17, 33, 17)):
        lw, lh, W, H = size
        lo, lf, hf = ur.case(*size, seed=4)
        assert not ur.bits_differ(lf, hf)
        out, res, work = _twin_equals(apt, ur.record(apt), lo, lf, lw, lh, hf, W, H)
        assert np.all(np.abs(out.astype(D) - lo.astype(D)) <= 4 * E * lo.astype(D))
        assert np.all(work[2, :, 3] == 0) and not ur.bits_differ(work[0, :, 3], lf[ur.COVERAGE])


# ---- the patch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 1001])
def test_patch_twin_equals_the_restatement(apt, count):
    n = 1500
    rng = np.random.default_rng(count)
    out = (rng.random((3, n)) * 2).astype(F)
    lst = rng.permutation(n)[:count].astype(U32)
    if count >= 63:
        lst[5], lst[count - 1] = n, 0xFFFFFFFF                        # entries beyond the image are skipped
    sums = (rng.random((3, count)) * 8).astype(F)
    for passes in (1, 3, 4):
        rc, got, intact = ur.patch_host(apt, sums, lst, passes, out)
        assert rc == 0 and intact and apt._lib.upscale_lib().apt_film_upscale_last_error() == b""
        want = ur.patch(sums, lst, passes, out)
        ur.assert_same(got, want)
        inside = lst[lst < n]
        rest = np.setdiff1d(np.arange(n), inside)
        assert not ur.bits_differ(got[:, rest], out[:, rest])
        if count:
            assert np.array_equal(got[:, inside], (sums[:, lst < n] / F(passes)).astype(F))


# ---- three wrong implementations ---------------------------------------------------------------------------------------------------------
def test_three_wrong_implementations_are_told_apart():
    """On the restatement: the taps summed in reverse change its bits (rounding alone: the same pixels resolve, values move by ulps);
    the low-res albedo multiplied back fails closed form (a) and g dropped fails closed form (b): asserted in those tests."""
    size = lw, lh, W, H = (7, 5, 33, 17)
    lo, lf, hf = ur.case(*size, seed=0)
    right = ur.upscale(ur.DEFAULTS, lo, lf, lw, lh, hf, W, H)
    for wrong in ("reverse_taps", "lo_albedo", "no_g"):
        out, res, work = ur.upscale(ur.DEFAULTS, lo, lf, lw, lh, hf, W, H, wrong=wrong)
        assert ur.bits_differ(out, right[0]), wrong
        assert not ur.bits_differ(work, right[2])
        if wrong == "reverse_taps":
            assert np.array_equal(res, right[1]) and np.abs(out - right[0]).max() < 1e-4
        if wrong == "no_g":
            assert res.all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(apt):
    L = apt._lib.upscale_lib()
    size = lw, lh, W, H = (3, 2, 5, 3)
    N, nl = W * H, lw * lh
    lo, lf, hf = ur.case(*size)

    def rec(**kw):
        r = ur.record(apt)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    nan, inf = float("nan"), float("inf")
    bad = [(rec(struct_size=28), APT_ERR_STRUCT), (rec(min_weight=0.0), APT_ERR_ARG), (rec(min_weight=1.5), APT_ERR_ARG),
           (rec(min_weight=nan), APT_ERR_ARG), (rec(albedo_floor=0.0), APT_ERR_ARG), (rec(albedo_floor=inf), APT_ERR_ARG),
           (rec(albedo_floor=nan), APT_ERR_ARG)]
    for s in ("sigma_n", "sigma_z", "sigma_c", "sigma_a"):
        bad += [(rec(**{s: -1.0}), APT_ERR_ARG), (rec(**{s: nan}), APT_ERR_ARG), (rec(**{s: inf}), APT_ERR_ARG)]
    for r, code in bad:
        rc, _, _, _, intact, untouched = ur.upscale_host(apt, r, lo, lf, lw, lh, hf, W, H)
        assert rc == code and intact and untouched and L.apt_film_upscale_last_error() != b""

    good = rec()
    out, res = np.full((3, N), nan, dtype=F), np.full(N, 7, dtype=U32)
    raw = np.full(12 * nl + 8, -3.5, dtype=F)
    off = (-raw.ctypes.data // 4) % 4
    work = raw[off:off + 12 * nl]
    p = ur.ptr
    args = [ctypes.byref(good), p(lo), p(lf), lw, lh, p(hf), W, H, p(work), p(out), p(res)]
    for i in (0, 1, 2, 5, 8, 9, 10):
        a = list(args)
        a[i] = None
        assert L.apt_film_upscale_host(*a) == APT_ERR_ARG, i
    for sizes in ((0, lh, W, H), (lw, 0, W, H), (lw, lh, 0, H), (lw, lh, W, 0), (W + 1, lh, W, H), (lw, H + 1, W, H),
                  (1, 1, 1 << 15, (1 << 13) + 1)):                    # a zero size, a low size above the full one, N > 2^28
        a = list(args)
        a[3], a[4], a[6], a[7] = sizes
        assert L.apt_film_upscale_host(*a) == APT_ERR_ARG, sizes
    a = list(args)
    a[8] = ctypes.c_void_p(work.ctypes.data + 4)                       # a work that is not 16-byte aligned
    assert L.apt_film_upscale_host(*a) == APT_ERR_ARG and b"aligned" in L.apt_film_upscale_last_error()
    before = [lo.copy(), lf.copy(), hf.copy()]
    for i, j in ((9, 1), (9, 2), (9, 5), (10, 1), (10, 5), (8, 2), (8, 5), (9, 8), (10, 8), (10, 9)):
        a = list(args)
        a[i] = a[j]                                                    # an output that is an input, or two outputs that are one
        assert L.apt_film_upscale_host(*a) == APT_ERR_ARG, (i, j)
    assert not any(ur.bits_differ(x, y) for x, y in zip((lo, lf, hf), before))
    assert np.isnan(out).all() and np.all(res == 7) and np.all(raw == F(-3.5))
    assert L.apt_film_upscale_host(*args) == 0 and L.apt_film_upscale_last_error() == b"" and not np.isnan(out).any()

    # the patch
    sums, lst, img = np.ones((3, 4), dtype=F), np.arange(4, dtype=U32), np.full((3, N), -7.0, dtype=F)
    for a in ([None, p(lst), 4, 1, N, p(img)], [p(sums), None, 4, 1, N, p(img)], [p(sums), p(lst), 4, 1, N, None],
              [p(sums), p(lst), 4, 0, N, p(img)], [p(sums), p(lst), 4, (1 << 24) + 1, N, p(img)], [p(sums), p(lst), 4, 1, 0, p(img)],
              [p(sums), p(lst), 4, 1, (1 << 28) + 1, p(img)], [p(sums), p(lst), (1 << 28) + 1, 1, N, p(img)], [p(img), p(lst), 4, 1, N, p(img)]):
        assert L.apt_film_upscale_patch_host(*a) == APT_ERR_ARG and L.apt_film_upscale_last_error() != b""
    assert np.all(img == F(-7))
    assert L.apt_film_upscale_patch_host(p(sums), p(lst), 0, 1, N, p(img)) == 0 and np.all(img == F(-7))     # list_count = 0 is accepted


# ---- a cap on the unresolved share ---------------------------------------------------------------------------------------------------------
def test_unresolved_share_on_the_open_scene(apt, open_scene):
    """A refine step must not hide a reconstruction that resolves nothing: on gen_spheres_open() at 64 x 48 from 32 x 24 (features at
    samples 1, seed 3, from history_ref.EYE) at most 0.15 of the pixels may be unresolved at the defaults."""
    lf, hf = open_scene[32, 24], open_scene[64, 48]
    lo = np.ones((3, 32 * 24), dtype=F)
    rc, out, res, _, intact, _ = ur.upscale_host(apt, ur.record(apt), lo, lf, 32, 24, hf, 64, 48)
    assert rc == 0 and intact
    assert np.array_equal(res, ur.upscale(ur.DEFAULTS, lo, lf, 32, 24, hf, 64, 48)[1])
    share = float((res == 0).mean())
    print("unresolved share at 64 x 48 from 32 x 24: %.4f" % share)
    assert 0 < share <= 0.15, share
