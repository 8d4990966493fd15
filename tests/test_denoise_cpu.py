"""CPU-only: the film's moments and its filter (libdenoise_mi355x.so, include/render_mi355x_denoise.h) -- the CPU twins apt_film_accumulate_host and
apt_film_denoise_host bit for bit against the restatement tests/denoise_ref.py, the moments' film against film_ref.accumulate, properties of
the contract with bounds counted from its operations, the filter's gain against a converged restatement, and every refusal.

Without the feature nothing here passes: the entries, the record and the restatement do not exist."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import camera_ref as cr
import denoise_ref as dr
import features_ref as ft
import film_ref as fr
import materials_ref as mr

F, D = np.float32, np.float64
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
U = 2.0 ** -24                                                                    # unit roundoff of float32: |fl(x) - x| <= U |x|


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data, render
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def _oparams(**kw):
    from oracle import oracle
    return oracle.make_params(**kw)


def _rec(apt, passes, iterations=None, **kw):
    return apt._lib.film_denoise_record(passes, iterations, **kw)


def _room(apt):
    """The diffuse closed room with smallpt's lamp: the scene the NumPy prototype of DESIGN "Feature planes" used."""
    sph = apt.gen_data.with_lamp(apt.gen_data.gen_spheres(), 8, 7)
    return sph, np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)


def _room_passes(apt, w, h, s, K, depth=4, seed=5):
    sph, mat = _room(apt)
    p = _oparams(width=w, height=h, samples=s, depth=depth, num_spheres=8, light_index=7, seed=seed, flags=apt.APT_FLAG_NEE)
    passes = [fr.render_pass(p, sph, mat, pass_index=k)[0] for k in range(K)]
    feat = ft.planes(cr.default_record(w, h), w, h, s, seed, sph, 8, 1e-4)
    return p, sph, mat, passes, feat


def _header_prototypes():
    """include/render_mi355x_denoise.h -> {name: (restype, [argtypes])} in the header's order, by the binding's type rules."""
    scalars = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(mr.ROOT, "include", "render_mi355x_denoise.h")).read(), flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    found = {}
    for statement in text.split(";"):
        m = re.fullmatch(r"\s*([\w\s*]+?)\s*\b(apt_[a-z0-9_]+)\s*\(([^()]*)\)\s*", statement)
        if m is None:
            continue
        ret, name, params = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        args = [] if params == "void" else [ctypes.c_void_p if "*" in a else scalars[[w for w in a.split() if w != "const"][0]]
                                            for a in params.split(",")]
        assert name not in found
        found[name] = (ctypes.c_char_p if ret == "const char *" else scalars[ret], args)
    return found


def test_symbols_record_and_defaults(apt):
    """The denoiser is a library and a header of its own: the binding's table is that header's, entry by entry and in its order, the
    library exports those names and nothing else, and librender_mi355x.so and its header know none of them."""
    from ascendpathtracing_amd._lib import ApFilmDenoise
    L = apt._lib.denoise_lib()
    assert ctypes.sizeof(ApFilmDenoise) == 40 and ApFilmDenoise.sigma_n.offset == 16 and ApFilmDenoise.albedo_floor.offset == 36
    header = _header_prototypes()
    assert list(header) == ["apt_film_accumulate_device", "apt_film_accumulate_host", "apt_film_denoise_default_host", "apt_film_denoise_work_floats",
                            "apt_film_denoise_device", "apt_film_denoise_host", "apt_film_denoise_last_error"]
    table = apt._lib.DENOISE_PROTOTYPES
    assert list(table) == list(header)
    for name, proto in header.items():
        assert (table[name][0], list(table[name][1])) == proto, name
        fn = getattr(L, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == list(table[name][1]), name
    out = subprocess.run(["nm", "-D", "--defined-only", apt._lib.DENOISE_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == set(header)
    assert not set(header) & set(apt._lib.ABI_SYMBOLS) and "apt_film_denoise" not in open(mr.ROOT + "/include/render_mi355x.h").read()
    assert apt._lib.lib().apt_abi_version() == 3
    r = _rec(apt, 7)
    assert (r.struct_size, r.passes, r.iterations, r.reserved) == (40, 7, 5, 0) and r.albedo_floor == 1 / 32
    assert all(np.isfinite(getattr(r, k)) and getattr(r, k) >= 0 for k in dr.SIGMAS)
    assert L.apt_film_denoise_default_host(None, 3) == APT_ERR_ARG and b"null" in L.apt_film_denoise_last_error()
    assert L.apt_film_denoise_default_host(ctypes.byref(r), 3) == 0 and L.apt_film_denoise_last_error() == b""
    assert L.apt_film_denoise_work_floats(1920, 1080) == 16 * 1920 * 1080 and L.apt_film_denoise_work_floats(65536, 65536) == 16 << 32
    assert _rec(apt, 4, 2, sigma_l=1.5).sigma_l == 1.5 and _rec(apt, 4, 2).iterations == 2
    with pytest.raises(apt.AptError):
        _rec(apt, 4, sigma_q=1.0)
    assert hasattr(apt.render, "film_accumulate") and hasattr(apt.render, "film_denoise") and hasattr(apt.render.Film, "denoise")


# ---- the twins against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape", dr.SHAPES, ids=lambda s: "%dx%d" % s)
def test_twins_equal_the_restatement(apt, shape, nan):
    """Accumulate and denoise, bit for bit with NaN positions included.  The finite inputs hold every value to its bits; with the NaN
    -- one pass value -- a zero weight times NaN is NaN, so it spreads over each iteration's footprint, and so it must in both."""
    W, H = shape
    ps, feat = dr.synthetic(W, H, passes=3, nan=nan)
    film, mom = dr.accumulate(list(ps))
    got_film, got_mom = dr.accumulate_host(apt, list(ps))
    dr.assert_same(got_film, film)
    dr.assert_same(got_mom, mom)
    assert np.isnan(film).sum() == (1 if nan else 0)
    for it in (range(1, 6) if shape == (33, 17) else (5,)):
        rec = _rec(apt, 3, it)
        rc, out, work, guards = dr.denoise_host(apt, rec, film, mom, feat, W, H)
        assert rc == 0 and guards
        want, steps = dr.denoise(rec, film, mom, feat, W, H, history=True)
        dr.assert_same(out, want)
        assert np.isnan(want).any() == nan
        # the work buffer's records, as the header lays them out: the last iteration's result and its input
        c = work.reshape(4, W * H, 4)[2:]
        for k in (it, it - 1):
            i, vi = steps[k]
            dr.assert_same(c[k & 1], np.stack([a.reshape(-1) for a in i + [vi]], axis=1))


def test_the_restatement_refuses_a_float64_intermediate():
    ps, feat = dr.synthetic(5, 3, nan=False)
    film, mom = dr.accumulate(list(ps))
    with pytest.raises(AssertionError):
        dr.accumulate([ps[0], ps[1].astype(D)])
    with pytest.raises(AssertionError):
        dr.prepare(film.astype(D), mom, feat, 3, F(1 / 32))


def test_a_real_film_and_its_moments(apt):
    """film_ref passes of the closed 8-sphere lamp scene with NEE, 16 x 8, K = 3, with features_ref planes: the moments' film is
    film_ref.accumulate of the same passes bit for bit, the twin is the restatement, and pass 0 stores over whatever was there."""
    w, h, K = 16, 8, 3
    p, sph, mat, passes, feat = _room_passes(apt, w, h, 2, K)
    film, mom = dr.accumulate_host(apt, passes)                                    # (into NaN-filled buffers)
    dr.assert_same(film, fr.accumulate(passes))
    want_film, want_mom = dr.accumulate(passes)
    dr.assert_same(film, want_film)
    dr.assert_same(mom, want_mom)
    assert np.isfinite(mom).all() and (mom[1] > 0).any() and not any(np.signbit(q).any() for q in passes)   # no -0: 0 + r is r
    rec = _rec(apt, K)
    rc, out, _, guards = dr.denoise_host(apt, rec, film, mom, feat, w, h)
    assert rc == 0 and guards
    dr.assert_same(out, dr.denoise(rec, film, mom, feat, w, h))
    assert np.isfinite(out).all() and out.min() >= 0


def test_accumulate_sizes_and_empty(apt):
    L = apt._lib.denoise_lib()
    one = np.zeros(6, dtype=F)
    assert L.apt_film_accumulate_host(dr.ptr(one), 0, dr.ptr(one), dr.ptr(one), 0) == 0
    rng = np.random.default_rng(4)
    for n in (1, 3, 64, 257):
        ps = [(rng.random((3, n)) * 50).astype(F) for _ in range(4)]
        film, mom = dr.accumulate_host(apt, ps)
        want = dr.accumulate(ps)
        dr.assert_same(film, want[0])
        dr.assert_same(mom, want[1])


# ---- properties of the contract, on the twin ----------------------------------------------------------------------------------------------
def _pow2_guides(W, H, seed):
    """Arbitrary guides whose A = albedo + (1 - cov) is a power of two per channel, so that c / A and i * A are exact."""
    rng = np.random.default_rng(seed)
    N = W * H
    feat = np.zeros((dr.PLANES, N), dtype=F)
    cov = rng.choice([1.0, 0.5, 0.0], size=N)
    feat[dr.COVERAGE] = cov
    feat[dr.DEPTH] = cov * (20 + 200 * rng.random(N))
    nrm = rng.normal(size=(3, N))
    feat[dr.NORMAL:dr.NORMAL + 3] = nrm / np.linalg.norm(nrm, axis=0) * cov
    A = rng.choice([1.0, 0.5, 0.25], size=(3, N))
    A = np.where(cov == 0.0, 1.0, np.where(cov == 0.5, np.maximum(A, 0.5), A))    # cov 0: albedo 0; cov 1/2: albedo 0 or 1/2
    feat[dr.ALBEDO:dr.ALBEDO + 3] = A - (1.0 - cov)
    return feat, A.astype(F)


def test_constant_illumination_comes_back(apt):
    """i = c for every pixel, over arbitrary guides and moments.  An iteration returns S / W with S the sequential sum of at most 25
    products w * i_q and W of the same w: when every i_q lies in c (1 +- e), S lies in c (1 +- e) * sum(w) * (1 + U)^25 (one rounding per
    product, at most 24 per running sum), W in sum(w) * (1 - U)^24 at the least, and the divide rounds once more:
    (1 + e') = (1 + e) (1 + U)^26 / (1 - U)^24, from e = 0.  No weight is negative, so nothing cancels.  A product w * i_q below the normal range is
    off by 2^-150 at most instead: 25 of them over W >= 9/64.  film = K c A with K = 4 and A a power of two makes i = c and out = i A exact."""
    W, H, K, c = 23, 19, 4, F(1.3125)
    feat, A = _pow2_guides(W, H, 11)
    film = (F(K) * c * A).astype(F)
    ps, _ = dr.synthetic(W, H, passes=K, nan=False)
    mom = dr.accumulate(list(ps))[1]                                              # arbitrary, valid moments
    for it in (1, 5):
        rc, out, _, guards = dr.denoise_host(apt, _rec(apt, K, it), film, mom, feat, W, H)
        assert rc == 0 and guards
        e = ((1 + U) ** 26 / (1 - U) ** 24) ** it - 1 + it * 25 * 2.0 ** -150 * 64 / 9
        err = np.abs(out.astype(D) / A.astype(D) - D(c)) / D(c)
        print("constant illumination, %d iterations: relative error %.3g, bound %.3g" % (it, err.max(), e))
        assert err.max() <= e


def test_opposed_normals_never_exchange_illumination(apt):
    """Two half-images of full coverage with normals (0, 0, 1) and (0, 0, -1): across the border x_n = sigma_n * (1 - (-1)) = 2 sigma_n
    > 8, so t = 0 and w = 0 exactly, and S + 0 * i_q = S.  Through all 5 iterations a half of exactly 0 stays exactly 0 beside a half
    that is positive everywhere -- any illumination that crossed, at any iteration, would show --, on either side.  What does cross is
    the variance: gv has no edge stop, so from the second iteration on a border pixel's isd knows the other half's weights.  With
    one iteration gv is prepare's, and then neither half's result changes by a bit when the other half's film changes."""
    W, H, K = 12, 9, 3
    rec = _rec(apt, K, sigma_n=16.0)
    assert 2 * rec.sigma_n > 8 and rec.iterations == 5
    ps, feat = dr.synthetic(W, H, passes=K, nan=False)
    film, mom = dr.accumulate(list(ps))
    left = np.arange(W * H) < (W // 2) * H
    feat[dr.COVERAGE] = 1
    feat[dr.NORMAL:dr.NORMAL + 3] = 0
    feat[dr.NORMAL + 2] = np.where(left, 1, -1)
    assert (film > 0).all()
    for dark in (left, ~left):
        rc, out, _, _ = dr.denoise_host(apt, rec, np.where(dark, F(0), film), mom, feat, W, H)
        assert rc == 0 and np.all(out[:, dark].view(np.uint32) == 0) and (out[:, ~dark] > 0).all()
    one = _rec(apt, K, 1, sigma_n=16.0)
    outs = [dr.denoise_host(apt, one, f, mom, feat, W, H)[1] for f in
            (film, np.where(left, F(3) * film + F(1), film).astype(F), np.where(left, film, F(3) * film + F(1)).astype(F))]
    dr.assert_same(outs[1][:, ~left], outs[0][:, ~left])                          # the left half changed: the right half did not
    dr.assert_same(outs[2][:, left], outs[0][:, left])                            # and the other way round
    assert not np.array_equal(outs[1][:, left], outs[0][:, left]) and not np.array_equal(outs[2][:, ~left], outs[0][:, ~left])


def test_zero_variance_passes_through(apt):
    """K = 4 equal passes: m0 = 4 l and m1 = 4 fl(l l) exactly, so v = 0, gv = 0 and isd = 1 / 1e-6.  With luminances of i at least
    5e-4 apart every tap but the centre has x_l >= 5e-4 / 1e-6 (1 - 3 U) > 8 and weight 0: i' = fl(w i) / w with w = 9/64, one product
    and one divide, so i' is within (1 + U)^2 of i per iteration.  Around the 5 iterations: c = film / K, i = c / A and out = i A, one
    rounding each.  The luminances drift by those few ulps and stay apart."""
    W, H, K = 9, 7, 4
    N = W * H
    rng = np.random.default_rng(3)
    feat = np.zeros((dr.PLANES, N), dtype=F)
    feat[dr.COVERAGE] = 1
    feat[dr.DEPTH] = 100
    feat[dr.NORMAL + 2] = 1
    feat[dr.ALBEDO:dr.ALBEDO + 3] = 0.2 + 0.7 * rng.random((3, N))
    tint = 0.5 + rng.random((3, N))
    i = tint / (0.2126 * tint[0] + 0.7152 * tint[1] + 0.0722 * tint[2]) * (1 + rng.permutation(N)) * 1e-3     # lum(i) = 1e-3 (k + 1)
    one = (i * feat[dr.ALBEDO:dr.ALBEDO + 3]).astype(F)
    film, mom = dr.accumulate([one] * K)
    li = np.sort(dr.lum(*(film / F(K) / feat[dr.ALBEDO:dr.ALBEDO + 3]).astype(F)).astype(D))
    assert np.diff(li).min() > 5e-4
    rc, out, work, _ = dr.denoise_host(apt, _rec(apt, K), film, mom, feat, W, H)
    assert rc == 0 and np.all(work.reshape(4, N, 4)[2:, :, 3] == 0)                # vi stays 0
    mean = film.astype(D) / K
    err = np.abs(out.astype(D) - mean) / mean
    bound = (1 + U) ** (2 * 5 + 3) - 1
    print("zero variance: relative error %.3g, bound %.3g" % (err.max(), bound))
    assert err.max() <= bound


@pytest.mark.parametrize("it", [1, 2, 3, 4, 5])
def test_the_variance_never_grows_past_its_taps(apt, it):
    """vi' = V / (W W), V = sum (w w) vi_q <= max(vi_q) sum(w w) <= max(vi_q) (sum w)^2.  Roundings: two products per term and at most 24 adds
    in V (upwards, (1 + U)^26), at most 24 adds in W, twice (downwards, (1 - U)^48), W W and the divide (two more)."""
    W, H, K = 33, 17, 3
    ps, feat = dr.synthetic(W, H, passes=K, nan=False)
    film, mom = dr.accumulate(list(ps))
    rc, _, work, _ = dr.denoise_host(apt, _rec(apt, K, it), film, mom, feat, W, H)
    assert rc == 0
    c = work.reshape(4, W * H, 4)[2:]
    vin, vout = c[(it - 1) & 1][:, 3].reshape(W, H).astype(D), c[it & 1][:, 3].reshape(W, H).astype(D)
    s = 1 << (it - 1)
    top = np.zeros((W, H))
    for dx, dy, inside, qx, qy in dr._taps(W, H, 2, s):
        top = np.where(inside, np.maximum(top, vin[qx, qy]), top)
    assert (vin > 0).any() and np.all(vout <= top * (1 + U) ** 28 / (1 - U) ** 48)


# ---- quality ------------------------------------------------------------------------------------------------------------------------------------
def test_the_filter_gains_on_the_lamp_room(apt):
    """The diffuse closed room with its lamp under APT_FLAG_NEE at 4 passes of 1 sample (16 paths per pixel) against one pass of 256
    samples (1024 paths per pixel: 64 times the paths).  The error is the old prototype's: the mean squared error of the means
    clipped to [0, 1].  Asserted: the ordering, with the default record.  The ratio is printed (DESIGN "Denoise" records it)."""
    w, h, K = 32, 24, 4
    p, sph, mat, passes, feat = _room_passes(apt, w, h, 1, K, seed=11)
    film, mom = dr.accumulate_host(apt, passes)
    ref = fr.render_pass(_oparams(width=w, height=h, samples=256, depth=4, num_spheres=8, light_index=7, seed=977, flags=apt.APT_FLAG_NEE),
                         sph, mat)[0].astype(D)
    rc, out, _, _ = dr.denoise_host(apt, _rec(apt, K), film, mom, feat, w, h)
    assert rc == 0
    clip = lambda a: np.clip(a, 0, 1)
    noisy = film.astype(D) / K
    mse = lambda a: float(np.mean((clip(a) - clip(ref)) ** 2))
    raw = lambda a: float(np.mean((a - ref) ** 2))
    print("lamp room %dx%d, %d x 4 paths: clipped MSE unfiltered %.6f filtered %.6f ratio %.3f (prototype 0.00121 / 0.00147 = %.3f); "
          "unclipped %.4f -> %.4f" % (w, h, K, mse(noisy), mse(out.astype(D)), mse(out.astype(D)) / mse(noisy), 0.00121 / 0.00147,
                                    raw(noisy), raw(out.astype(D))))
    assert mse(out.astype(D)) < mse(noisy)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_denoise_refusals_write_nothing(apt):
    L = apt._lib.denoise_lib()
    W, H = 5, 3
    N = W * H
    ps, feat = dr.synthetic(W, H, nan=False)
    film, mom = dr.accumulate(list(ps))
    work = np.full(16 * N + 4, -7.0, dtype=F)
    work = work[(-work.ctypes.data // 4) % 4:][:16 * N]
    out = np.full((3, N), -7.0, dtype=F)

    def call(rec, film_=film, mom_=mom, feat_=feat, w=W, h=H, work_=work, out_=out):
        work_p = work_ if work_ is None or isinstance(work_, ctypes.c_void_p) else ctypes.c_void_p(work_.ctypes.data)
        rc = L.apt_film_denoise_host(None if rec is None else ctypes.byref(rec), dr.ptr(film_), dr.ptr(mom_), dr.ptr(feat_), w, h, work_p,
                                     dr.ptr(out_))
        assert np.all(out == -7.0) and np.all(work == -7.0)
        assert rc != 0 and L.apt_film_denoise_last_error() != b""
        return rc

    good = lambda **kw: _rec(apt, kw.pop("passes", 3), kw.pop("iterations", None), **kw)
    assert call(None) == APT_ERR_ARG
    for name in ("film_", "mom_", "feat_", "work_", "out_"):
        assert call(good(), **{name: None}) == APT_ERR_ARG
    assert call(good(), work_=ctypes.c_void_p(work.ctypes.data + 4)) == APT_ERR_ARG and b"aligned" in L.apt_film_denoise_last_error()
    assert call(good(), w=0) == APT_ERR_ARG and call(good(), h=0) == APT_ERR_ARG
    for passes in (0, 1, (1 << 24) + 1):
        assert call(good(passes=passes)) == APT_ERR_ARG and b"passes" in L.apt_film_denoise_last_error()
    for it in (0, 6):
        assert call(good(iterations=it)) == APT_ERR_ARG and b"iterations" in L.apt_film_denoise_last_error()
    for bad in (-1.0, float("nan"), float("inf")):
        for k in dr.SIGMAS:
            assert call(good(**{k: bad})) == APT_ERR_ARG and b"sigma" in L.apt_film_denoise_last_error()
        assert call(good(albedo_floor=bad)) == APT_ERR_ARG
    assert call(good(albedo_floor=0.0)) == APT_ERR_ARG and b"albedo_floor" in L.apt_film_denoise_last_error()
    assert call(good(), w=1 << 14, h=(1 << 14) + 1) == APT_ERR_ARG and b"2^28" in L.apt_film_denoise_last_error()
    rec = good()
    rec.struct_size = 36
    assert call(rec) == APT_ERR_STRUCT
    # the limits themselves are accepted
    rec = good(passes=1 << 24, iterations=1, sigma_n=0.0, sigma_z=0.0, sigma_c=0.0, sigma_a=0.0, sigma_l=0.0)
    assert L.apt_film_denoise_host(ctypes.byref(rec), dr.ptr(film), dr.ptr(mom), dr.ptr(feat), W, H, ctypes.c_void_p(work.ctypes.data),
                                   dr.ptr(out)) == 0
    assert not np.any(out == -7.0)


def test_accumulate_refusals_write_nothing(apt):
    L = apt._lib.denoise_lib()
    a = np.full((3, 4), 2.0, dtype=F)
    film, mom = np.full((3, 4), -7.0, dtype=F), np.full((2, 4), -7.0, dtype=F)
    for args in ((None, 4, dr.ptr(film), dr.ptr(mom)), (dr.ptr(a), 4, None, dr.ptr(mom)), (dr.ptr(a), 4, dr.ptr(film), None),
                 (dr.ptr(a), 1 << 40, dr.ptr(film), dr.ptr(mom))):
        assert L.apt_film_accumulate_host(*args, 0) == APT_ERR_ARG and L.apt_film_denoise_last_error() != b""
        assert np.all(film == -7.0) and np.all(mom == -7.0)
    # the device form refuses the same before any HIP call
    assert L.apt_film_accumulate_device(None, None, 4, dr.ptr(film), dr.ptr(mom), 0) == APT_ERR_ARG
    assert L.apt_film_accumulate_device(None, dr.ptr(a), 0, dr.ptr(film), dr.ptr(mom), 0) == 0
    rec = _rec(apt, 1)
    p16 = ctypes.c_void_p(0x1000)
    assert L.apt_film_denoise_device(ctypes.byref(rec), None, p16, p16, p16, 4, 4, p16, p16) == APT_ERR_ARG and b"passes" in L.apt_film_denoise_last_error()
