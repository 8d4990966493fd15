"""CPU-only: the film (include/render_mi355x.h "film") -- the restatement tests/film_ref.py against tests/materials_ref.py's frames, the pass
seed, the independence of passes, the curve tables, the resolve's CPU twin apt_film_resolve_host bit for bit against the restatement
with every refusal, and the PFM writer.

Without the feature nothing here passes: the entries and gen_data.film_curve do not exist."""
import ctypes

import numpy as np
import pytest

import film_ref as fr
import materials_ref as mr

F, U = np.float32, np.uint64
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data, render
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def _bits_equal(got, want):
    got, want = np.ascontiguousarray(got, dtype=F), np.ascontiguousarray(want, dtype=F)
    diff = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def _oparams(**kw):
    from oracle import oracle
    return oracle.make_params(**kw)


# ---- a pass ---------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_record(apt):
    from ascendpathtracing_amd._lib import ApFilmResolve
    assert ctypes.sizeof(ApFilmResolve) == 24 and ApFilmResolve.exposure.offset == 16 and ApFilmResolve.inv_white2.offset == 20
    assert apt._lib.lib().apt_abi_version() == 3                                  # additive: same ABI version
    for name in ("apt_film_pass_seed", "apt_render_frame_film", "apt_context_render_frame_film", "apt_film_curve_host",
                 "apt_film_resolve_device", "apt_film_resolve_host", "apt_write_pfm"):
        assert name in apt._lib.ABI_SYMBOLS
    header = open(mr.ROOT + "/include/render_mi355x.h").read()
    assert "APT_FILM_PASS_SALT 0x%016Xull" % fr.PASS_SALT in header and "#define APT_ABI_VERSION 3 " in header
    assert apt._lib.APT_FILM_PASS_SALT == fr.PASS_SALT


def test_pass_zero_clipped_is_the_frame(apt):
    """clip(pass 0) is materials_ref.render_frame's fb bit for bit (NaNs as bits), in the closed room and under a sun far above 1."""
    g = apt.gen_data
    sph, mat = g.gen_spheres_materials()
    room = (g.with_lamp(sph, 9, 7), mat, 9, 7, None, apt.APT_FLAG_NEE)
    sph, mat = g.gen_spheres_open()
    env = mr.Env.from_ctypes(g.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45),
                                           sun_radiance=(300.0, 280.0, 240.0), sun_angle_deg=8.0, sample_sun=True))
    open_ = (sph, mat, 8, -1, env, g.materials_flags(mat))
    for name, (sph, mat, ns, light, env, flags) in (("room", room), ("open", open_)):
        p = _oparams(width=16, height=8, samples=3, depth=4, num_spheres=ns, light_index=light, seed=5, flags=flags)
        film, _ = fr.render_pass(p, sph, mat, env=env)
        fb = mr.render_frame(p, sph, mat, env=env)[0]
        assert film.dtype == F and film.shape == fb.shape == (3, 128)
        with np.errstate(invalid="ignore"):
            _bits_equal(np.clip(film, F(0), F(1)), fb)
        assert film.max() > 1.0, name                                             # else the clip is not exercised and this shows nothing
        assert np.isfinite(film).all()


def test_pass_seed(apt):
    L = apt._lib.lib()
    seeds = (0, 5, 0xFFFFFFFFFFFFFFFF)
    seen = set()
    for s in seeds:
        assert fr.pass_seed(s, 0) == s == L.apt_film_pass_seed(s, 0)
        vals = [fr.pass_seed(s, k) for k in range(4096)]
        assert vals == [L.apt_film_pass_seed(s, k) for k in range(4096)]
        seen.update(vals)
    assert len(seen) == 3 * 4096
    assert fr.pass_seed(1, 0xFFFFFFFF) == L.apt_film_pass_seed(1, 0xFFFFFFFF)
    # the salt: a pass seed is not the roulette key splitmix64(seed ^ splitmix64(path)) of path `pass`
    assert all(fr.pass_seed(5, k) != int(mr.splitmix64(U(5) ^ mr.splitmix64(U(k)))) for k in range(1, 64))


def test_accumulate_is_the_sequential_float32_sum():
    rng = np.random.default_rng(1)
    ps = [(rng.random((3, 7)) * 1e3).astype(F) for _ in range(5)]
    want = ps[0].copy()
    for p in ps[1:]:
        want = (want + p).astype(F)
    _bits_equal(fr.accumulate(ps), want)
    _bits_equal(fr.accumulate(ps[:1]), ps[0])
    with pytest.raises(AssertionError):
        fr.accumulate([ps[0], ps[1].astype(np.float64)])


# The acceptance band of the independence test.  For each of the N pixel channels the variance of the K-pass mean over the 32 base seeds
# is an unbiased estimate s_i^2 of sigma_i^2 / K when the passes are independent, with 31 degrees of freedom; V_K is their sum, so
# E[V_1] / E[V_8] = 8.  Were V_1 and V_8 independent and the means Gaussian, (V_1 / 8) / V_8 would be F(nu, nu) distributed with the
# Satterthwaite degrees of freedom nu = 31 * (sum sigma_i^2)^2 / sum sigma_i^4 >= 31.  nu depends on the scene, so the band is taken at its
# worst case nu = 31 (one pixel carrying all the variance; the real figure is 31 times a good part of the 384 pixel channels, which also
# pays for the means not being Gaussian): the two-sided 1e-6 points of F(31, 31) are 6.6059 and its reciprocal
# (scipy.stats.f.isf(5e-7, 31, 31) = 6.60590).  Both variances are taken over the SAME base seeds, so pass 0 is in both and they are
# positively correlated, which only narrows the ratio's distribution: the band is conservative for that too.  A pass_seed that
# returns `seed` for every pass makes every pass pass 0 and the 8-pass mean (a sum of 8 equal float32 values, divided by 8: exact) that
# pass again: the ratio is then exactly 1, below 8 / 6.6059 = 1.211.
F31_31_5E7 = 6.6059
RATIO_BAND = (8.0 / F31_31_5E7, 8.0 * F31_31_5E7)


def _variance_ratio(apt, pass_seed):
    g = apt.gen_data
    sph, mat = g.gen_spheres_materials()
    sph = g.with_lamp(sph, 9, 7)
    w, h, K = 16, 8, 8

    def means(base_seeds, k):
        out = []
        for s in base_seeds:
            passes = []
            for i in range(k):
                p = _oparams(width=w, height=h, samples=2, depth=3, num_spheres=9, light_index=7, seed=pass_seed(s, i), flags=apt.APT_FLAG_NEE)
                passes.append(fr.render_pass(p, sph, mat)[0])                     # (pass 0 of its own seed: the seed rule is pass_seed's)
            out.append(fr.accumulate(passes).astype(np.float64) / k)
        return np.stack(out)

    v1 = means(range(1000, 1032), 1).var(axis=0, ddof=1).sum()
    v8 = means(range(1000, 1032), K).var(axis=0, ddof=1).sum()
    return v1 / v8


def test_passes_are_independent(apt):
    try:
        from scipy.stats import f
        assert abs(f.isf(5e-7, 31, 31) - F31_31_5E7) < 1e-3
    except ImportError:
        pass
    ratio = _variance_ratio(apt, fr.pass_seed)
    print("variance ratio V_1 / V_8 =", ratio, "band", RATIO_BAND)
    assert RATIO_BAND[0] < ratio < RATIO_BAND[1], ratio


# ---- curve tables ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [fr.CURVE_LINEAR, fr.CURVE_SRGB], ids=["linear", "srgb"])
def test_curve_tables(apt, curve):
    t = apt.gen_data.film_curve(curve)
    assert t.dtype == F and t.shape == (256,) and t[0] == 0 and np.all(np.diff(t) > 0) and t[255] < 1
    _bits_equal(t, apt.gen_data.film_curve("linear" if curve == fr.CURVE_LINEAR else "srgb"))
    want = fr.curve(curve)
    ulp = np.abs(t.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1, ulp.max()
    if curve == fr.CURVE_LINEAR:
        _bits_equal(t, want)
    # round trip: the code of table[c] is c, of the float below it c - 1
    y = np.stack([t[1:], np.nextafter(t[1:], F(0)), t[1:]])
    out, u8 = fr.resolve(y, 1, 1.0, fr.TONEMAP_CLIP, 0.0, t)
    _bits_equal(out, y)
    c = np.arange(1, 256)
    assert np.array_equal(u8[:, 0], c) and np.array_equal(u8[:, 1], c - 1) and np.array_equal(u8[:, 2], c)
    assert fr.resolve(np.zeros((3, 1), dtype=F), 1, 1.0, fr.TONEMAP_CLIP, 0.0, t)[1].tolist() == [[0, 0, 0]]
    assert fr.resolve(np.ones((3, 1), dtype=F), 1, 1.0, fr.TONEMAP_CLIP, 0.0, t)[1].tolist() == [[255, 255, 255]]


def test_curve_refusals(apt):
    L = apt._lib.lib()
    t = np.full(256, 7.0, dtype=F)
    assert L.apt_film_curve_host(ctypes.c_uint32(2), t.ctypes.data_as(ctypes.c_void_p)) == APT_ERR_ARG and b"curve" in L.apt_last_error()
    assert np.all(t == 7.0)
    assert L.apt_film_curve_host(ctypes.c_uint32(0), None) == APT_ERR_ARG
    with pytest.raises(apt.AptError):
        apt.gen_data.film_curve("gamma")


# ---- resolve: the CPU twin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [fr.CURVE_LINEAR, fr.CURVE_SRGB], ids=["linear", "srgb"])
@pytest.mark.parametrize("tonemap", [fr.TONEMAP_CLIP, fr.TONEMAP_REINHARD], ids=["clip", "reinhard"])
def test_resolve_host_equals_the_restatement(apt, tonemap, curve):
    tables = [apt.gen_data.film_curve(c) for c in (fr.CURVE_LINEAR, fr.CURVE_SRGB)]
    table = tables[curve]
    pool = fr.value_pool(tables)
    pool = np.concatenate([pool, np.zeros(-len(pool) % 3, dtype=F)])
    whole = pool.reshape(3, -1)
    for passes in (1, 3, 1000):
        for exposure in (0.25, 1.0, 7.5):
            for iw in (0.0, 1.0 / 16.0):
                rc, out, u8, guards = fr.resolve_host(apt, whole, passes, exposure, tonemap, iw, table)
                assert rc == 0 and guards
                want_out, want_u8 = fr.resolve(whole, passes, exposure, tonemap, iw, table)
                _bits_equal(out, want_out)
                assert np.array_equal(u8, want_u8)
                assert not np.isnan(out).any() and out.min() >= 0 and out.max() <= 1
    for n in (1, 2, 3, 5, 64, 257):
        for offset in range(4):
            film = np.resize(np.roll(pool, n + offset), (3, n))
            rc, out, u8, guards = fr.resolve_host(apt, film, 3, 7.5, tonemap, 1.0 / 16.0, table, offset)
            assert rc == 0 and guards
            want_out, want_u8 = fr.resolve(film, 3, 7.5, tonemap, 1.0 / 16.0, table)
            _bits_equal(out, want_out)
            assert np.array_equal(u8, want_u8)
    # one output at a time
    film = np.resize(pool, (3, 65))
    want_out, want_u8 = fr.resolve(film, 1, 1.0, tonemap, 0.0, table)
    rc, out, u8, _ = fr.resolve_host(apt, film, 1, 1.0, tonemap, 0.0, table, want_u8=False)
    assert rc == 0 and np.all(u8 == 0xA5)
    _bits_equal(out, want_out)
    rc, out, u8, _ = fr.resolve_host(apt, film, 1, 1.0, tonemap, 0.0, table, want_out=False)
    assert rc == 0 and np.all(out == -7.0) and np.array_equal(u8, want_u8)


def test_reinhard_maps_white_to_one_and_infinity_to_one(apt):
    t = apt.gen_data.film_curve("linear")
    film = np.array([[4.0, np.inf, 3e38], [0.0, 8.0, 1.0], [2.0, 1e30, np.nan]], dtype=F)
    out, u8 = fr.resolve(film, 1, 1.0, fr.TONEMAP_REINHARD, 1.0 / 16.0, t)
    assert out[0].tolist() == [1.0, 1.0, 1.0] and out[1].tolist() == [0.0, 1.0, float(F(F(1) * F(1.0625)) / F(2))] and out[2, 1:].tolist() == [1.0, 0.0]
    rc, got, _, _ = fr.resolve_host(apt, film, 1, 1.0, fr.TONEMAP_REINHARD, 1.0 / 16.0, t)
    assert rc == 0
    _bits_equal(got, out)
    plain = fr.resolve(film, 1, 1.0, fr.TONEMAP_REINHARD, 0.0, t)[0]
    assert plain[0, 0] == F(4.0) / F(5.0) and plain[0, 1] == 1.0


def test_resolve_with_a_table_that_is_not_increasing(apt):
    rng = np.random.default_rng(3)
    table = rng.random(256).astype(F)
    film = rng.random((3, 100)).astype(F)
    rc, out, u8, _ = fr.resolve_host(apt, film, 1, 1.0, fr.TONEMAP_CLIP, 0.0, table)
    assert rc == 0 and np.array_equal(u8, fr.resolve(film, 1, 1.0, fr.TONEMAP_CLIP, 0.0, table)[1])


def test_resolve_refusals_write_nothing(apt):
    L = apt._lib.lib()
    table = apt.gen_data.film_curve("srgb")
    film = np.full((3, 5), 0.5, dtype=F)
    out = np.full((3, 5), -7.0, dtype=F)
    u8 = np.full((5, 3), 0xA5, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(rec, film_=film, table_=table, out_=out, u8_=u8):
        rc = L.apt_film_resolve_host(None if rec is None else ctypes.byref(rec), None if film_ is None else ptr(film_), ctypes.c_uint64(5),
                                     None if table_ is None else ptr(table_), None if out_ is None else ptr(out_),
                                     None if u8_ is None else ptr(u8_))
        assert np.all(out == -7.0) and np.all(u8 == 0xA5)
        assert rc == apt._lib.lib().apt_last_status() and (rc == 0 or L.apt_last_error() != b"")
        return rc

    good = lambda **kw: apt._lib.film_resolve_record(**{**dict(passes=2, exposure=1.0, tonemap=0, inv_white2=0.0), **kw})
    assert call(None) == APT_ERR_ARG
    assert call(good(), film_=None) == APT_ERR_ARG
    assert call(good(), table_=None) == APT_ERR_ARG
    assert call(good(), out_=None, u8_=None) == APT_ERR_ARG
    assert call(good(passes=0)) == APT_ERR_ARG
    assert call(good(passes=(1 << 24) + 1)) == APT_ERR_ARG
    assert call(good(tonemap=2)) == APT_ERR_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(good(exposure=bad)) == APT_ERR_ARG
        assert call(good(tonemap=1, inv_white2=bad)) == APT_ERR_ARG
    rec = good()
    rec.struct_size = 20
    assert call(rec) == APT_ERR_STRUCT
    rec = good(passes=1 << 24)
    assert L.apt_film_resolve_host(ctypes.byref(rec), ptr(film), ctypes.c_uint64(5), ptr(table), ptr(out), ptr(u8)) == 0
    assert np.all(out == F(0.5) / F(1 << 24))


# ---- PFM -----------------------------------------------------------------------------------------------------------------------------------
def test_write_pfm(apt, tmp_path):
    L = apt._lib.lib()
    w, h = 3, 2
    planes = np.arange(18, dtype=F).reshape(3, w * h) + F(0.5)                   # plane c, pixel (x, y) at x * h + y
    path = str(tmp_path / "a.pfm")
    assert L.apt_write_pfm(path.encode(), ctypes.c_uint32(w), ctypes.c_uint32(h), planes.ctypes.data_as(ctypes.c_void_p)) == 0
    body = b""
    for y in range(h):                                                           # file row r is y = r: bottom to top, as PFM wants
        for x in range(w):
            for c in range(3):
                body += np.array([c * 6 + x * h + y + 0.5], dtype="<f4").tobytes()
    assert open(path, "rb").read() == b"PF\n3 2\n-1.0\n" + body
    assert L.apt_write_pfm(None, ctypes.c_uint32(w), ctypes.c_uint32(h), planes.ctypes.data_as(ctypes.c_void_p)) == APT_ERR_ARG
    assert L.apt_write_pfm(path.encode(), ctypes.c_uint32(w), ctypes.c_uint32(h), None) == APT_ERR_ARG
    assert L.apt_write_pfm(str(tmp_path / "no" / "dir.pfm").encode(), ctypes.c_uint32(w), ctypes.c_uint32(h),
                           planes.ctypes.data_as(ctypes.c_void_p)) == 5
