"""CPU-only: adaptive sampling (libadaptive_mi355x.so, include/render_mi355x_adaptive.h) -- the CPU twins of select, accumulate-list
and mean bit for bit against the restatement tests/adaptive_ref.py, the tie of the new normalisation to the resolve's, every refusal,
and, on the restatement, that a list pass is told from three wrong renderers by the lists the GPU tests use.

Without the feature nothing here passes: the library, the header, the binding and the restatement do not exist."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adaptive_ref as ar
import film_ref as fr
import materials_ref as mr

F, U32 = np.float32, np.uint32
APT_ERR_ARG, APT_ERR_STRUCT = 1, 2
NAMES = ["apt_film_select_default_host", "apt_film_select_work_words", "apt_film_select_device", "apt_film_select_host",
         "apt_film_accumulate_list_device", "apt_film_accumulate_list_host", "apt_film_mean_device", "apt_film_mean_host",
         "apt_film_adaptive_last_error"]


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data, render
    pkg.gen_data, pkg.render = gen_data, render
    return pkg


def _header_prototypes():
    """include/render_mi355x_adaptive.h -> {name: (restype, [argtypes])} in the header's order, by the binding's type rules."""
    scalars = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(mr.ROOT, "include", "render_mi355x_adaptive.h")).read(), flags=re.S)
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


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_symbols_record_and_defaults(apt):
    """A third library with a header of its own: the binding's table is that header's, entry by entry and in its order, the library
    exports those names and nothing else, and the other two libraries and their headers know none of them."""
    from ascendpathtracing_amd._lib import ApFilmSelect
    L = apt._lib.adaptive_lib()
    assert ctypes.sizeof(ApFilmSelect) == 24 and ApFilmSelect.threshold.offset == 16 and ApFilmSelect.floor.offset == 20
    header = _header_prototypes()
    assert list(header) == NAMES
    table = apt._lib.ADAPTIVE_PROTOTYPES
    assert list(table) == list(header)
    for name, proto in header.items():
        assert (table[name][0], list(table[name][1])) == proto, name
        fn = getattr(L, name)
        assert fn.restype is table[name][0] and list(fn.argtypes) == list(table[name][1]), name
    assert _exports(apt._lib.ADAPTIVE_LIB_PATH) == set(header)
    new = set(header) | {"apt_film_select"}
    assert not new & (set(apt._lib.ABI_SYMBOLS) | set(apt._lib.DENOISE_PROTOTYPES))
    assert not new & (_exports(apt._lib.LIB_PATH) | _exports(apt._lib.DENOISE_LIB_PATH))
    for h in ("render_mi355x.h", "render_mi355x_denoise.h"):
        text = open(os.path.join(mr.ROOT, "include", h)).read()
        assert not re.search(r"\b(%s)\s*\(" % "|".join(sorted(new)), text), h          # (render_mi355x.h names one in prose: no prototype)
    assert apt._lib.lib().apt_abi_version() == 3
    assert apt.APT_FLAG_PIXEL_LIST == 256 and apt._lib.APT_DEV_LIST_RANGE == 64
    head = open(os.path.join(mr.ROOT, "include", "render_mi355x.h")).read()
    assert re.search(r"APT_FLAG_PIXEL_LIST = 256u", head) and re.search(r"APT_DEV_LIST_RANGE = 64u", head)
    r = apt._lib.film_select_record(7)
    assert (r.struct_size, r.base_passes) == (24, 7) and 2 <= r.min_passes <= r.max_passes <= 1 << 24
    assert all(np.isfinite(v) and v >= 0 for v in (r.threshold, r.floor))
    big = apt._lib.film_select_record(1 << 24)
    assert big.min_passes == big.max_passes == 1 << 24
    assert L.apt_film_select_default_host(None, 3) == APT_ERR_ARG and b"null" in L.apt_film_adaptive_last_error()
    assert L.apt_film_select_default_host(ctypes.byref(r), 1) == APT_ERR_ARG and L.apt_film_select_default_host(ctypes.byref(r), (1 << 24) + 1) == APT_ERR_ARG
    assert L.apt_film_select_default_host(ctypes.byref(r), 3) == 0 and L.apt_film_adaptive_last_error() == b""
    assert [L.apt_film_select_work_words(n) for n in (1, 256, 257, 1920 * 1080, 1 << 28)] == [1, 1, 2, 8100, 1 << 20]
    assert apt._lib.film_select_record(4, threshold=0.5, max_passes=9).max_passes == 9
    with pytest.raises(apt.AptError):
        apt._lib.film_select_record(4, sigma=1.0)
    for name in ("film_select", "film_accumulate_list", "film_mean"):
        assert hasattr(apt.render, name)
    assert hasattr(apt.render.Film, "add_adaptive_pass")


# ---- the twins against the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ar.KINDS)
@pytest.mark.parametrize("n", ar.SIZES)
def test_select_twin_equals_the_restatement(apt, n, kind):
    """The list is np.nonzero of the predicate: ascending, its length in count, and no word written from count on or outside."""
    _, mom, extra = ar.synthetic(n, kind)
    recs = [ar.REC] + ([dict(ar.REC, floor=0.0)] if kind == "floor" else [])
    for rec in recs:
        want = ar.select(mom, extra, **rec)
        rc, got, count, untouched = ar.select_host(apt, mom, extra, ar.record(apt, **rec))
        assert rc == 0 and count == want.size and untouched
        assert np.array_equal(got, want)
        assert np.all(np.diff(got.astype(np.int64)) > 0)
    # the kinds are what they say they are
    sel = ar.predicate(mom, extra, **ar.REC)
    if kind == "none":
        assert not sel.any()
    elif kind == "all":
        assert sel.all()
    elif kind == "alternating":
        assert np.array_equal(sel, np.arange(n) % 2 == 0)
    elif kind == "threshold":
        assert not sel[0::3].any() and not sel[2::3].any()              # e == t, and below it: not selected
    elif kind == "nan":
        nu = ar.REC["base"] + extra
        assert not sel[(np.isnan(mom).any(axis=0)) & (nu >= ar.REC["min_passes"])].any()
        assert sel[nu < ar.REC["min_passes"]].all()
    elif kind == "counts":
        nu = ar.REC["base"] + extra.astype(np.int64)
        assert sel[nu < ar.REC["min_passes"]].all() and not sel[nu >= ar.REC["max_passes"]].any()
        inside = (nu >= ar.REC["min_passes"]) & (nu < ar.REC["max_passes"])
        assert np.array_equal(sel[inside], (np.arange(n) % 2 == 0)[inside])
    elif kind == "floor":
        assert not sel.any() and ar.predicate(mom, extra, **dict(ar.REC, floor=0.0)).all()


@pytest.mark.parametrize("kind", ["random", "nan"])
@pytest.mark.parametrize("n", ar.SIZES)
def test_accumulate_list_and_mean_twins_equal_the_restatement(apt, n, kind):
    film, mom, extra = ar.synthetic(n, kind)
    lst = ar.select(mom, extra, **ar.REC)
    rng = np.random.default_rng(n)
    planes = (rng.random((3, lst.size)) * 3).astype(F)
    if kind == "nan" and lst.size:
        planes[1, 0] = np.nan
    want = ar.accumulate_list(planes, lst, film, mom, extra)
    rc, f, m, e, intact = ar.accumulate_list_host(apt, planes, lst, film, mom, extra)
    assert rc == 0 and intact
    for g, w in zip((f, m, e), want):
        ar.assert_same(g, w)
    if lst.size:
        assert np.array_equal(e[lst] - extra[lst], np.ones(lst.size, dtype=U32))
    for ex in (None, e):
        rc, out = ar.mean_host(apt, f, ar.REC["base"], ex)
        assert rc == 0
        ar.assert_same(out, ar.mean(f, ar.REC["base"], ex))


def test_accumulate_list_skips_entries_beyond_the_image(apt):
    """An entry >= N -- a slot the list pass left untouched, NaN here -- stays out of the film; nothing outside the planes is written."""
    n = 65
    film, mom, extra = ar.synthetic(n, "random")
    lst = np.array([3, n, 64, 0xFFFFFFFF, 0, n + 1000], dtype=U32)
    planes = np.arange(18, dtype=F).reshape(3, 6) + F(1)
    planes[:, [1, 3, 5]] = np.nan
    rc, f, m, e, intact = ar.accumulate_list_host(apt, planes, lst, film, mom, extra)
    assert rc == 0 and intact
    for g, w in zip((f, m, e), ar.accumulate_list(planes, lst, film, mom, extra)):
        ar.assert_same(g, w)
    touched = np.zeros(n, dtype=bool)
    touched[[3, 64, 0]] = True
    assert np.array_equal(e != extra, touched) and not np.isnan(f).any()
    assert ar.bits_differ(f[:, touched], film[:, touched]) and not ar.bits_differ(f[:, ~touched], film[:, ~touched])


@pytest.mark.parametrize("n", [1, 257, 1001])
def test_mean_without_extra_is_the_resolves_normalisation(apt, n):
    """mean (extra NULL or all zero), then the resolve with passes = 1, is the resolve of the film with passes = base, bit for bit:
    x / 1 is exact."""
    table = apt.gen_data.film_curve("srgb")
    film = fr.value_pool([table])[: 3 * n]
    film = np.resize(film, 3 * n).reshape(3, n).astype(F)
    for base in (2, 3, 7, 1 << 24):
        for ex in (None, np.zeros(n, dtype=U32)):
            rc, mean = ar.mean_host(apt, film, base, ex)
            assert rc == 0
            for tonemap in (fr.TONEMAP_CLIP, fr.TONEMAP_REINHARD):
                rc1, out1, u1, g1 = fr.resolve_host(apt, mean, 1, 1.5, tonemap, 0.25, table)
                rc2, out2, u2, g2 = fr.resolve_host(apt, film, base, 1.5, tonemap, 0.25, table)
                assert rc1 == rc2 == 0 and g1 and g2
                ar.assert_same(out1, out2)
                assert np.array_equal(u1, u2)


# ---- refusals: nothing written --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(apt):
    L = apt._lib.adaptive_lib()
    n = 70
    film, mom, extra = ar.synthetic(n, "random")
    good = ar.record(apt, **ar.REC)

    def rec(**kw):
        r = ar.record(apt, **ar.REC)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad = [(rec(struct_size=20), APT_ERR_STRUCT), (rec(base_passes=1), APT_ERR_ARG), (rec(base_passes=(1 << 24) + 1), APT_ERR_ARG),
           (rec(min_passes=1), APT_ERR_ARG), (rec(max_passes=(1 << 24) + 1), APT_ERR_ARG), (rec(min_passes=10, max_passes=9), APT_ERR_ARG),
           (rec(threshold=float("nan")), APT_ERR_ARG), (rec(threshold=-1.0), APT_ERR_ARG), (rec(floor=float("inf")), APT_ERR_ARG),
           (rec(floor=-0.5), APT_ERR_ARG)]
    for r, code in bad:
        rc, got, count, untouched = ar.select_host(apt, mom, extra, r)
        assert rc == code and untouched and count == 0xDEADBEEF and L.apt_film_adaptive_last_error() != b""
    lst, work, count = (np.full(n, 0xDEADBEEF, dtype=U32) for _ in range(3))
    p = ar._p
    args = [ctypes.byref(good), p(mom), p(extra), n, p(work), p(lst), p(count)]
    for i in (0, 1, 2, 4, 5, 6):
        a = list(args)
        a[i] = None
        assert L.apt_film_select_host(*a) == APT_ERR_ARG
    for big in (0, (1 << 28) + 1):
        a = list(args)
        a[3] = big
        assert L.apt_film_select_host(*a) == APT_ERR_ARG
    assert all(np.all(x == 0xDEADBEEF) for x in (lst, work, count))
    assert L.apt_film_select_host(*args) == 0 and L.apt_film_adaptive_last_error() == b""

    planes = np.ones((3, 4), dtype=F)
    l4 = np.array([1, 2, 3, 4], dtype=U32)
    f, m, e = film.copy(), mom.copy(), extra.copy()
    args = [p(planes), p(l4), 4, n, p(f), p(m), p(e)]
    for i in (0, 1, 4, 5, 6):
        a = list(args)
        a[i] = None
        assert L.apt_film_accumulate_list_host(*a) == APT_ERR_ARG
    for i, v in ((3, 0), (3, (1 << 28) + 1), (2, n + 1)):
        a = list(args)
        a[i] = v
        assert L.apt_film_accumulate_list_host(*a) == APT_ERR_ARG, (i, v)
    a = list(args)
    a[2] = 0
    assert L.apt_film_accumulate_list_host(*a) == 0                                   # an empty list: nothing done
    assert not ar.bits_differ(f, film) and not ar.bits_differ(m, mom) and np.array_equal(e, extra)

    out = np.full((3, n), -7.0, dtype=F)
    for a in ([None, None, 3, n, p(out)], [p(film), None, 3, n, None], [p(film), None, 1, n, p(out)], [p(film), None, (1 << 24) + 1, n, p(out)],
              [p(film), None, 3, 0, p(out)], [p(film), None, 3, (1 << 28) + 1, p(out)]):
        assert L.apt_film_mean_host(*a) == APT_ERR_ARG
    assert np.all(out == F(-7))


# ---- the restatement of a list pass, and the lists of the GPU tests ---------------------------------------------------------------------
def _lamp_room(apt):
    sph = apt.gen_data.with_lamp(apt.gen_data.gen_spheres(), 8, 7)
    return sph, np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)


@pytest.mark.parametrize("shape", [(48, 32), (24, 16)], ids=lambda s: "%dx%d" % s)
def test_gpu_test_lists_tell_a_list_pass_from_three_wrong_renderers(apt, shape):
    """On the restatement: the compact index used as the pixel, pass 0's seed for every round and the list read one entry late each give
    other bits than the list pass on the lists tests/test_gpu_film_list.py uses.  Two lists cannot see one of the three by their
    nature -- every pixel in order IS its compact index, and a single entry has no later one -- and are held to the other two."""
    from oracle import oracle
    w, h = shape
    sph, mat = _lamp_room(apt)
    p = oracle.make_params(width=w, height=h, samples=3, depth=3, num_spheres=8, light_index=7, seed=3, flags=apt.APT_FLAG_NEE)
    pass0, pass2 = (fr.render_pass(p, sph, mat, pass_index=k)[0] for k in (0, 2))
    differs = lambda a, b: ar.bits_differ(a, b)
    for name, lst in ar.gpu_lists(w * h).items():
        right = ar.list_pass(pass2, lst)
        ar.assert_same(right, pass2[:, lst.astype(np.int64)])
        compact, seed0, late = ar.wrong_compact_index(pass2, lst), ar.list_pass(pass0, lst), ar.wrong_late_read(pass2, lst)
        assert differs(right, seed0), name
        if name == "all":
            assert not differs(right, compact) and differs(right, late)
        elif name == "one":
            assert differs(right, compact) and not differs(right, late)
        else:
            assert ar.sensitive(lst, pass0, pass2), name
    # and the accumulate of such a pass is the accumulate of the whole pass at the listed pixels
    lst = ar.gpu_lists(w * h)["strided17"]
    film, mom = fr.accumulate([pass0, pass0]), ar.moments_of([pass0, pass0])
    f, m, e = ar.accumulate_list(ar.list_pass(pass2, lst), lst, film, mom, np.zeros(w * h, dtype=U32))
    whole_f, whole_m = fr.accumulate([pass0, pass0, pass2]), ar.moments_of([pass0, pass0, pass2])
    idx = lst.astype(np.int64)
    ar.assert_same(f[:, idx], whole_f[:, idx])
    ar.assert_same(m[:, idx], whole_m[:, idx])
    rest = np.setdiff1d(np.arange(w * h), idx)
    ar.assert_same(f[:, rest], film[:, rest])
    assert e.sum() == 17
