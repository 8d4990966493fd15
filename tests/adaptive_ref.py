"""NumPy restatement of adaptive sampling (include/render_mi355x_adaptive.h; include/render_mi355x.h "List passes"), for the tests
only: float32 NumPy, one separately rounded operation per step in the header's order.  The list of a select is np.nonzero of the
predicate -- ascending by construction --, a list pass is film_ref.render_pass of the WHOLE frame gathered at the listed pixels.
As in the other restatements f32() fails on a float64 intermediate."""
import ctypes

import numpy as np

import film_ref as fr
from materials_ref import F, f32

U32 = np.uint32
SIZES = (1, 63, 64, 65, 255, 256, 257, 1001, 65537)     # 65537: 257 workgroup counts, more than one 256-wide chunk of the scan


def lum(r, g, b):
    l = f32(F(0.2126) * r)
    l = f32(l + f32(F(0.7152) * g))
    return f32(l + f32(F(0.0722) * b))


def fmax(a, b):
    """a > b ? a : b: a NaN a falls to b."""
    return f32(np.where(a > b, a, b))


def predicate(moments, extra, base, min_passes, max_passes, threshold, floor):
    """-> bool [N]: the pixels apt_film_select_* selects."""
    moments = f32(np.asarray(moments))
    extra = np.asarray(extra)
    assert moments.ndim == 2 and moments.shape[0] == 2 and extra.dtype == U32 and extra.shape == moments.shape[1:]
    assert 2 <= base <= 1 << 24 and 2 <= min_passes <= max_passes <= 1 << 24
    nu = np.uint64(base) + extra.astype(np.uint64)
    arith = (nu >= min_passes) & (nu < max_passes)
    nu_a = np.where(arith, nu, 2).astype(np.uint64)              # the others never reach the arithmetic: any valid count in their place
    with np.errstate(all="ignore"):
        n = nu_a.astype(F)
        assert np.array_equal(n.astype(np.uint64), nu_a)
        lm = f32(moments[0] / n)
        s = f32(moments[1] / n)
        d = fmax(f32(s - f32(lm * lm)), F(0))
        v = f32(d / (nu_a - np.uint64(1)).astype(F))
        e = f32(np.sqrt(v))
        r = fmax(lm, F(floor))
        t = f32(F(threshold) * r)
        hit = e > t
    return (nu < max_passes) & ((nu < min_passes) | hit)


def select(moments, extra, **rec):
    """-> the list, uint32 ascending."""
    return np.nonzero(predicate(moments, extra, **rec))[0].astype(U32)


def accumulate_list(pass_planes, lst, film, moments, extra):
    """apt_film_accumulate_list_* on copies -> (film, moments, extra); lst without repeats among its entries inside the image."""
    pass_planes, film, moments = f32(np.asarray(pass_planes)), f32(np.array(film, copy=True)), f32(np.array(moments, copy=True))
    extra, lst = np.array(extra, dtype=U32, copy=True), np.asarray(lst, dtype=U32)
    n = film.shape[1]
    assert pass_planes.shape == (3, lst.size) and moments.shape == (2, n) and extra.shape == (n,)
    keep = lst < n
    p = lst[keep].astype(np.int64)
    assert np.unique(p).size == p.size
    pp = pass_planes[:, keep]
    with np.errstate(all="ignore"):
        film[:, p] = f32(film[:, p] + pp)
        l = lum(pp[0], pp[1], pp[2])
        moments[0, p] = f32(moments[0, p] + l)
        moments[1, p] = f32(moments[1, p] + f32(l * l))
    extra[p] += U32(1)
    return film, moments, extra


def mean(film, base, extra=None):
    film = f32(np.asarray(film))
    k = np.uint64(base) + (np.zeros(film.shape[1], dtype=np.uint64) if extra is None else np.asarray(extra).astype(np.uint64))
    with np.errstate(all="ignore"):
        return f32(film / k.astype(F)[None, :])


def moments_of(passes):
    """The luminance moments of whole passes (render_mi355x_denoise.h "Moments") -> [2][N]."""
    m = None
    for p in passes:
        l = lum(p[0], p[1], p[2])
        cur = np.stack([l, f32(l * l)])
        m = cur if m is None else f32(m + cur)
    return m


def list_pass(whole_pass, lst):
    """What a list launch stores for `lst`, given the planes [3][N] of the whole pass of the same index: a gather.  Entries beyond the
    image have no value: NaN here, and the tests compare the other slots."""
    lst = np.asarray(lst, dtype=np.int64)
    n = whole_pass.shape[1]
    out = np.full((3, lst.size), np.nan, dtype=F)
    ok = lst < n
    out[:, ok] = whole_pass[:, lst[ok]]
    return out


def render_list_pass(params, spheres, materials, lst, pass_index, **kw):
    """A list pass from scratch: film_ref.render_pass of the whole frame, gathered -> planes [3][len(lst)]."""
    planes, _ = fr.render_pass(params, spheres, materials, pass_index=pass_index, **kw)
    return list_pass(planes, lst)


# ---- the three wrong list renderers a test list must tell from the right one -------------------------------------------------------------
def wrong_compact_index(whole_pass, lst):
    """The compact index used as the pixel."""
    return whole_pass[:, np.arange(len(lst)) % whole_pass.shape[1]]


def wrong_late_read(whole_pass, lst):
    """The list read one entry late (the last lane wraps to entry 0)."""
    return list_pass(whole_pass, np.roll(np.asarray(lst), -1))


def sensitive(lst, pass0, passk):
    """Is `lst` a list on which the three wrong renderers -- the compact index as the pixel, pass 0's seed for every round, the list
    read one entry late -- all differ from the right one?  pass0, passk: whole-frame planes of pass 0 and of the pass the list renders."""
    right = list_pass(passk, lst)
    ok = np.asarray(lst) < passk.shape[1]
    differs = lambda other: not np.array_equal(right[:, ok].view(U32), other[:, ok].view(U32))
    return differs(wrong_compact_index(passk, lst)) and differs(list_pass(pass0, lst)) and differs(wrong_late_read(passk, lst))


# ---- the synthetic films and predicates the CPU and the GPU tests of the library share ----------------------------------------------------
REC = dict(base=3, min_passes=4, max_passes=9, threshold=0.125, floor=0.25)


def synthetic(n, kind, seed=11):
    """-> (film [3][n], moments [2][n], extra [n]) whose selection under REC is of the `kind`: "none", "all", "alternating", "random",
    "threshold" (pixels with e == t exactly, and their two neighbours in m1), "nan" (NaN moments and NaN film values), "counts"
    (extra at min_passes - 1, min_passes, max_passes - 1, max_passes around base), "floor" (dark pixels that only the floor decides)."""
    rng = np.random.default_rng(seed + n)
    base, lo, hi = REC["base"], REC["min_passes"], REC["max_passes"]
    film = rng.random((3, n)).astype(F) * F(4)
    extra = np.full(n, lo - base + 1, dtype=U32)                       # n_u = 5: inside the arithmetic
    nu = F(base) + extra.astype(F)
    lm = (rng.random(n).astype(F) + F(0.5))                           # mean luminance in [0.5, 1.5)
    m0 = f32(lm * nu)
    quiet = f32(f32(lm * lm) * nu)                                    # s ~ lm^2: d ~ 0
    loud = f32(quiet * F(3))                                          # d = 2 lm^2: e = lm * sqrt(2 / (n_u - 1)) > 0.125 lm
    if kind == "none":
        m1 = quiet
        m1 = f32(m1 * F(0.5))                                         # s < lm^2: d clamps to 0
    elif kind == "all":
        m1 = loud
    elif kind == "alternating":
        m1 = np.where(np.arange(n) % 2 == 0, loud, f32(quiet * F(0.5))).astype(F)
    elif kind == "random":
        m1 = np.where(rng.random(n) < 0.3, loud, f32(quiet * F(0.5))).astype(F)
        extra = rng.integers(0, hi - base + 2, n).astype(U32)
    elif kind == "threshold":
        # n_u = 5, lm = 1 (m0 = 5), floor below: t = 0.125; e = sqrt(d / 4) == 0.125 <=> d = 1/16 <=> s = 1.0625, m1 = 5.3125: all exact
        m0 = np.full(n, 5.0, dtype=F)
        m1 = np.full(n, 5.3125, dtype=F)
        m1[1::3] = np.nextafter(F(5.3125), F(9))                      # just above: selected, if the quotient moves at all
        m1[2::3] = np.nextafter(F(5.3125), F(0))
    elif kind == "nan":
        m1 = loud.copy()
        m0 = m0.copy()
        m0[0::4] = np.nan
        m1[1::4] = np.nan
        film[:, 2::4] = np.nan
        extra[3::8] = 0                                               # n_u = 3 < min_passes: selected whatever the moments are
        m0[3::8] = np.nan
    elif kind == "counts":
        m1 = loud
        around = np.array([lo - 1, lo, hi - 1, hi, hi + 1], dtype=np.int64) - base
        extra = around[np.arange(n) % around.size].astype(U32)
        m1 = np.where(np.arange(n) % 2 == 0, loud, f32(quiet * F(0.5))).astype(F)
    elif kind == "floor":
        # dark pixels: lm = 1/64, relative error large -> selected with floor 0, not with floor 0.25 (t = 0.125 * 0.25 > e)
        lm = np.full(n, 1.0 / 64.0, dtype=F)
        nu = np.full(n, 5.0, dtype=F)
        m0 = f32(lm * nu)
        m1 = f32(f32(f32(lm * lm) * nu) * F(2))                       # d = lm^2, e = lm / 2 = 1/128 > 0.125 / 64 and < 0.125 / 4
    else:
        raise ValueError(kind)
    return film, np.stack([m0, m1]).astype(F), extra


KINDS = ("none", "all", "alternating", "random", "threshold", "nan", "counts", "floor")


# ---- the host twins on NumPy buffers --------------------------------------------------------------------------------------------------------
def record(apt, **rec):
    r = apt._lib.film_select_record(rec["base"], **{k: v for k, v in rec.items() if k != "base"})
    return r


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def select_host(apt, moments, extra, rec, guard=7):
    """apt_film_select_host -> (rc, list[:count], count, untouched): list and work sit inside guard words."""
    L = apt._lib.adaptive_lib()
    n = moments.shape[1]
    moments, extra = np.ascontiguousarray(moments, dtype=F), np.ascontiguousarray(extra, dtype=U32)
    lst = np.full(n + 2 * guard, 0xDEADBEEF, dtype=U32)
    work = np.full(L.apt_film_select_work_words(n) + 2 * guard, 0xDEADBEEF, dtype=U32)
    count = np.full(1, 0xDEADBEEF, dtype=U32)
    rc = L.apt_film_select_host(ctypes.byref(rec), _p(moments), _p(extra), n, ctypes.c_void_p(work.ctypes.data + 4 * guard),
                                ctypes.c_void_p(lst.ctypes.data + 4 * guard), _p(count))
    c = int(count[0]) if rc == 0 else 0
    body = lst[guard:guard + n]
    untouched = bool(np.all(lst[:guard] == 0xDEADBEEF) and np.all(lst[guard + n:] == 0xDEADBEEF) and np.all(body[c:] == 0xDEADBEEF)
                     and np.all(work[:guard] == 0xDEADBEEF) and np.all(work[-guard:] == 0xDEADBEEF))
    return rc, body[:c].copy(), int(count[0]), untouched


def accumulate_list_host(apt, pass_planes, lst, film, moments, extra, n=None, guard=5):
    """apt_film_accumulate_list_host on copies that sit inside guard words -> (rc, film, moments, extra, guards intact)."""
    L = apt._lib.adaptive_lib()
    n = film.shape[1] if n is None else n
    lst = np.ascontiguousarray(lst, dtype=U32)
    pass_planes = np.ascontiguousarray(pass_planes, dtype=F)
    blocks = []
    for a, dt, fill in ((film, F, F(-7)), (moments, F, F(-7)), (extra, U32, U32(0xDEADBEEF))):
        b = np.full(a.size + 2 * guard, fill, dtype=dt)
        b[guard:guard + a.size] = np.ascontiguousarray(a, dtype=dt).ravel()
        blocks.append(b)
    ptr = [ctypes.c_void_p(b.ctypes.data + 4 * guard) for b in blocks]
    rc = L.apt_film_accumulate_list_host(_p(pass_planes), _p(lst), lst.size, n, *ptr)
    intact = all(np.all(b[:guard] == b[0]) and np.all(b[-guard:] == b[0]) and (b[0] == fill)
                 for b, fill in zip(blocks, (F(-7), F(-7), U32(0xDEADBEEF))))
    f, m, e = (b[guard:-guard].copy() for b in blocks)
    return rc, f.reshape(film.shape), m.reshape(moments.shape), e, bool(intact)


def mean_host(apt, film, base, extra=None):
    L = apt._lib.adaptive_lib()
    film = np.ascontiguousarray(film, dtype=F)
    n = film.shape[1]
    out = np.full((3, n), -7.0, dtype=F)
    rc = L.apt_film_mean_host(_p(film), _p(None if extra is None else np.ascontiguousarray(extra, dtype=U32)), base, n, _p(out))
    return rc, out


def assert_same(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    view = np.uint32 if got.dtype.itemsize == 4 else np.uint8
    diff = np.argwhere(got.view(view) != want.view(view))
    assert diff.size == 0, (diff.shape[0], diff[:5], got[tuple(diff[0])], want[tuple(diff[0])])


def bits_differ(a, b):
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return a.shape != b.shape or not np.array_equal(a.view(U32), b.view(U32))


# ---- the lists of the GPU tests of a list pass (tests/test_gpu_film_list.py), and what tests/test_adaptive_cpu.py holds them to ----------
def gpu_lists(npix):
    """name -> uint32 list for an image of npix pixels (1536 = 48 x 32, or 384 = 24 x 16).  "all" is every pixel in order; "one" a
    single entry that is not pixel 0; the strided ones wrap round the image, so they are neither contiguous nor monotonic; 17 entries
    end inside the first wave at GROUP 8 (2 pixels a wave) and GROUP 1 (16 a wave) alike, 1001 leave a ragged last workgroup."""
    a = np.arange(npix, dtype=np.int64)
    many = min(1001, npix - npix // 4 - 1)
    lists = {"all": a, "one": np.array([npix // 2 + 3]), "strided17": (11 + 89 * a[:17]) % npix, "strided%d" % many: (7 + 5 * a[:many]) % npix,
             "descending": a[::-1][::3], "repeat": npix // 2 + np.array([9, 40, 9, 3, 40, 77, 9])}
    return {k: v.astype(U32) for k, v in lists.items()}
