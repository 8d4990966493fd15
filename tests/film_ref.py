"""NumPy restatement of the film (include/render_mi355x.h "film": an unclipped float32 accumulation buffer filled pass by pass, and its
resolve), for the tests only.

A pass is tests/materials_ref.py's trace with the pass's seed and the oracle's decode_color, whose `pre` -- the float64 mean before the clip --
is rounded once to float32.  The film is the sequential float32 sum of the passes.  The resolve is float32 NumPy, one separately
rounded operation per step in the header's order, and np.searchsorted in the curve table.  As in the other restatements f32() fails on
a float64 intermediate."""
import re

import numpy as np

import materials_ref as mr
from materials_ref import F, ROOT, U, f32, splitmix64

TONEMAP_CLIP, TONEMAP_REINHARD = 0, 1
CURVE_LINEAR, CURVE_SRGB = 0, 1


def _pass_salt():
    import os
    text = open(os.path.join(ROOT, "include", "render_mi355x.h")).read()
    return int(re.search(r"#define APT_FILM_PASS_SALT\s+(0x[0-9A-Fa-f]+)ull", text).group(1), 16)


PASS_SALT = _pass_salt()
# every stream salt of the header: the bounce's, APT_FLAG_NEE's, the light table's, the lens's, the sun's; roulette has none
assert PASS_SALT not in (0, 0x6A09E667F3BCC909, 0xBB67AE8584CAA73B, 0x3C6EF372FE94F82B, 0xA54FF53A5F1D36F1, int(mr.SUN_SALT))


def pass_seed(seed, k):
    """apt_film_pass_seed -> int: pass 0 is the seed itself."""
    if k == 0:
        return int(seed)
    with np.errstate(over="ignore"):
        return int(splitmix64(U(seed) ^ splitmix64(U(k) ^ U(PASS_SALT))))


def render_pass(params, spheres, materials, env=None, table=None, pass_index=0, rays=None, pixel_begin=0, pixel_count=None):
    """One pass of `params` (an oracle.Params; its seed is the film's base seed, its flags are read by materials_ref.trace_params) ->
    (float32 planes [3][count], segments).  rays: a callable seed -> camera rays (camera_ref.rays with the pass's seed), or None: the
    reference camera's."""
    from oracle import oracle
    q = oracle.Params.from_buffer_copy(bytes(params))
    q.seed = pass_seed(params.seed, pass_index)
    w, h, s = q.width, q.height, q.samples
    r = oracle.gen_rays_counter(q) if rays is None else rays(q.seed)
    L, bad, seg = mr.trace_params(q, r, spheres, materials, env, table)
    assert not bad.any()
    pre = oracle.decode_color(L, w, h, s)[0]                   # float64 [W*H][3]: the mean before the clip
    assert pre.dtype == np.float64
    planes = np.ascontiguousarray(pre.T).astype(F)
    if pixel_count is None:
        pixel_count = w * h - pixel_begin
    return planes[:, pixel_begin:pixel_begin + pixel_count], seg


def accumulate(passes):
    """The film after the passes (float32 planes, in order): pass 0 stored, every later one added in one float32 add."""
    film = f32(np.array(passes[0], dtype=F, copy=True))
    for p in passes[1:]:
        film = f32(film + f32(p))
    return film


def resolve(film, passes, exposure, tonemap, inv_white2, table):
    """-> (out float32 like film, u8 [count][3]) of apt_film_resolve_* for a [3][count] film."""
    assert 1 <= passes <= 1 << 24
    film, table = f32(np.asarray(film)), f32(np.asarray(table))
    with np.errstate(all="ignore"):
        m = f32(film / F(passes))
        x = f32(m * F(exposure))
        x = f32(np.where(x > F(0), x, F(0)))
        y = x
        if tonemap == TONEMAP_REINHARD:
            t = f32(x * F(inv_white2))
            t = f32(F(1) + t)
            num = f32(x * t)
            den = f32(F(1) + x)
            y = f32(np.where(x == F(np.inf), F(1), f32(num / den)))
        else:
            assert tonemap == TONEMAP_CLIP
        y = f32(np.where(y < F(1), y, F(1)))
    # #{k in 1..255 : table[k] <= y}; the 8 steps of the header, which is searchsorted for an increasing table
    code = np.zeros(y.shape, dtype=np.int64)
    for b in (128, 64, 32, 16, 8, 4, 2, 1):
        code = code + np.where(table[code + b] <= y, b, 0)
    if np.all(np.diff(table[1:]) > 0):
        assert np.array_equal(code, np.searchsorted(table[1:], y, side="right"))
    return y, np.ascontiguousarray(code.reshape(3, -1).T).astype(np.uint8)


def curve(which):
    """apt_film_curve_host's table from the float64 formula in NumPy (libm's and NumPy's pow may differ in the last double bit: the
    tests allow one float32 ulp)."""
    k = np.arange(1, 256, dtype=np.float64)
    e = (k - 0.5) / 255.0
    v = e if which == CURVE_LINEAR else np.where(e <= 0.04045, e / 12.92, ((e + 0.055) / 1.055) ** 2.4)
    return np.concatenate([[0.0], v]).astype(F)


# ---- what the CPU and the GPU tests of the resolve share --------------------------------------------------------------------------
def value_pool(tables):
    """The values the resolve is held to: zeros, negatives, NaN, infinities, denormals, exactly 1, large ones, and every entry of both
    tables with its two neighbours."""
    special = [0.0, -0.0, -1.0, -1e-40, np.nan, np.inf, -np.inf, 1e-45, 1e-40, 1.1754944e-38, 1.0, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2)),
               0.5, 2.0, 3.0, 15.0, 16.0, 17.0, 1e4, 1e19, 1e20, 3e38, 3.4028235e38]
    vals = [np.array(special, dtype=F)]
    for t in tables:
        vals += [t, np.nextafter(t, F(2)), np.nextafter(t, F(-1))]
    return np.concatenate(vals).astype(F)


def resolve_host(apt, film, passes, exposure, tonemap, inv_white2, table, offset=0, want_out=True, want_u8=True):
    """apt_film_resolve_host on a [3][n] film -> (rc, out, u8, guards intact); the 8-bit image sits `offset` bytes into an aligned block."""
    L = apt._lib.lib()
    import ctypes
    film = np.ascontiguousarray(film, dtype=F)
    n = film.shape[1]
    rec = apt._lib.film_resolve_record(passes, exposure, tonemap, inv_white2)
    out = np.full((3, n), -7.0, dtype=F)
    block = np.full(3 * n + 16, 0xA5, dtype=np.uint8)
    base = block.ctypes.data + offset
    assert block.ctypes.data % 4 == 0
    rc = L.apt_film_resolve_host(ctypes.byref(rec), film.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                                 table.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p) if want_out else None,
                                 ctypes.c_void_p(base) if want_u8 else None)
    guards = np.all(block[:offset] == 0xA5) and np.all(block[offset + 3 * n:] == 0xA5)
    return rc, out, block[offset:offset + 3 * n].reshape(n, 3).copy(), guards
