"""NumPy float64 restatement of the camera (include/render_mi355x.h "camera"), for the tests only: the record builders
(apt_camera_default_host / apt_camera_build_host) and ray generation in the general form with the thin lens.

Every operation is one separately rounded float64 NumPy operation in the header's order; the norms are np.linalg.norm's FMA chain
(norm3_sq of pt_core.h) with fma() taken from libm through ctypes (Python 3.10 has no math.fma).  The two path uniforms come from the
oracle's counter generator (existing, exact), the lens's fp32 part from materials_ref (uniforms, sincos).  rays() gives [6][N] float32,
which go through materials_ref.trace and oracle.decode_color for frames.
"""
import ctypes
import ctypes.util

import numpy as np

import materials_ref as mr

F, D, U = np.float32, np.float64, np.uint64
LENS_SALT = 0xA54FF53A5F1D36F1

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
assert _libm.fma(1 + 2.0 ** -30, 1 + 2.0 ** -30, -(1 + 2.0 ** -29)) == 2.0 ** -60    # a true FMA: the product is not rounded first


def fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, D), np.asarray(b, D), np.asarray(c, D))
    out = np.fromiter((_libm.fma(x, y, z) for x, y, z in zip(a.ravel().tolist(), b.ravel().tolist(), c.ravel().tolist())), D, a.size)
    return out.reshape(a.shape)


def norm3_sq(x, y, z):
    return fma(z, z, fma(y, y, np.asarray(x, D) * np.asarray(x, D)))


def norm3(x, y, z):
    return np.sqrt(norm3_sq(x, y, z))


def cross(p, q):
    return [p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]]


FIELDS = ("pos", "g", "cx", "cy", "offset", "aperture", "focus", "lens_u", "lens_v", "offset_over_focus")


def _record(**kw):
    rec = {k: (np.array([D(x) for x in v], dtype=D) if k in ("pos", "g", "cx", "cy", "lens_u", "lens_v") else D(v)) for k, v in kw.items()}
    assert set(rec) == set(FIELDS)
    return rec


def default_record(w, h):
    """camera_init (pt_core.h; scripts/gen_data.py:24-30) as a record."""
    pos = [D(50), D(52), D(295.6)]
    dirv = [D(0), D(-0.042612), D(-1)]
    n = norm3(*dirv)
    g = [x / n for x in dirv]
    cx = [D(w) * D(0.5135) / D(h), D(0), D(0)]
    cr = cross(cx, g)
    cn = norm3(*cr)
    lens_v = [x / cn for x in cr]
    cy = [x * D(0.5135) for x in lens_v]
    return _record(pos=pos, g=g, cx=cx, cy=cy, offset=140.0, aperture=0.0, focus=0.0, lens_u=[1.0, 0.0, 0.0], lens_v=lens_v,
                   offset_over_focus=0.0)


def build_record(eye, dirv, up, scale, offset, aperture, focus, w, h):
    """apt_camera_build_host, operation by operation."""
    eye, dirv, up = [D(x) for x in eye], [D(x) for x in dirv], [D(x) for x in up]
    scale, offset, aperture, focus = D(scale), D(offset), D(aperture), D(focus)
    gn = norm3(*dirv)
    g = [x / gn for x in dirv]
    c = cross(g, up)
    cn = np.sqrt(norm3_sq(*c))
    right = [x / cn for x in c]
    sx = (D(w) * scale) / D(h)
    cx = [x * sx for x in right]
    e = cross(cx, g)
    en = norm3(*e)
    lens_v = [x / en for x in e]
    cy = [x * scale for x in lens_v]
    return _record(pos=eye, g=g, cx=cx, cy=cy, offset=offset, aperture=aperture, focus=focus, lens_u=right, lens_v=lens_v,
                   offset_over_focus=(offset / focus) if aperture > 0 else 0.0)


def record_bytes(rec):
    """The record as apt_camera lays it out (struct_size 184, reserved 0, then the doubles in FIELDS order)."""
    body = np.concatenate([np.atleast_1d(np.asarray(rec[k], dtype=D)) for k in FIELDS])
    assert body.size == 22
    return np.array([8 + 8 * body.size, 0], dtype=np.uint32).tobytes() + body.tobytes()


def from_ctypes(cam):
    """An ApCamera -> a record (so that the ray restatement can run on what the library built)."""
    return _record(**{k: (list(getattr(cam, k)) if k in ("pos", "g", "cx", "cy", "lens_u", "lens_v") else getattr(cam, k)) for k in FIELDS})


def tent(u):
    r = D(2) * u
    lower = r < 1
    x = np.where(lower, r, D(2) - r)
    t = np.sqrt(x) - D(1)
    return np.where(lower, t, -t)


def image_coords(w, h, s, seed, paths):
    """(a, b) of the given path indices: render_frame's tent-filtered image-plane coordinates."""
    from oracle import oracle
    paths = np.asarray(paths, dtype=np.int64)
    r = paths // s
    sx, sy = r & 1, (r >> 1) & 1
    r = r >> 2
    j, i = r % h, r // h
    u = np.empty((paths.size, 2), dtype=D)
    if paths.size and (np.diff(paths) == 1).all():
        u[:] = oracle.path_uniforms(seed, int(paths[0]), paths.size)
    else:
        for n, p in enumerate(paths.tolist()):
            u[n] = oracle.path_uniforms(seed, p, 1)[0]
    ddx, ddy = tent(u[:, 0]), tent(u[:, 1])
    xa = (sx.astype(D) + D(0.5) + ddx) / D(2) + i.astype(D)
    xb = (sy.astype(D) + D(0.5) + ddy) / D(2) + j.astype(D)
    return xa / D(w) - D(0.5), xb / D(h) - D(0.5)


def lens_points(rec, seed, paths):
    """(lx, ly) float32 of the given paths: the lens's own stream, DIFF's sqrt and polynomial."""
    key = mr.splitmix64(U(seed) ^ mr.splitmix64(np.asarray(paths, dtype=U)) ^ U(LENS_SALT))
    v1, v2 = mr.uniforms(key, 0)
    r = np.sqrt(v1)
    sn, cs = mr.sincos(v2)
    ap = F(rec["aperture"])
    return mr.f32((cs * r) * ap, (sn * r) * ap)


def rays_ab(rec, a, b, lx=None, ly=None):
    """The rays of image-plane coordinates (a, b) (float64 arrays) and lens points (lx, ly) (float32; read when aperture > 0)
    -> float32 [6][n]."""
    a, b = np.asarray(a, D), np.asarray(b, D)
    d = [(rec["cx"][k] * a + rec["cy"][k] * b) + rec["g"][k] for k in range(3)]
    if rec["aperture"] > 0:
        dlx, dly = np.asarray(lx, F).astype(D), np.asarray(ly, F).astype(D)
        s = [rec["pos"][k] + (rec["lens_u"][k] * dlx + rec["lens_v"][k] * dly) for k in range(3)]
        v = [(rec["pos"][k] + d[k] * rec["focus"]) - s[k] for k in range(3)]
        t = rec["offset_over_focus"]
    else:
        s = [np.full(a.shape, rec["pos"][k], dtype=D) for k in range(3)]
        v, t = d, rec["offset"]
    n = norm3(*v)
    out = [(s[k] + v[k] * t).astype(F) for k in range(3)] + [(v[k] / n).astype(F) for k in range(3)]
    assert all(x.dtype == D for x in d + v + [n])
    return np.stack(out)


def rays(rec, w, h, s, seed=0, path_begin=0, path_count=None):
    """float32 [6][path_count] for paths [path_begin, path_begin + path_count) of a w x h image with `s` samples."""
    n = w * h * 4 * s
    if path_count is None:
        path_count = n - path_begin
    paths = np.arange(path_begin, path_begin + path_count, dtype=np.int64)
    a, b = image_coords(w, h, s, seed, paths)
    lx, ly = lens_points(rec, seed, paths) if rec["aperture"] > 0 else (None, None)
    return rays_ab(rec, a, b, lx, ly)
