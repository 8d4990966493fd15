"""Shared by the tests of the first-bounce plan (csrc/pt_first_plan.h); no test in it.

  * one loader for the plan's CPU twin, libfirstplan_mi355x.so: prototypes, record(), camera(), masks();
  * the float32 restatement of the first bounce's keys (first_bounce_keys) and the jitter set of a pixel's footprint (jitters);
  * THE FAMILY: tables and cameras, deterministic from a seed, that vary everything the header's premises leave free -- the shared
    planes, the walls' radii (ends of the allowed range included) and near faces, a ball that is ordinary, tiny, huge, far away or
    sitting on the origins, a light of radius 10 .. 1e7 that protrudes through the top or the bottom face, lies inside the room or
    wholly outside, eps from 1e-4 to 1, and a camera that is the reference's or a moved and rescaled one of the same frame pattern.
    Some members break a premise (the moved origins leave the room, a near face comes too close): the twin must refuse those with
    the all-zero record, and the tests bound how many may be refused so that the family cannot go hollow."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-4
RULE_BITS = (0, 1, 3, 4, 5, 6, 7)      # sphere 2, the wall the camera looks at, has no rule
WORDS = 16                             # kFirstPlanWords; entries 14 and 15 are unused and zero

_twin = None


def twin():
    """libfirstplan_mi355x.so with its prototypes (built by __graft_entry__.build())."""
    global _twin
    if _twin is None:
        import __graft_entry__ as g
        g.build()
        L = ctypes.CDLL(os.path.join(ROOT, "ascendpathtracing_amd", "libfirstplan_mi355x.so"))
        L.apt_first_plan_host.restype = ctypes.c_int
        L.apt_first_plan_host.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
        L.apt_first_plan_camera_host.restype = ctypes.c_int
        L.apt_first_plan_camera_host.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
        L.apt_first_plan_mask_host.restype = ctypes.c_uint32
        L.apt_first_plan_mask_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        _twin = L
    return _twin


def reference_table():
    from ascendpathtracing_amd import gen_data
    return np.ascontiguousarray(gen_data.gen_spheres(), dtype=np.float32)


def camera(L, w, h):
    """The reference's camera for a w x h frame: pos, g, cx, cy (12 doubles)."""
    cam = np.zeros(12)
    assert L.apt_first_plan_camera_host(w, h, cam.ctypes.data) == 0
    return cam


def record(L, w, h, sph, cam=None, eps=EPS):
    sph = np.ascontiguousarray(sph, dtype=np.float32)
    rec = np.full(WORDS, -1, dtype=np.int32)
    assert L.apt_first_plan_host(w, h, sph.ctypes.data, eps, None if cam is None else cam.ctypes.data, rec.ctypes.data) == 0
    return rec


def masks(L, rec, w, h, cols, rows):
    """-> uint32 [len(cols), len(rows)]: apt_first_plan_mask_host of every (column, row)."""
    rec = np.ascontiguousarray(rec, dtype=np.int32)
    return np.array([[L.apt_first_plan_mask_host(rec.ctypes.data, w, h, int(c), int(r)) for r in rows] for c in cols], dtype=np.uint32)


def jitters(rng, n):
    """Offsets inside a pixel, camera_ray_t's ((s + 0.5 + tent) / 2 with s in {0, 1}, tent in [-1, 1)): the footprint's corners and
    edges first, then uniform ones."""
    lo, hi = -0.25, np.nextafter(1.25, 0.0)
    edge = np.array([lo, hi, 0.0, 0.5, 1.0])
    gx, gy = np.meshgrid(edge, edge, indexing="ij")
    fx = np.concatenate([gx.ravel(), rng.uniform(lo, hi, n), np.full(n // 8, lo), np.full(n // 8, hi), rng.uniform(lo, hi, n // 4)])
    fy = np.concatenate([gy.ravel(), rng.uniform(lo, hi, n), rng.uniform(lo, hi, n // 4), np.full(n // 8, lo), np.full(n // 8, hi)])
    return fx, fy


def first_bounce_keys(cam, w, h, sph, cols, rows, fx, fy, eps=EPS):
    """-> keys [pixel, jitter, sphere] (inf: no accepted root), float32 arithmetic in the kernel's order."""
    pos, g, cx, cy = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    a = (cols[:, None] + fx[None, :]) / w - 0.5
    b = (rows[:, None] + fy[None, :]) / h - 0.5
    d = np.stack([cx[k] * a + cy[k] * b + g[k] for k in range(3)], axis=-1)            # gen_data.py:41-43, float64
    o = (pos + d * 140).astype(np.float32)
    d = (d / np.sqrt((d * d).sum(-1, keepdims=True))).astype(np.float32)
    f = np.float32
    r2, C = sph[0:8], np.stack([sph[8:16], sph[16:24], sph[24:32]], axis=-1)
    t = C[None, None, :, :] - o[:, :, None, :]                                           # c - o, per coordinate
    p = t * d[:, :, None, :]
    q = t * t
    bb = (p[..., 0] + p[..., 1]) + p[..., 2]
    cc = ((q[..., 0] + q[..., 1]) + q[..., 2]) - r2[None, None, :]
    assert bb.dtype == f and cc.dtype == f
    disc = bb * bb - cc
    with np.errstate(invalid="ignore", over="ignore"):
        root = np.sqrt(disc)
        t0, t1 = bb - root, bb + root
        k0 = np.where(t0 > f(eps), t0, f(np.inf))
        k1 = np.where(t1 > f(eps), t1, f(np.inf))
    return np.minimum(k0, k1)


# ---- the family ------------------------------------------------------------------------------------------------------------
FAMILY_EPS = (1e-4, 1e-2, 0.3, 1.0)
FAMILY_SHAPES = ((33, 19), (64, 36), (1, 40), (40, 1), (128, 8), (8, 128), (17, 31), (3, 5), (2, 2), (1, 1))
BALL_KINDS = ("ordinary", "tiny", "huge", "far", "origins")
REF_POS = np.array([50.0, 52.0, 295.6])
REF_DIR = np.array([0.0, -0.042612, -1.0])


def family_table(rng):
    """One table of the family: float32 [128], the reference table with the eight spheres' r2, x, y, z replaced."""
    t = np.array(reference_table(), dtype=np.float64)[:80].reshape(10, 8)
    X, Y, Z = 50 + rng.uniform(-20, 20), 40.8 + rng.uniform(-15, 15), 81.6 + rng.uniform(-30, 30)
    R = rng.uniform(5e4, 1.3e5, 6)
    if rng.random() < 0.3:                                   # one radius exactly at an end of the range the header allows
        R[rng.integers(6)] = rng.choice([5e4, 1.3e5])
    xlo, xhi = rng.uniform(-60, 20), rng.uniform(80, 160)    # the near faces
    ylo, yhi = rng.uniform(-60, 5), rng.uniform(75, 200)
    zlo, zhi = rng.uniform(-200, 10), rng.uniform(165, 400)
    # spheres 0 / 1 beyond +x / -x, 2 / 3 beyond +z / -z, 4 / 5 beyond +y / -y
    centres = [(xlo + R[0], Y, Z), (xhi - R[1], Y, Z), (X, Y, zlo + R[2]), (X, Y, zhi - R[3]), (X, ylo + R[4], Z), (X, yhi - R[5], Z)]
    for k in range(6):
        t[0, k], t[1:4, k] = R[k] ** 2, centres[k]
    kind = BALL_KINDS[rng.integers(5)]
    near = np.array([rng.uniform(xlo - 30, xhi + 30), rng.uniform(ylo - 30, yhi + 30), rng.uniform(zlo - 30, zhi + 30)])
    if kind == "ordinary":
        br, bc = rng.uniform(1, 40), near
    elif kind == "tiny":
        br, bc = rng.uniform(0.05, 2), near
    elif kind == "huge":
        br, bc = rng.uniform(40, 120), near
    elif kind == "far":                                      # 1e3 .. 8e8 away, a radius of up to nearly that distance
        bc = rng.uniform(-1, 1, 3) * 10 ** rng.uniform(3, 8.9)
        br = 10 ** rng.uniform(-1, 0.95 * np.log10(np.abs(bc).max()))
    else:                                                    # on the origins pos + 140 d, or behind them towards the camera
        g = REF_DIR / np.linalg.norm(REF_DIR)
        d = g + np.array([rng.uniform(-0.45, 0.45), rng.uniform(-0.25, 0.25), 0.0])
        br, bc = rng.uniform(1, 40), REF_POS + d * rng.uniform(60, 150)
    t[0, 6], t[1:4, 6] = br * br, bc
    lr = 10 ** rng.uniform(1, 7)
    ly = rng.choice([yhi + lr - rng.uniform(0, 5),           # just protruding through the +y face
                     ylo - lr + rng.uniform(0, 5),           # just through the -y face
                     rng.uniform(ylo, yhi),                  # inside the room
                     yhi + lr + rng.uniform(0, 50)])         # wholly outside
    t[0, 7], t[1:4, 7] = lr * lr, (X, ly, Z)
    out = np.zeros(128, dtype=np.float32)
    out[:80] = t.astype(np.float32).ravel()
    return out


def family_camera(rng, w, h):
    """Half the cases: the reference's camera.  The others: pos moved by up to 8 per axis, cx[0] and cy[1..2] rescaled by 0.6 .. 1.6
    (the frame pattern cx = (., 0, 0), cy = (0, ., .), g = (0, ., .) is kept)."""
    cam = camera(twin(), w, h)
    if rng.random() < 0.5:
        cam[0:3] += rng.uniform(-8, 8, 3)
        cam[6] *= rng.uniform(0.6, 1.6)
        cam[10:12] *= rng.uniform(0.6, 1.6)
    return cam


def line_disc(cam, w, h, sph, k, cols, rows, fx, fy):
    """-> float64 [pixel, jitter]: the exact discriminant of sphere k for the LINE through cam.pos along each camera ray,
    N^2 / |d|^2 - (|w|^2 - r2) with w = C - pos, N = w . d -- the quantity the header's BALL RULE bounds by -(4 + r2 * 2^-12).
    Also the ray's own c and b from its origin pos + 140 d (the LIGHT RULE's second form): -> (disc, c, b)."""
    pos, g, cx, cy = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    a = (cols[:, None] + fx[None, :]) / w - 0.5
    b = (rows[:, None] + fy[None, :]) / h - 0.5
    d = np.stack([cx[i] * a + cy[i] * b + g[i] for i in range(3)], axis=-1)
    C, r2 = np.array([sph[8 + k], sph[16 + k], sph[24 + k]], dtype=np.float64), float(sph[k])
    wv = C - pos
    n2 = (d * d).sum(-1)
    N = (d * wv).sum(-1)
    disc = N * N / n2 - ((wv * wv).sum() - r2)
    t = C - (pos + 140 * d)
    return disc, (t * t).sum(-1) - r2, (t * d).sum(-1) / np.sqrt(n2)


GRAZING_SHAPES = ((64, 36), (33, 19), (8, 128), (17, 31), (128, 8))


def grazing_case(seed, index):
    """A member made to sit where the ball rule's margin decides: a family room whose ball is a huge one (radius R of a few hundred to
    some ten thousand) placed so that its silhouette, seen from cam.pos, runs along the footprint edge of the n-th row from the top
    or from the bottom, at a distance of 0.3 of the margin 4 + r2 * 2^-12 in units of the discriminant.  The rows beyond that edge
    miss the ball in exact arithmetic, by less than the margin: a rule without the margin marks them, the header's rule must not.
    -> (table, eps, (w, h), camera, (side, n)): side 0 = the first n rows, 1 = the last n rows."""
    rng = np.random.default_rng([int(seed), int(index), 77])
    sph = family_table(rng)
    eps = float(FAMILY_EPS[rng.integers(len(FAMILY_EPS))])
    w, h = GRAZING_SHAPES[index % len(GRAZING_SHAPES)]
    cam = family_camera(rng, w, h)
    side, n = int(index // len(GRAZING_SHAPES)) % 2, int(rng.integers(1, 3))
    pos, g, cy = cam[0:3], cam[3:6], cam[9:12]
    T = rng.uniform(165, 250)                               # cam.pos to the point of tangency: beyond the origins, inside the room
    R = T * h / (4 * (n + 0.5))                             # the band of lines that miss the ball is wide enough for the n rows
    margin = 4 + R * R * 2.0 ** -12
    edge = (n + 0.25) / h - 0.5 if side == 0 else (h - n - 0.25) / h - 0.5
    inward = 1.0 if side == 0 else -1.0                     # from the n rows towards the ball, in b
    db = np.array([0.0, cy[1], cy[2]])

    def unit(b):
        d = np.array([0.0, cy[1] * b + g[1], cy[2] * b + g[2]])
        return d / np.linalg.norm(d), np.linalg.norm(d)

    u, dn = unit(edge)
    turn = np.linalg.norm(db - u * (db @ u)) / dn           # radians per unit of b
    u, _ = unit(edge + inward * 0.3 * margin / (2 * R * T * turn))
    nrm = db - u * (db @ u)
    nrm = inward * nrm / np.linalg.norm(nrm)
    sph[6], (sph[8 + 6], sph[16 + 6], sph[24 + 6]) = np.float32(R * R), (pos + T * u + R * nrm).astype(np.float32)
    return sph, eps, (w, h), cam, (side, n)


def family_case(seed, index, shape=None, reference_camera=False):
    """Member `index` of the family of `seed` -> (table, eps, (w, h), camera); each member has a generator of its own, so a test may
    take any subset."""
    rng = np.random.default_rng([int(seed), int(index)])
    sph = family_table(rng)
    eps = float(FAMILY_EPS[rng.integers(len(FAMILY_EPS))])
    w, h = FAMILY_SHAPES[index % len(FAMILY_SHAPES)] if shape is None else shape
    cam = family_camera(rng, w, h)
    if reference_camera:
        cam = camera(twin(), w, h)
    return sph, eps, (w, h), cam
