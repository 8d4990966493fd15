"""What the tests of the per-sphere form of pair (6,7)'s skip share (pt_trace.h sphere_reachable_mask, intersect_ns8_v2<.., SKIP>):
the device predicate and the oracle's root selection restated in float32, the scene tables, the bounce restated with the oracle's
operation order (b, c and the discriminant of every sphere at every bounce), and the kernel's grouping of paths into waves."""
import numpy as np

f = np.float32
GUARD = f(2.0 ** -60)            # pt_trace.h kBehindGuard
MISS_T = f(1e20)
SCENES = ("ref", "ball_front", "light_r1", "both_away", "ball_big")
W, H, S, SEED = 48, 32, 16, 5


def cannot_hit(b, c, disc):
    """not sphere_reachable_mask's bit: med3(disc, b, -c) >= -2^-60 fails.  v_med3_f32 returns the minimum of the operands that are
    not NaN when one is NaN (NaN when all are)."""
    b, c, disc = (np.asarray(x, f) for x in (b, c, disc))
    v = np.stack([disc, b, -c])
    with np.errstate(all="ignore"):
        med = np.where(np.isnan(v).any(axis=0), np.fmin(np.fmin(v[0], v[1]), v[2]), np.sort(v, axis=0)[1])
        return ~(med >= -GUARD)


def intersect_post(b, disc, eps):
    """pt_oracle.c trace_path's root selection (pt_core.h intersect_post): float32 operation for operation; np.sqrt rounds correctly."""
    b, disc, eps = (np.asarray(x, f) for x in (b, disc, eps))
    with np.errstate(all="ignore"):
        q = np.sqrt(disc)
        t0, t1 = b - q, b + q
        t = np.where(t0 > eps, t0, t1)
        return np.where(t > eps, t, MISS_T)


def scene(oracle, name):
    """The table [10][8] (r^2, cx, cy, cz, emission x 3, albedo x 3) inside the padded 128 floats.  Every table keeps the equality pattern
    of centre coordinates (pt_trace.h scene8_shares_planes: all of sphere 6's are free, of sphere 7's only cy), so all of them run the
    shared-planes form."""
    t = oracle.gen_spheres().copy()
    tab = t[:80].reshape(10, 8)

    def put(k, r, cx, cy, cz):
        tab[0, k] = f(np.float64(r) * np.float64(r))      # squared in float64 before the cast, as gen_spheres does
        tab[1, k], tab[2, k], tab[3, k] = cx, cy, cz

    if name == "ball_front":      # the mirror ball (r = 16.5 as it is) 35 in front of the camera rays' origins, in the middle of the view
        put(6, 16.5, 50.0, 44.0, 120.0)
    elif name == "ball_big":      # and grown to r = 150 round the back wall's middle: every camera ray reaches it (no r = 16.5 ball can
        put(6, 150.0, 50.0, 40.8, 0.0)   # cover the rays' origins, 108 x 73 wide); the origins stay outside it (z >= 154)
    elif name == "light_r1":      # the light's radius 1, its centre where it was (600 above the ceiling's plane)
        put(7, 1.0, tab[1, 7], tab[2, 7], tab[3, 7])
    elif name == "both_away":     # the ball far outside the room behind the left wall, the light far above it
        put(6, 16.5, -3.0e4, 16.5, 47.0)
        put(7, 600.0, tab[1, 7], 3.0e5, tab[3, 7])
    else:
        assert name == "ref"
    return t


def same(got, want):
    got, want = np.asarray(got, dtype=f), np.asarray(want, dtype=f)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return bool(ok.all()), np.argwhere(~ok)[:5]


_TRACES = {}


def trace(oracle, name, depth=8):
    """K-mode paths of the W x H frame at S samples -> b, c, disc float32 [depth][8][N] (pt_oracle.c trace_path, operation for operation,
    on float32 arrays: numpy rounds every operation).  The colours of the restatement are checked against the oracle's, bit for bit."""
    key = (name, depth)
    if key in _TRACES:
        return _TRACES[key]
    p = oracle.make_params(W, H, S, depth=depth, mode=oracle.MODE_K, seed=SEED)
    rays = oracle.gen_rays_counter(p)
    table = scene(oracle, name)
    tab = table[:80].reshape(10, 8)
    r2, cx, cy, cz = (tab[m][:, None] for m in range(4))
    ox, oy, oz, dx, dy, dz = (rays[m].copy() for m in range(6))
    n = ox.size
    ret = [np.ones(n, f), np.ones(n, f), np.ones(n, f)]
    alive = np.ones(n, bool)
    eps, light, lanes = f(p.eps), int(p.light_index), np.arange(n)
    bs, cs, discs = [], [], []
    with np.errstate(all="ignore"):
        for _ in range(depth):
            ocx, ocy, ocz = cx - ox, cy - oy, cz - oz
            b = ocx * dx
            b = b + ocy * dy
            b = b + ocz * dz
            c = ocx * ocx
            c = c + ocy * ocy
            c = c + ocz * ocz
            c = c - r2
            disc = b * b
            disc = disc - c
            bs.append(b), cs.append(c), discs.append(disc)
            t = intersect_post(b, disc, eps)
            idx = np.argmin(t, axis=0)                      # the first minimum: strict '<' in ascending order; all-miss -> 0
            tmin = t[idx, lanes]
            hx, hy, hz = ox + dx * tmin, oy + dy * tmin, oz + dz * tmin
            nx, ny, nz = hx - tab[1][idx], hy - tab[2][idx], hz - tab[3][idx]
            s2 = f(0.0) + nx * nx
            s2 = s2 + ny * ny
            s2 = s2 + nz * nz
            L = np.sqrt(s2)
            ux, uy, uz = nx / L, ny / L, nz / L
            dot = f(0.0) + dx * ux
            dot = dot + dy * uy
            dot = dot + dz * uz
            k2 = dot * f(2.0)
            dx, dy, dz = dx - ux * k2, dy - uy * k2, dz - uz * k2
            ox, oy, oz = hx, hy, hz
            alive &= idx != light
            for m in range(3):
                ret[m] = np.where(alive, tab[7 + m][idx] * ret[m], ret[m])
    out = tuple(np.stack(x) for x in (bs, cs, discs))
    assert all(x.dtype == np.float32 for x in out)
    want, _ = oracle.render_paths(p, rays, table, threads=oracle.max_threads())
    ok, where = same(np.stack([r * f(p.gain) for r in ret]), want)
    assert ok, ("the restatement of the bounce differs from the oracle", name, where)
    for x in out:
        x.setflags(write=False)
    _TRACES[key] = out
    return out


def wave_groups(x):
    """[depth][N] per-path values -> [depth][waves * 2 halves][64] as the two-path kernel's waves hold them (pt_frame.h frame_lane: a
    wave is two consecutive pixels x 4 sub-pixels x 8 chain lanes; path half A of the pair is samples 0-7, half B samples 8-15);
    path index = (pixel * 4 + sub) * S + sample."""
    depth = x.shape[0]
    d = x.reshape(depth, W * H // 2, 2, 4, S // 8, 8)       # wave, pixel of the wave, sub-pixel, half, chain lane
    return d.transpose(0, 1, 4, 2, 3, 5).reshape(depth, W * H // 2 * (S // 8), 64)


def arms(oracle, name, depth=8):
    """-> (u6, u7) bool [depth][groups]: no lane of the wave-sized group can hit sphere 6 / sphere 7 at that bounce."""
    b, c, disc = trace(oracle, name, depth)
    u = [wave_groups(cannot_hit(b[:, k], c[:, k], disc[:, k])).all(axis=2) for k in (6, 7)]
    return u[0], u[1]
