"""A wave of the two-path bounce branches round the root stage of sphere pair (6,7) when none of its 64 lanes can hit either sphere
(pt_trace.h intersect_ns8_v2<.., SKIP>, pair_misses_wave(); pt_trace2.h kPairSkip).  The frame must not change: framebuffer and 8-bit image
of the two-path frame kernel against the oracle, bit for bit, in K- and O-mode, on five scene tables:

  ref      the gen_spheres() table: some waves skip pair (6,7), some do not, within one frame
  tiny67   spheres 6 and 7 shrunk to r = 0.01, in a corner of the room and under the ceiling: the pair is skipped almost always
  big6     sphere 6 with r = 40 in front of the camera, 65 away from it: every camera ray's line meets it (it fills the view: 37 degrees
           of half-angle against the frame's 30), so no wave skips the pair at the first bounce
  general  spheres 0 and 6 exchanged (bench.py's general scene): the form without shared planes, pair (6,7) is (left wall, light)
  nowalls  walls 4 and 5 shrunk to r = 1 far outside the room: a wall pair that a whole wave can miss

tiny67, big6 and nowalls keep the table's equality pattern of centre coordinates (pt_trace.h scene8_shares_planes), so they run the
shared-planes form like ref.  Frames: 16x8 whole and a 29-pixel range of 7x5 (an odd count: the last wave's second pixel lies past the
range), samples 16 -- the smallest count the host gives to the two-path kernel (render_kernels.hip: samples >= 16, no retirement, no
roulette) -- and 24 (a pair, then the chain's single member), depth 1, 2, 3 and 8: the bounce that is first and last, first + last,
first + one ping-pong step + last, and the headline's loop.

That the scenes reach the arm they are meant to is checked on the CPU: the bounce is restated here in float32 with the oracle's
operation order (and checked against the oracle's colours, bit for bit), the discriminants of spheres 6 and 7 are taken at every bounce
of every path of the 16x8 frame at 16 samples, and the paths are grouped as the kernel's waves hold them (pt_frame.h frame_lane: a
wave is two consecutive pixels x 4 sub-pixels x 8 chain lanes; path half A of the pair is samples 0-7, half B samples 8-15)."""
import numpy as np
import pytest

K, O = 0, 1
DEPTHS = (1, 2, 3, 8)
SCENES = ("ref", "tiny67", "big6", "general", "nowalls")
FRAMES = ((16, 8, 0, None), (7, 5, 3, 29))      # w, h, pixel_begin, pixel_count
SEED = 5


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()                   # a no-op when the in-tree library is current
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.render, pkg.gen_data = render, gen_data
    return pkg


def _scene(oracle, name):
    """The table [10][8] (r^2, cx, cy, cz, emission x 3, albedo x 3) inside the padded 128 floats."""
    t = oracle.gen_spheres().copy()
    tab = t[:80].reshape(10, 8)

    def put(k, r, cx, cy, cz):
        tab[0, k] = np.float32(np.float64(r) * np.float64(r))    # squared in float64 before the cast, as gen_spheres does
        tab[1, k], tab[2, k], tab[3, k] = cx, cy, cz

    if name == "tiny67":
        put(6, 0.01, 2.0, 1.0, 2.0)
        put(7, 0.01, tab[1, 7], 81.0, tab[3, 7])
    elif name == "big6":
        put(6, 40.0, 50.0, 52.0, 230.0)
    elif name == "general":
        tab[:, [0, 6]] = tab[:, [6, 0]]
    elif name == "nowalls":
        put(4, 1.0, tab[1, 4], 1.0e4, tab[3, 4])
        put(5, 1.0, tab[1, 5], -1.0e4, tab[3, 5])
    else:
        assert name == "ref"
    return t


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return bool(ok.all()), np.argwhere(~ok)[:5]


_WANT = {}


def _oracle_frame(oracle, name, w, h, begin, count, s, depth, mode):
    key = (name, w, h, begin, count, s, depth, mode)
    if key not in _WANT:
        fb, u8, _, _ = oracle.render_frame(oracle.make_params(w, h, s, depth=depth, mode=mode, seed=SEED), _scene(oracle, name),
                                           pixel_begin=begin, pixel_count=count, threads=oracle.max_threads())
        fb.setflags(write=False)
        u8.setflags(write=False)
        _WANT[key] = (fb, u8)
    return _WANT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", SCENES)
def test_two_path_frame_equals_the_oracle(apt, oracle, name, depth, mode):
    import torch
    d_scene = torch.from_numpy(_scene(oracle, name)).cuda()
    for w, h, begin, count in FRAMES:
        for s in (16, 24):
            fb_w, u8_w = _oracle_frame(oracle, name, w, h, begin, count, s, depth, mode)
            fb, u8 = apt.render.render_frame(apt.make_params(w, h, s, depth=depth, mode=mode, seed=SEED), d_scene,
                                             pixel_begin=begin, pixel_count=count)
            torch.cuda.synchronize()
            ok, where = _same(fb.cpu().numpy(), fb_w)
            assert ok, (name, w, h, s, depth, mode, where)
            assert np.array_equal(u8.cpu().numpy(), u8_w), (name, w, h, s, depth, mode)


# ---- which arm the scenes reach: the bounce restated in float32 ------------------------------------------------------------------

W, H, S, DEPTH = 16, 8, 16, 8


def _trace_discriminants(oracle, name):
    """K-mode paths of the 16x8 frame at 16 samples, depth 8 -> (disc float32 [DEPTH][8][N], colours [3][N] as the restatement has them,
    the oracle's colours).  pt_oracle.c trace_path, operation for operation, on float32 arrays (numpy rounds every operation)."""
    f = np.float32
    p = oracle.make_params(W, H, S, depth=DEPTH, mode=oracle.MODE_K, seed=SEED)
    rays = oracle.gen_rays_counter(p)
    table = _scene(oracle, name)
    tab = table[:80].reshape(10, 8)
    r2, cx, cy, cz = (tab[m][:, None] for m in range(4))
    ox, oy, oz, dx, dy, dz = (rays[m].copy() for m in range(6))
    n = ox.size
    ret = [np.ones(n, f), np.ones(n, f), np.ones(n, f)]
    alive = np.ones(n, bool)
    eps, light, lanes = f(p.eps), int(p.light_index), np.arange(n)
    discs = []
    with np.errstate(all="ignore"):
        for _ in range(DEPTH):
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
            discs.append(disc)
            q = np.sqrt(disc)
            t0, t1 = b - q, b + q
            t = np.where(t0 > eps, t0, t1)
            t = np.where(t > eps, t, f(1e20))
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
    assert all(d.dtype == np.float32 for d in discs)
    colours = np.stack([r * f(p.gain) for r in ret])
    want, _ = oracle.render_paths(p, rays, table, threads=oracle.max_threads())
    return np.stack(discs), colours, want


def _wave_groups(x):
    """[DEPTH][N] per-path booleans -> [DEPTH][waves * 2 halves][64]: path index = ((pixel * 4 + sub) * S + sample)."""
    d = x.reshape(DEPTH, W * H // 2, 2, 4, S // 8, 8)       # wave, pixel of the wave, sub-pixel, half, chain lane
    return d.transpose(0, 1, 4, 2, 3, 5).reshape(DEPTH, W * H // 2 * (S // 8), 64)


_ARMS = {}


def _pair67_cannot_hit(oracle, name):
    """-> [DEPTH][groups] : no lane of the wave-sized group can hit sphere 6 or 7 at that bounce (pair_misses_wave)."""
    if name not in _ARMS:
        disc, colours, want = _trace_discriminants(oracle, name)
        ok, where = _same(colours, want)
        assert ok, ("the restatement of the bounce differs from the oracle", name, where)
        miss = ~((disc[:, 6] >= 0) | (disc[:, 7] >= 0))      # per path: negative or NaN in both
        _ARMS[name] = (_wave_groups(miss).all(axis=2), miss)
    return _ARMS[name]


def test_reference_scene_takes_both_arms(oracle):
    skipped, _ = _pair67_cannot_hit(oracle, "ref")
    print("ref: share of (wave, half) groups that skip pair (6,7), per bounce:", skipped.mean(axis=1).round(3).tolist())
    assert skipped.any() and not skipped.all()
    assert skipped[0].any() and not skipped[0].all()          # already at the first bounce, which is a form of its own


def test_tiny_pair_is_skipped(oracle):
    skipped, miss = _pair67_cannot_hit(oracle, "tiny67")
    print("tiny67: share of groups that skip, per bounce:", skipped.mean(axis=1).round(3).tolist())
    assert skipped.any()
    assert skipped.mean() > 0.99                              # "almost always"
    assert miss[0].all()                                      # no camera ray's line comes within 0.01 of either centre


def test_big_sphere_is_never_skipped_at_the_first_bounce(oracle):
    skipped, miss = _pair67_cannot_hit(oracle, "big6")
    print("big6: share of groups that skip, per bounce:", skipped.mean(axis=1).round(3).tolist())
    assert not miss[0].any()                                  # every path's first bounce has a non-negative discriminant on sphere 6
    assert not skipped[0].any()                               # so no group skips there
    # (No placement of an r = 40 sphere keeps every group of every LATER bounce from missing both spheres -- the reflected rays of a
    # wave leave in one direction --, so "never" is claimed for the first bounce, whose form the kernel keeps apart.)
    assert not skipped[2].any() and not skipped[4:].any()     # as it happens, also none at the third and from the fifth bounce on


def test_a_wall_pair_can_be_missed_by_a_whole_wave(oracle):
    """nowalls: the discriminants of spheres 4 and 5 are negative for whole groups (what an enabled wall pair's skip arm would need)."""
    disc, colours, want = _trace_discriminants(oracle, "nowalls")
    ok, where = _same(colours, want)
    assert ok, where
    miss = ~((disc[:, 4] >= 0) | (disc[:, 5] >= 0))
    assert _wave_groups(miss).all(axis=2).any()
