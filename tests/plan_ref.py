"""NumPy's float32 pairwise sum as a PLAN of leaves, written from numpy's own rule (not from pt_leaf.h), for the deep-plan tests.

np.mean of a contiguous float32 run of n samples sums it pairwise: a run of at most 128 samples is one block (summed with eight
interleaved accumulators); a longer run is split at n // 2 rounded down to a multiple of 8, the left part first, the right part taking
the remainder.  Flattened left to right that is a list of leaves [(len, ncomb)]: sum the leaf, push it, then `ncomb` times add the two
topmost partial sums.

frames() builds, from per-path colours, the frame of that tree (np.add.reduce on each contiguous leaf, the tree's additions in float32)
and of two WRONG summation orders over the same samples.  A test input is sensitive to the summation order when the wrong orders give
other frames: only then does a bitwise comparison of a kernel's frame see the order in which the kernel summed.

CASES below are the scenes and parameters the deep-plan tests run; tests/test_deep_plans_cpu.py holds each to the sensitivity
conditions, tests/test_gpu_deep_plans.py runs them on the device."""
import numpy as np

F = np.float32
BLOCK = 128                                  # numpy's PW_BLOCKSIZE
DEEP = (257, 521, 1025, 4096, 4199, 7688)    # see stats(): stack depths 3 .. 7, 64 leaves, the camera's 44-leaf limit


def plan(s):
    """-> [(len, ncomb)] for a run of s samples."""
    out = []

    def rec(n):
        if n <= BLOCK:
            out.append([n, 0])
            return
        n2 = n // 2
        n2 -= n2 % 8
        rec(n2)
        rec(n - n2)
        out[-1][1] += 1

    rec(int(s))
    return [tuple(x) for x in out]


def stats(s):
    """-> dict(leaves, maxleaf, ncomb (the largest), depth (of the stack of partial sums), tails (the leaves with a len % 8 tail))."""
    pl = plan(s)
    depth = top = 0
    for _, ncomb in pl:
        top += 1
        depth = max(depth, top)
        assert top > ncomb
        top -= ncomb
    assert top == 1 and sum(n for n, _ in pl) == s
    return dict(leaves=len(pl), maxleaf=max(n for n, _ in pl), ncomb=max(c for _, c in pl), depth=depth,
                tails=[n for n, _ in pl if n % 8])


def _runs(colors, npix, s):
    """colours [3][npix * 4 * s] -> float32 [3 * npix * 4][s]: one row per (channel, pixel, sub-pixel), its s samples contiguous."""
    c = np.ascontiguousarray(colors, dtype=F).reshape(3 * npix * 4, s)
    return c


def _block_sums(rows, bounds):
    """np.add.reduce over each contiguous [a, b) of every row (b - a <= 128: one pairwise block) -> list of float32 [rows]."""
    out = []
    for a, b in bounds:
        assert 0 < b - a <= BLOCK
        out.append(np.add.reduce(np.ascontiguousarray(rows[:, a:b]), axis=1, dtype=F))
    return out


def _fold_left(parts):
    acc = parts[0]
    for x in parts[1:]:
        acc = acc + x
        assert acc.dtype == F
    return acc


def sums(colors, npix, s):
    """-> dict(tree, left, blocks): float32 [3 * npix * 4] sums of every sub-pixel's run in the three orders."""
    rows = _runs(colors, npix, s)
    pl = plan(s)
    ends = np.cumsum([n for n, _ in pl])
    leaves = _block_sums(rows, [(e - n, e) for e, (n, _) in zip(ends, pl)])
    stack = []
    for x, (_, ncomb) in zip(leaves, pl):
        stack.append(x)
        for _ in range(ncomb):
            b = stack.pop()
            a = stack.pop()
            stack.append(a + b)
            assert stack[-1].dtype == F
    assert len(stack) == 1
    blocks = _block_sums(rows, [(a, min(a + BLOCK, s)) for a in range(0, s, BLOCK)])
    return dict(tree=stack[0], left=_fold_left(leaves), blocks=_fold_left(blocks))


def decode(total, npix, s):
    """The decode's last steps on float32 sums [3 * npix * 4]: sum / count in float32 (np.mean), the float64 mean of the four sub-pixels,
    clip, float32 framebuffer, truncation to 8 bits -> (pre float64 [npix][3], fb float32 [3][npix], u8 [npix][3])."""
    m = (total / F(s)).astype(F).reshape(3, npix, 4).astype(np.float64)
    acc = np.zeros((3, npix))
    for sub in range(4):
        acc = acc + m[:, :, sub]
    pre = acc / 4
    cl = np.clip(pre, 0, 1)
    return np.ascontiguousarray(pre.T), cl.astype(F), np.ascontiguousarray((cl * 255).astype(np.uint8).T)


def frames(colors, npix, s):
    """-> dict(tree, left, blocks) of (pre, fb, u8): numpy's pairwise tree; mutant 1, the leaf sums folded left to right; mutant 2,
    consecutive 128-sample blocks folded left to right."""
    return {k: decode(v, npix, s) for k, v in sums(colors, npix, s).items()}


def differing(fb_a, fb_b):
    """Number of float32 framebuffer values whose bits differ."""
    return int((np.ascontiguousarray(fb_a, dtype=F).view(np.uint32) != np.ascontiguousarray(fb_b, dtype=F).view(np.uint32)).sum())


def saturated(fb):
    """Number of framebuffer values that are exactly 0 or 1 (clipped, or black: such a value hides its sum)."""
    fb = np.asarray(fb)
    return int(((fb == 0) | (fb == 1)).sum())


def check_sensitive(colors, npix, s):
    """The sensitivity conditions on per-path colours: each mutant frame differs from the tree frame in at least 4 float32 framebuffer
    values, and at most a third of the framebuffer values are exactly 0 or 1.  -> (frames, (differing left, differing blocks, saturated))."""
    fr = frames(colors, npix, s)
    fb = fr["tree"][1]
    d1, d2, sat = differing(fr["left"][1], fb), differing(fr["blocks"][1], fb), saturated(fb)
    assert d1 >= 4 and d2 >= 4, ("a wrong summation order gives nearly the same frame", s, d1, d2)
    assert 3 * sat <= fb.size, ("too many framebuffer values at 0 or 1", s, sat, fb.size)
    return fr, (d1, d2, sat)


def mixed_colors(npix, s, seed):
    """Random colours [3][npix * 4 * s] of mixed magnitude: every sample is a uniform [0, 1) value times one of 0, 0.01, 1 and 30 (so
    the rounding of a partial sum depends on what was added before it), times its pixel's brightness, one of 0.02 .. 1 in turn: the
    means run from 0.08 to 3.9, so that every fifth pixel is clipped and the others show their sums."""
    rng = np.random.default_rng(seed)
    scale = np.array([0.0, 0.01, 1.0, 30.0], dtype=F)[rng.integers(0, 4, (3, npix, 4 * s))]
    bright = np.array([0.02, 0.05, 0.1, 0.25, 1.0], dtype=F)[np.arange(npix) % 5]
    return (rng.random((3, npix, 4 * s), dtype=F) * scale * bright[None, :, None]).astype(F).ravel()


def decode_colors(s):
    """The colours of the device decode tests: 12 pixels of mixed_colors()."""
    return mixed_colors(12, s, seed=2000 + s)


# ---- the cases of the deep-plan tests ------------------------------------------------------------------------------------------------
W, H = 4, 3                                  # 12 pixels: in the one-lane-group kernels one whole 8-pixel workgroup and a partial one
SUB = (3, 7)                                 # the second range: pixels [3, 10)
K, O = 0, 1
RETIRE, RR = 1, 2
TILE_NS, GRID_NS = 40, 300                   # tests/test_gpu_launch_matrix.py's generated scenes (oracle.gen_scene(ns, seed=7))

# Mirror renderer, per scene.  Gain 1 (the default gain of 12 clips 24 of the 36 values of such a frame to 1, and a clipped value hides
# its sum); depth and seed chosen by measurement on the CPU oracle so that check_sensitive() holds at every count, in both modes, with
# and without roulette (seed 11 of the reference scene misses it with roulette at 257 samples: 1 value differs for mutant 2).
# The brute-force oracle pays depth x spheres per path, hence the smaller depths of the larger scenes (7688 samples are 369 024 paths).
MIRROR = {
    "ref": dict(ns=8, depth=5, gain=1.0, seed=12, rr_start=2),
    "tiles": dict(ns=TILE_NS, depth=3, gain=1.0, seed=12, rr_start=2),
    "grid": dict(ns=GRID_NS, depth=2, gain=1.0, seed=12, rr_start=1),
}
TILE_SAMPLES = (256,) + DEEP                 # 256 = 2 x 128: the first count whose leaves are 128 long (no order to tell apart: one addition)
GRID_SAMPLES = (257, 1025, 7688)


def mode_of(scene, s):
    """The arithmetic modes a scene's rows run at `s` samples: the 8-sphere scene both at every count; the larger scenes both up to 1025
    samples and one above (alternating), to bound the brute-force oracle's time."""
    if scene == "ref" or s <= 1025:
        return (K, O)
    return (O,) if s == 4199 else (K,)


def mirror_cases():
    """Every (scene, mode, flags, samples) the mirror-renderer GPU rows render, each once."""
    out = []
    for s in DEEP:
        for m in mode_of("ref", s):
            out += [("ref", m, f, s) for f in (0, RR, RETIRE, RETIRE | RR)]
    for s in TILE_SAMPLES:
        for m in mode_of("tiles", s):
            out += [("tiles", m, f, s) for f in (0, RETIRE)]
    for s in GRID_SAMPLES:
        for m in mode_of("grid", s):
            out += [("grid", m, f, s) for f in (0, RETIRE | RR)]
    return out


_SCENES = {}


def mirror_scene(oracle, name):
    """-> (the padded [10][Ns] table, Ns): the reference's 8 spheres, or the launch matrix's generated scenes."""
    if name not in _SCENES:
        ns = MIRROR[name]["ns"]
        _SCENES[name] = (oracle.gen_spheres() if name == "ref" else oracle.gen_scene(ns, seed=7), ns)
    return _SCENES[name]


def mirror_params(oracle, scene, mode, flags, s, **kw):
    c = MIRROR[scene]
    return oracle.make_params(W, H, s, depth=c["depth"], num_spheres=c["ns"], gain=c["gain"], mode=mode, flags=flags, seed=c["seed"],
                              rr_start=c["rr_start"], **kw)


# The fused MT19937 frame (np.random.seed(0) rays, O-mode): two 78-pixel groups, the second partial; depth 2.  Gain 1: with 12, 211 of
# the 270 values are clipped.
MT_W, MT_H, MT_DEPTH, MT_GAIN = 10, 9, 2, 1.0
MT_SAMPLES = (257, 1025, 4199, 7688)
MT_SUB = (41, 40)                            # an odd start inside the first group, the end inside the second


def mt_colours(oracle, s):
    rays = oracle.gen_rays(MT_W, MT_H, s, seed=0)
    col, _ = oracle.render_paths(oracle.make_params(MT_W, MT_H, s, depth=MT_DEPTH, mode=O, gain=MT_GAIN), rays, mirror_scene(oracle, "ref")[0],
                                 threads=oracle.max_threads())
    return col


# Material renderer: depth 5, seed 20 (measured: seeds 11 and 12 miss the conditions at 257 samples with direct light sampling).
MAT_SAMPLES = (257, 4199, 7688)
MAT_DEPTH, MAT_SEED = 5, 20
CAMERA_SAMPLES = 4199                        # 44 leaves: the contract's 44-leaf limit with a camera
# (scene, light mode): diff8 plain and with APT_FLAG_NEE, demo9 with the lamp and a light table (by tiles and through its grid: one restatement)
MAT_CASES = (("diff8", "plain"), ("diff8", "nee"), ("demo9lamp", "table"))


def mat_scene(gen_data, name):
    """-> (spheres, materials int32, ns, light index, light table or None)."""
    if name == "diff8":                      # 8-sphere form: gen_spheres with DIFF walls and light, the mirror SPEC
        return gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 8, 7, None
    sph, mat = gen_data.gen_spheres_materials()   # tile form: gen_spheres + the glass ball, the light smallpt's small lamp
    sph = gen_data.with_lamp(sph, 9, 7)
    return sph, np.asarray(mat, dtype=np.int32), 9, 7, gen_data.build_lights(sph, 9, [7])


def lens_camera(gen_data):
    """A thin-lens camera inside the room, oblique (tests/test_gpu_camera.py's first look-at camera with its lens)."""
    return gen_data.camera(width=W, height=H, eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05), vfov_deg=55.0,
                           offset=0.0, aperture=2.5)


def mat_colours(oracle, gen_data, name, mode, s, cam=None):
    """The restatement's per-path colours [3][W * H * 4 * s] of a material case (materials_ref), from the
    counter generator's rays or, with `cam` (an ApCamera), from camera_ref's."""
    import camera_ref as cr
    import materials_ref as mr
    sph, mat, ns, light, table = mat_scene(gen_data, name)
    p = oracle.make_params(W, H, s, depth=MAT_DEPTH, num_spheres=ns, light_index=light, seed=MAT_SEED)
    rays = oracle.gen_rays_counter(p) if cam is None else cr.rays(cr.from_ctypes(cam), W, H, s, seed=MAT_SEED)
    args = (rays, sph, mat, ns, MAT_DEPTH, p.eps, MAT_SEED, np.arange(rays.shape[1], dtype=np.uint64))
    L, bad, _ = mr.trace(*args, light=light, nee=mode == "nee", table=table if mode == "table" else None, gloss=False)
    assert not bad.any()
    return L
