"""GPU: a light table in the material renderer (the *_lights entries, include/render_mi355x.h "several lights").
Pinned to the code that exists -- a one-light table against the same launch with APT_FLAG_NEE, bit for bit --, then bit for bit against
the NumPy restatement tests/materials_ref.py with several lights on all three scene forms (8 spheres in SGPRs, LDS tiles, the uniform
grid), against a closed form that depends on neither, and statistically against the renderer without sampling: same expectation, less
variance than sampling no lamp or one lamp of two."""
import numpy as np
import pytest

import lights_ref as lr
import materials_ref as mr
from gpu_harness import Scene, apt, bits_equal, dev, oracle_params, same, scene  # noqa: F401

pytestmark = pytest.mark.gpu


def _checked(sc):
    """Every light table of this file is also lights_ref's."""
    assert np.array_equal(sc.table, lr.build_table(sc.sph, sc.ns, sc.lights))
    return sc


_big16 = []


def _scene(apt, name):
    """The catalogue's pin scenes "<diff8|demo9|big1030>-<stock|lamp>" (one light, listed alone), two8 and demo9x2; big16: sixteen lamps
    among 1030 spheres, by tiles and through a grid."""
    if name != "big16":
        return _checked(scene(apt, name))
    if not _big16:
        sph, mat, ns, idx = lr.sixteen_lamps(apt.gen_data)
        _big16.append(_checked(Scene(apt, sph, mat, ns, lights=idx, grid=True)))
    return _big16[0]


# ---- the pin: a one-light table IS APT_FLAG_NEE with that light ----------------------------------------------------------------------------
PIN_SCENES = ["diff8-stock", "diff8-lamp", "demo9-stock", "demo9-lamp", "big1030-stock", "big1030-lamp"]


@pytest.mark.parametrize("name", PIN_SCENES)
def test_pin_one_light_table_is_the_flag_bit_for_bit(apt, name):
    from oracle import oracle
    sc = _scene(apt, name)
    big = name.startswith("big")
    w, h = (24, 16) if big else (48, 32)
    for grid in ((True, False) if big else (False,)):
        for s_, depth, rr in ((3, 5, True), (8, 5, False), (13, 8, True)):           # both GROUP arms, a tail, roulette
            on = sc.params(w, h, s_, depth, mode="nee", rr=rr, seed=11 + s_, grid=grid)
            off = sc.params(w, h, s_, depth, rr=rr, seed=11 + s_, grid=grid)
            with apt.render.TraceCounter() as tc_f:
                want = sc.frame(on)
            with apt.render.TraceCounter() as tc_t:
                got = sc.frame(off, "table")
            same(got, want)
            assert tc_f.value == tc_t.value > 0
            assert not np.array_equal(got[0], sc.frame(off)[0])   # and it is not the plain frame
        b, c = (117, 203) if big else (517, 700)                                     # a pixel range
        on = sc.params(w, h, 16, 5, mode="nee", seed=2, grid=grid)
        same(sc.frame(on.copy(flags=on.flags & ~apt.APT_FLAG_NEE, light_index=-1), "table", pixel_begin=b, pixel_count=c),
             sc.frame(on, pixel_begin=b, pixel_count=c))            # light_index is not read
        on = sc.params(16, 16, 4, 8, mode="nee", rr=True, seed=9, grid=grid)        # paths, and a path range
        rays = oracle.gen_rays_counter(oracle_params(on))
        with apt.render.TraceCounter() as tc_f:
            want = sc.paths(on, rays)
        with apt.render.TraceCounter() as tc_t:
            got = sc.paths(on, rays, "table")                                            # the flag bit itself is not read either
        assert bits_equal(got, want) and tc_f.value == tc_t.value > rays.shape[1]
        b, c = 1001, 1537
        got = sc.paths(on.copy(path_begin=b, path_count=c), rays, "table")
        assert bits_equal(got[:, b:b + c], want[:, b:b + c]) and np.isnan(got[:, :b]).all() and np.isnan(got[:, b + c:]).all()


# ---- bit for bit against the restatement, several lights -----------------------------------------------------------------------------
# tests/test_gpu_nee.py's FRAME_CASES: (samples, depth, roulette, width, height): both GROUP arms (samples < 8, >= 8), a tail
# (13 = 8 + 5), depths 1, 2, 5, 8, and 136 = two pairwise leaves (64 + 72) combined through the LDS stack
FRAME_CASES = [(1, 1, False, 48, 32), (8, 1, True, 48, 32), (3, 2, False, 48, 32), (8, 2, True, 48, 32), (8, 5, False, 48, 32),
               (3, 5, True, 48, 32), (13, 8, False, 48, 32), (3, 8, True, 48, 32), (136, 3, True, 24, 16)]


@pytest.mark.parametrize("name", ["two8", "demo9x2"])
@pytest.mark.parametrize("s_,depth,rr,w,h", FRAME_CASES)
def test_frame_bitwise(apt, name, s_, depth, rr, w, h):
    sc = _scene(apt, name)
    p = sc.params(w, h, s_, depth, rr=rr, seed=11 + s_)
    fb, u8 = sc.frame(p, "table")
    fb_w, u8_w, bad, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat, table=sc.table)
    assert not bad.any()
    same((fb, u8), (fb_w, u8_w))
    off = sc.frame(p)
    if depth == 1:                                        # no sample at the last bounce: the table changes nothing
        same((fb, u8), off)
    else:
        assert not np.array_equal(fb, off[0])


BIG_CASES = [(2, 1, False), (2, 2, False), (8, 5, True), (13, 8, False)]


@pytest.mark.parametrize("s_,depth,rr", BIG_CASES)
def test_frame_bitwise_16_lamps_by_tiles_and_through_the_grid(apt, s_, depth, rr):
    sc = _scene(apt, "big16")
    p = sc.params(24, 16, s_, depth, rr=rr, grid=True)
    fb_g, u8_g = sc.frame(p, "table")
    fb_t, u8_t = sc.frame(sc.params(24, 16, s_, depth, rr=rr, grid=False), "table")
    same((fb_g, u8_g), (fb_t, u8_t))                         # grid form == tile form
    fb_w, u8_w, bad, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat, table=sc.table)
    assert not bad.any()
    same((fb_t, u8_t), (fb_w, u8_w))
    if depth > 1:
        assert not np.array_equal(fb_g, sc.frame(p)[0])


@pytest.mark.parametrize("name,grid,b,c", [("two8", False, 517, 700), ("demo9x2", False, 517, 700), ("big16", True, 117, 203),
                                           ("big16", False, 117, 203)])
def test_frame_mid_image_pixel_range(apt, name, grid, b, c):
    sc = _scene(apt, name)
    w, h = (48, 32) if name != "big16" else (24, 16)
    p = sc.params(w, h, 16, 5, seed=2, grid=grid, flags=apt.APT_FLAG_RETIRE)      # RETIRE: accepted, changes nothing
    fb, u8 = sc.frame(p, "table", pixel_begin=b, pixel_count=c)
    fb_w, u8_w, _, _ = mr.render_frame(oracle_params(p.copy(flags=p.flags & ~apt.APT_FLAG_RETIRE)), sc.sph, sc.mat, table=sc.table, pixel_begin=b, pixel_count=c)
    same((fb, u8), (fb_w, u8_w))


@pytest.mark.parametrize("name,grid", [("two8", False), ("demo9x2", False), ("big16", False), ("big16", True)])
def test_paths_bitwise_with_ranges(apt, name, grid):
    from oracle import oracle
    sc = _scene(apt, name)
    p = sc.params(16, 16, 4, 8, rr=True, seed=9, grid=grid)
    rays = oracle.gen_rays_counter(oracle_params(p))
    n = rays.shape[1]
    want, bad, segments = mr.trace(rays, sc.sph, sc.mat, sc.ns, 8, p.eps, p.seed, np.arange(n, dtype=np.uint64), rr_start=2, table=sc.table, gloss=False)
    assert not bad.any()
    with apt.render.TraceCounter() as tc:
        got = sc.paths(p, rays, "table")
    assert bits_equal(got, want), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    assert tc.value == segments > n                       # shadow segments count as traced segments
    b, c = 1001, 1537                                     # a path range of the whole-image buffers, then the same range in band buffers
    got = sc.paths(p.copy(path_begin=b, path_count=c), rays, "table")
    assert bits_equal(got[:, b:b + c], want[:, b:b + c])
    assert np.isnan(got[:, :b]).all() and np.isnan(got[:, b + c:]).all()
    pb = p.copy(path_begin=b, path_count=c, flags=p.flags | apt.APT_FLAG_BAND_BUFFERS)
    got = sc.paths(pb, np.ascontiguousarray(rays[:, b:b + c]), "table")
    assert bits_equal(got, want[:, b:b + c])
    for depth in (1, 2, 5):                               # no roulette, the other depths
        q = sc.params(16, 16, 4, depth, seed=9, grid=grid)
        want, _, _ = mr.trace(rays, sc.sph, sc.mat, sc.ns, depth, q.eps, q.seed, np.arange(n, dtype=np.uint64), table=sc.table, gloss=False)
        got = sc.paths(q, rays, "table")
        assert bits_equal(got, want), depth
        if depth == 1:
            assert bits_equal(got, sc.paths(q, rays))


def test_context_methods_take_the_table(apt):
    import torch
    sc = _scene(apt, "two8")
    p = sc.params(48, 32, 8, 5, seed=4)
    want = sc.frame(p, "table")
    ctx = apt.render.Context()
    try:
        fb, u8 = ctx.render_frame(p, sc.d_sph, materials=sc.d_mat, lights=sc.d_table)
        ctx.check()
        same((fb.cpu().numpy(), u8.cpu().numpy()), want)
    finally:
        ctx.close()
    with pytest.raises(apt.AptError, match="lights needs materials"):
        apt.render.render_frame(p, sc.d_sph, lights=sc.d_table)
    torch.cuda.synchronize()


# ---- the S = false group --------------------------------------------------------------------------------------------------------------
def test_a_light_we_stand_on_is_never_sampled(apt):
    """The white furnace listed as the only light: S is false at every bounce, so the frame is the plain frame bit for bit and every
    pixel is exactly 0.5 (1 - 2^-D)."""
    sph, mat, ns = lr.furnace(False)
    sc = _checked(Scene(apt, sph, mat, ns, lights=[0]))
    for depth, s_ in ((1, 1), (2, 3), (5, 8), (8, 16)):
        p = apt.make_params(32, 16, s_, depth=depth, num_spheres=ns, eps=0.5, seed=depth, light_index=-1)
        with apt.render.TraceCounter() as tc:
            fb, u8 = sc.frame(p, "table")
        assert tc.value == depth * p.num_paths            # no shadow segment either
        same((fb, u8), sc.frame(p))
        assert (fb == np.float32(0.5 * (1 - 2.0 ** -depth))).all(), (depth, np.unique(fb))


# z-scores on the CPU restatement (the GPU equals it bit for bit): -0.48 -0.48 -0.50 per channel with seed 21
def test_a_light_we_are_inside_of_is_gathered_by_the_next_hit(apt):
    """The furnace with a small lamp inside, both listed: the enclosing sphere is never sampled (we stand on it) and the lamp is; the
    mean is the plain renderer's."""
    from oracle import oracle
    sph, mat, ns = lr.furnace(True)
    sc = _checked(Scene(apt, sph, mat, ns))
    assert mr.Table(sc.table).idx.tolist() == [0, 1]
    p = apt.make_params(128, 64, 4, depth=4, num_spheres=ns, eps=0.5, seed=21, light_index=-1)
    rays = oracle.gen_rays_counter(oracle_params(p))
    on, off = sc.paths(p, rays, "table").astype(np.float64), sc.paths(p, rays).astype(np.float64)
    _expect_equal_means("furnace + lamp", on, off)


def _expect_equal_means(what, on, off):
    n = on.shape[1]
    for ch in range(3):
        s_on, s_off = on[ch].std(ddof=1) / np.sqrt(n), off[ch].std(ddof=1) / np.sqrt(n)
        z = (on[ch].mean() - off[ch].mean()) / np.hypot(s_on, s_off)
        print("%s channel %d: table %.5f +- %.5f  plain %.5f +- %.5f  z %+.2f" % (what, ch, on[ch].mean(), s_on, off[ch].mean(), s_off, z))
        assert s_on > 0 and s_off > 0
        assert abs(on[ch].mean() - off[ch].mean()) < 4 * np.hypot(s_on, s_off)


# ---- analytic, independent of the library and of the restatement -----------------------------------------------------------------------
@pytest.mark.parametrize("j", range(8))
def test_closed_form_lambertian_point_under_three_lights(apt, j):
    """A Lambertian point under three listed sphere lights, two unoccluded with different radius, distance and emission and one below
    the horizon, reflects sum_j albedo * Le_j * (r_j / dist_j)^2 * cos(theta_j) over the two.  8 points, 4096 paths each, depth 2,
    every point within 4 sigma (tests/test_nee_cpu.py's protocol for one light)."""
    per = 4096
    rays, sph, mat, ns, paths, want = lr.three_lights_point(j, per)
    sc = _checked(Scene(apt, sph, mat, ns, lights=[1, 2, 3]))
    # path ids j * per ..: the launch's own numbering is 0 .. per - 1, so render the point as the j-th band of an 8-band buffer
    n = 8 * per
    p = apt.make_params(64, 32, 4, depth=2, num_spheres=ns, eps=1e-4, seed=7, light_index=-1, path_begin=j * per, path_count=per,
                        flags=apt.APT_FLAG_BAND_BUFFERS)
    assert p.num_paths == n
    L = sc.paths(p, rays, "table").astype(np.float64)
    for ch in range(3):
        sigma = L[ch].std(ddof=1) / np.sqrt(per)
        print("x = %4.1f ch %d  closed form %.6f  mean %.6f  sigma %.3e  z %+.2f" % (2.0 * j - 6.0, ch, want[ch], L[ch].mean(), sigma,
                                                                                    (L[ch].mean() - want[ch]) / sigma))
        assert sigma > 0 and abs(L[ch].mean() - want[ch]) < 4 * sigma


# ---- against the renderer without sampling (the plain *_materials launch on the same rays is the yardstick, never the new code) ----------
def _on_off(apt, name, depth, seed, grid=False):
    """-> (radiance with the table, plain, the camera ray hits an emitter) for 2^17 camera rays; float64 [3][n], bool [n]."""
    from oracle import oracle
    sc = _scene(apt, name)
    p = sc.params(128, 64, 4, depth, seed=seed, grid=grid)
    assert p.num_paths == 1 << 17
    rays = oracle.gen_rays_counter(oracle_params(p))
    on = sc.paths(p, rays, "table").astype(np.float64)
    off = sc.paths(p, rays).astype(np.float64)
    first = sc.paths(sc.params(128, 64, 4, 1, seed=seed, grid=grid), rays)
    return on, off, first.any(axis=0), rays


# z-scores of these inputs on the CPU restatement (which the GPU equals bit for bit, so the test is deterministic), per channel, seed 21:
#   two8 depth 2: -0.02 +0.11 +0.17      two8 depth 5: -0.07 -0.01 +0.20
#   demo9x2 depth 8: -0.02 +0.08 +0.30   big16 through the grid, depth 5: +0.36 +0.27 +0.19
# The plain renderer finds a lamp of these scenes by chance, so its sigma is spiky (a few paths carry most of the variance) and the
# check is blunt; the closed-form test above is the sharp one.
@pytest.mark.parametrize("name,depth,seed,grid", [("two8", 2, 21, False), ("two8", 5, 21, False), ("demo9x2", 8, 21, False),
                                                  ("big16", 5, 21, True)])
def test_same_expectation_as_the_plain_renderer(apt, name, depth, seed, grid):
    on, off, _, _ = _on_off(apt, name, depth, seed, grid)
    _expect_equal_means("%s depth %d" % (name, depth), on, off)


def test_it_pays_less_variance_than_no_sampling_and_than_one_lamp_of_two(apt):
    """Two lamps, depth 5, over the paths whose camera ray hits no lamp: the per-channel sample variance of the table launch is below
    the plain renderer's AND below APT_FLAG_NEE's sampling either one of the two lamps.  Only the ordering is asserted; the restatement
    gives plain / table = 239 / 342 / 276, NEE(6) / table = 211 / 327 / 273, NEE(7) / table = 29.6 / 16.0 / 3.7 per channel on these inputs."""
    on, off, direct, rays = _on_off(apt, "two8", 5, 21)
    sc = _scene(apt, "two8")
    assert 0 < direct.sum() < direct.size // 20
    nee = [sc.paths(sc.params(128, 64, 4, 5, mode="nee", seed=21).copy(light_index=l), rays).astype(np.float64)
           for l in (6, 7)]
    for ch in range(3):
        v_on, v_off = on[ch][~direct].var(ddof=1), off[ch][~direct].var(ddof=1)
        v_nee = [a[ch][~direct].var(ddof=1) for a in nee]
        print("channel %d variance: plain / table %.1f   NEE(6) / table %.1f   NEE(7) / table %.1f" % (ch, v_off / v_on, v_nee[0] / v_on,
                                                                                                     v_nee[1] / v_on))
        assert v_on < v_off and v_on < v_nee[0] and v_on < v_nee[1]


# ---- a table that is not this scene's -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two8", "demo9x2", "big16"])
def test_a_table_for_another_scene_renders_nothing_and_is_reported(apt, name):
    """A refusal path, not a fault: the kernel checks the head and returns before it reads anything else of the table."""
    import torch
    sc = _scene(apt, name)
    other = apt.gen_data.build_lights(np.concatenate([sc.sph[:10 * sc.ns].reshape(10, sc.ns), np.ones((10, 1), np.float32)], axis=1).ravel(),
                                      sc.ns + 1, [0])
    assert mr.Table(other).ns == sc.ns + 1
    wrong_magic = sc.table.copy()
    wrong_magic[0] ^= 1
    apt.render.check_device_status()                      # nothing pending
    for bad in (other, wrong_magic):
        d_bad = dev(bad.view(np.int32))
        for grid in ((True, False) if sc.grid is not None else (False,)):
            p = sc.params(24, 16, 8, 3, grid=grid)
            fb = torch.full((3, 24 * 16), float("nan"), dtype=torch.float32, device="cuda")
            u8 = torch.full((24 * 16, 3), 7, dtype=torch.uint8, device="cuda")
            apt.render.render_frame(p, sc.d_sph, materials=sc.d_mat, lights=d_bad, fb=fb, fb_u8=u8)
            torch.cuda.synchronize()
            assert torch.isnan(fb).all() and (u8 == 7).all()
            with pytest.raises(apt.AptError, match="lights-mismatch") as e:
                apt.render.check_device_status()
            assert "unknown-bits" not in str(e.value) and "grid" not in str(e.value) and "bad-material" not in str(e.value)
            colors = torch.full((3 * p.num_paths,), float("nan"), dtype=torch.float32, device="cuda")
            rays = torch.zeros(6 * p.num_paths, dtype=torch.float32, device="cuda")
            apt.render.render_do_ex(p, None, rays, sc.d_sph, colors, materials=sc.d_mat, lights=d_bad)
            torch.cuda.synchronize()
            assert torch.isnan(colors).all()
            with pytest.raises(apt.AptError, match="lights-mismatch"):
                apt.render.check_device_status()
    apt.render.check_device_status()                      # read and cleared
