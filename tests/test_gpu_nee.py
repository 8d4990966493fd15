"""GPU: direct light sampling in the material renderer (APT_FLAG_NEE, include/render_mi355x.h "Direct light sampling").
Bit for bit against the NumPy restatement tests/materials_ref.py on all three scene forms (8 spheres in SGPRs, LDS tiles, the uniform grid),
with the stock light and with smallpt's small lamp; and statistically against the renderer that exists -- the same launches without
the flag: same expectation, less variance where a small light makes the plain renderer noisy."""
import numpy as np
import pytest

import materials_ref as mr
from gpu_harness import Scene, apt, oracle_params, same, scene  # noqa: F401

pytestmark = pytest.mark.gpu


def _scene(apt, name, lamp):
    return scene(apt, "%s-%s" % (name, "lamp" if lamp else "stock"))


# (samples, depth, roulette, width, height): both GROUP arms (samples < 8, >= 8), a tail (13 = 8 + 5), depths 1, 2, 5, 8, and
# 136 = two pairwise leaves (64 + 72) combined through the LDS stack
FRAME_CASES = [(1, 1, False, 48, 32), (8, 1, True, 48, 32), (3, 2, False, 48, 32), (8, 2, True, 48, 32), (8, 5, False, 48, 32),
               (3, 5, True, 48, 32), (13, 8, False, 48, 32), (3, 8, True, 48, 32), (136, 3, True, 24, 16)]


@pytest.mark.parametrize("lamp", [False, True], ids=["stock", "lamp"])
@pytest.mark.parametrize("name", ["diff8", "demo9"])
@pytest.mark.parametrize("s_,depth,rr,w,h", FRAME_CASES)
def test_frame_bitwise(apt, name, lamp, s_, depth, rr, w, h):
    sc = _scene(apt, name, lamp)
    p = sc.params(w, h, s_, depth, mode="nee", rr=rr, seed=11 + s_)
    fb, u8 = sc.frame(p)
    fb_w, u8_w, bad, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat)
    assert not bad.any()
    same((fb, u8), (fb_w, u8_w))
    off = sc.frame(sc.params(w, h, s_, depth, rr=rr, seed=11 + s_))
    if depth == 1:                                        # no sample at the last bounce: the flag changes nothing
        same((fb, u8), off)
    else:                                                 # and otherwise it does (what fails while the bit is ignored)
        assert not np.array_equal(fb, off[0])


BIG_CASES = [(2, 1, False), (2, 2, False), (8, 5, True), (13, 8, False)]


@pytest.mark.parametrize("lamp", [False, True], ids=["stock", "lamp"])
@pytest.mark.parametrize("s_,depth,rr", BIG_CASES)
def test_frame_bitwise_1030_spheres_by_tiles_and_through_the_grid(apt, lamp, s_, depth, rr):
    sc = _scene(apt, "big1030", lamp)
    p = sc.params(24, 16, s_, depth, mode="nee", rr=rr, grid=True)
    fb_g, u8_g = sc.frame(p)
    fb_t, u8_t = sc.frame(sc.params(24, 16, s_, depth, mode="nee", rr=rr, grid=False))
    same((fb_g, u8_g), (fb_t, u8_t))                         # grid form == tile form, flag on
    fb_w, u8_w, bad, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat)
    assert not bad.any()
    same((fb_t, u8_t), (fb_w, u8_w))
    off = sc.frame(sc.params(24, 16, s_, depth, rr=rr, grid=True))
    if depth == 1:
        same((fb_g, u8_g), off)
    else:
        assert not np.array_equal(fb_g, off[0])


def test_the_lamp_is_binned_in_the_grid(apt):
    """With the lamp the light is no longer in the always-tested list: shadow rays find it by walking cells."""
    stock, lamp = _scene(apt, "big1030", False), _scene(apt, "big1030", True)
    assert int(lamp.hgrid[6]) == int(stock.hgrid[6]) - 1      # GridHeader.nlarge (pt_core.h)
    demo = _scene(apt, "demo9", True)
    sc = Scene(apt, demo.sph, demo.mat, demo.ns, light=demo.light, grid=True)     # a degenerate grid: nothing is large
    p = sc.params(48, 32, 8, 5, mode="nee", rr=True, seed=11, grid=True)
    fb, u8 = sc.frame(p)
    same((fb, u8), sc.frame(sc.params(48, 32, 8, 5, mode="nee", rr=True, seed=11, grid=False)))
    fb_w, u8_w, _, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat)
    same((fb, u8), (fb_w, u8_w))


@pytest.mark.parametrize("name,grid,b,c", [("diff8", False, 517, 700), ("demo9", False, 517, 700), ("big1030", True, 117, 203),
                                           ("big1030", False, 117, 203)])
def test_frame_mid_image_pixel_range(apt, name, grid, b, c):
    sc = _scene(apt, name, True)
    w, h = (48, 32) if name != "big1030" else (24, 16)
    p = sc.params(w, h, 16, 5, mode="nee", seed=2, grid=grid, flags=apt.APT_FLAG_RETIRE)      # RETIRE: accepted, changes nothing
    fb, u8 = sc.frame(p, pixel_begin=b, pixel_count=c)
    fb_w, u8_w, _, _ = mr.render_frame(oracle_params(p.copy(flags=p.flags & ~apt.APT_FLAG_RETIRE)), sc.sph, sc.mat, pixel_begin=b, pixel_count=c)
    same((fb, u8), (fb_w, u8_w))


@pytest.mark.parametrize("lamp", [False, True], ids=["stock", "lamp"])
@pytest.mark.parametrize("name,grid", [("diff8", False), ("demo9", False), ("big1030", False), ("big1030", True)])
def test_paths_bitwise_with_ranges(apt, name, grid, lamp):
    from oracle import oracle
    sc = _scene(apt, name, lamp)
    p = sc.params(16, 16, 4, 8, mode="nee", rr=True, seed=9, grid=grid)
    rays = oracle.gen_rays_counter(oracle_params(p))
    n = rays.shape[1]
    want, bad, segments = mr.trace(rays, sc.sph, sc.mat, sc.ns, 8, p.eps, p.seed, np.arange(n, dtype=np.uint64), rr_start=2, light=sc.light, nee=True, gloss=False)
    assert not bad.any()
    with apt.render.TraceCounter() as tc:
        got = sc.paths(p, rays)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5]
    assert tc.value == segments > n                       # shadow segments count as traced segments
    b, c = 1001, 1537                                     # a path range of the whole-image buffers, then the same range in band buffers
    got = sc.paths(p.copy(path_begin=b, path_count=c), rays)
    assert np.array_equal(got[:, b:b + c].view(np.uint32), want[:, b:b + c].view(np.uint32))
    assert np.isnan(got[:, :b]).all() and np.isnan(got[:, b + c:]).all()
    pb = p.copy(path_begin=b, path_count=c, flags=p.flags | apt.APT_FLAG_BAND_BUFFERS)
    got = sc.paths(pb, np.ascontiguousarray(rays[:, b:b + c]))
    assert np.array_equal(got.view(np.uint32), want[:, b:b + c].view(np.uint32))
    for depth in (1, 2, 5):                               # no roulette, the other depths
        q = sc.params(16, 16, 4, depth, mode="nee", seed=9, grid=grid)
        want, _, _ = mr.trace(rays, sc.sph, sc.mat, sc.ns, depth, q.eps, q.seed, np.arange(n, dtype=np.uint64), light=sc.light, nee=True, gloss=False)
        got = sc.paths(q, rays)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), depth
        if depth == 1:
            off = sc.paths(sc.params(16, 16, 4, 1, seed=9, grid=grid), rays)
            assert np.array_equal(got.view(np.uint32), off.view(np.uint32))


def test_a_light_of_any_material_needs_no_special_case(apt):
    """A mirror light with a non-zero albedo: bit for bit the restatement (the header gives it no special case)."""
    base = _scene(apt, "demo9", True)
    sph, mat = base.sph.copy(), base.mat.copy()
    mat[base.light] = 0                                   # APT_MAT_SPEC
    sph[:90].reshape(10, 9)[7:, base.light] = 0.5
    sc = Scene(apt, sph, mat, base.ns, light=base.light)
    p = sc.params(48, 32, 8, 6, mode="nee", seed=5)
    fb, u8 = sc.frame(p)
    fb_w, u8_w, _, _ = mr.render_frame(oracle_params(p), sc.sph, sc.mat)
    same((fb, u8), (fb_w, u8_w))


# ---- against the renderer that exists: the same launches without the flag (the yardstick is the flag-off path, never the new code) ----
def _on_off(apt, name, lamp, depth, seed):
    """-> (radiance with the flag, without it, the camera ray hits an emitter) for 2^17 camera rays; float64 [3][n], bool [n]."""
    from oracle import oracle
    sc = _scene(apt, name, lamp)
    p = sc.params(128, 64, 4, depth, mode="nee", seed=seed)
    assert p.num_paths == 1 << 17
    rays = oracle.gen_rays_counter(oracle_params(p))
    on = sc.paths(p, rays).astype(np.float64)
    off = sc.paths(sc.params(128, 64, 4, depth, seed=seed), rays).astype(np.float64)
    first = sc.paths(sc.params(128, 64, 4, 1, seed=seed), rays)
    return on, off, first.any(axis=0)


# z-scores of these inputs on the CPU restatement (which the GPU equals bit for bit, so the test is deterministic), per channel:
#   diff8 stock depth 2: -0.15 -0.25 -0.35      diff8 stock depth 5: -0.06 -0.15 -0.10
#   diff8 lamp  depth 5: -0.03 +0.06 +0.30      demo9 lamp  depth 8: -0.01 -0.04 +0.18      (all with seed 21: comfortably inside 4)
@pytest.mark.parametrize("name,lamp,depth,seed", [("diff8", False, 2, 21), ("diff8", False, 5, 21), ("diff8", True, 5, 21),
                                                  ("demo9", True, 8, 21)])
def test_same_expectation_as_the_plain_renderer(apt, name, lamp, depth, seed):
    on, off, _ = _on_off(apt, name, lamp, depth, seed)
    n = on.shape[1]
    for ch in range(3):
        s_on, s_off = on[ch].std(ddof=1) / np.sqrt(n), off[ch].std(ddof=1) / np.sqrt(n)
        z = (on[ch].mean() - off[ch].mean()) / np.hypot(s_on, s_off)
        print("%s lamp %s depth %d channel %d: on %.5f +- %.5f  off %.5f +- %.5f  z %+.2f" % (name, lamp, depth, ch, on[ch].mean(), s_on,
                                                                                            off[ch].mean(), s_off, z))
        assert s_on > 0 and s_off > 0
        assert abs(on[ch].mean() - off[ch].mean()) < 4 * np.hypot(s_on, s_off)


def test_less_variance_on_the_lamp_scene(apt):
    """Over the paths whose camera ray does not hit the lamp, the per-channel sample variance with the flag is smaller than that
    of the plain renderer on the same rays.  (The ratio for the stock light is printed, not asserted: ~1 is expected there.  The
    restatement gives 2042 / 912 / 499 per channel for the lamp and 1.05 / 0.91 / 0.83 for the stock light on these inputs.)"""
    on, off, direct = _on_off(apt, "diff8", True, 5, 21)
    assert 0 < direct.sum() < direct.size // 100          # the lamp is small
    for ch in range(3):
        v_on, v_off = on[ch][~direct].var(ddof=1), off[ch][~direct].var(ddof=1)
        print("lamp: channel %d variance off / on = %.2f" % (ch, v_off / v_on))
        assert v_off / v_on > 1
    on, off, direct = _on_off(apt, "diff8", False, 5, 21)
    for ch in range(3):
        print("stock light: channel %d variance off / on = %.2f" % (ch, off[ch][~direct].var(ddof=1) / on[ch][~direct].var(ddof=1)))
