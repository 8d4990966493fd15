"""The two-path bounce of a scene that shares planes solves each sphere ONCE for the lane's two paths (pt_trace2.h
intersect2_ns8_planes: every packed instruction holds path A's and path B's value of one quantity of one sphere) and branches round
the root stage of the ball or the light when no lane of the wave can reach it in either path (kAbSkip).  No result may change:

  frames      the reference scene through the fused frame kernel, K- and O-mode, bit for bit against the oracle, at 48x27 (the whole
              view at low resolution: single waves straddle wall edges, corners, the ball and the light's cap) and 50x3 (the last
              workgroup has lanes past the image), depth 1, 2, 3, 4 and 8 (last-as-first, first + last, both ping-pong exits, the
              headline's loop), 16, 24 and 40 samples (an even chain, a chain with an odd member, an n % 8 tail)
  tables      two more shared-planes tables at 48x27: the ball moved behind the camera (out of reach of every wave: the stage is always
              branched round), and the light grown round the camera rays' origins (c < 0 in every lane: the predicate must keep it)
  buffer      one render_do_ex row of 2^20 paths, the smallest range that render_paths2_kernel takes
  fused MT    one frame of a single 78-pixel group through the fused MT19937 kernel against the three-kernel pipeline, whose trace is
              the one-path kernel

and the exact re-runs of a 48x27 frame must not rise: a skipped stage leaves its discriminant out of the validity chain, a stage that
runs for one path's sake adds the other path's.  Measured on this input (K-mode, 16 samples, depth 8, seed 5): parent commit 0 exact
re-runs, this form 0 (at 480x270, seed 0: 20 and 19 of 129 600 waves)."""
import numpy as np
import pytest

import pair67_ref as pr

K, O = 0, 1
SIZES = ((48, 27), (50, 3))
DEPTHS = (1, 2, 3, 4, 8)
SAMPLES = (16, 24, 40)
SEED = 5
PARENT_EXACT_RERUNS_48x27 = 0


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
    t = oracle.gen_spheres().copy()
    tab = t[:80].reshape(10, 8)
    if name == "ball_behind":        # the mirror ball 100 behind the camera (rays start at z <= 295.6 and point to -z)
        tab[1, 6], tab[2, 6], tab[3, 6] = 50.0, 52.0, 400.0
    elif name == "inside_light":     # the light, r = 300, round the camera: its cx and cz are shared planes and stay, cy moves to the camera's
        tab[0, 7] = np.float32(300.0 * 300.0)
        tab[2, 7] = 52.0
    else:
        assert name == "ref"
    return t


_WANT = {}


def _oracle_frame(oracle, name, w, h, s, depth, mode):
    key = (name, w, h, s, depth, mode)
    if key not in _WANT:
        fb, u8, _, _ = oracle.render_frame(oracle.make_params(w, h, s, depth=depth, mode=mode, seed=SEED), _scene(oracle, name),
                                           threads=oracle.max_threads())
        fb.setflags(write=False)
        u8.setflags(write=False)
        _WANT[key] = (fb, u8)
    return _WANT[key]


def _check_frame(apt, oracle, name, w, h, s, depth, mode):
    import torch
    fb_w, u8_w = _oracle_frame(oracle, name, w, h, s, depth, mode)
    fb, u8 = apt.render.render_frame(apt.make_params(w, h, s, depth=depth, mode=mode, seed=SEED), torch.from_numpy(_scene(oracle, name)).cuda())
    torch.cuda.synchronize()
    ok, where = pr.same(fb.cpu().numpy(), fb_w)
    assert ok, (name, w, h, s, depth, mode, where)
    assert np.array_equal(u8.cpu().numpy(), u8_w), (name, w, h, s, depth, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("size", SIZES, ids=("48x27", "50x3"))
def test_reference_scene_frames_equal_the_oracle(apt, oracle, size, depth, mode):
    for s in SAMPLES:
        _check_frame(apt, oracle, "ref", size[0], size[1], s, depth, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("name", ("ball_behind", "inside_light"))
def test_moved_spheres_equal_the_oracle(apt, oracle, name, mode):
    for depth in (1, 2, 8):
        _check_frame(apt, oracle, name, 48, 27, 16, depth, mode)


def test_what_the_moved_tables_are_for(oracle):
    """ball_behind: b < 0 and c > 0 for the ball at the camera rays of every path; inside_light: c < 0 for the light there, so the
    predicate holds for no lane although b takes both signs."""
    for name, k in (("ball_behind", 6), ("inside_light", 7)):
        tab = _scene(oracle, name)[:80].reshape(10, 8)
        assert all(tab[1, j].view(np.uint32) == tab[1, 2].view(np.uint32) for j in (3, 4, 5, 7))      # still a shared-planes table
        assert all(tab[3, j].view(np.uint32) == tab[3, 0].view(np.uint32) for j in (1, 4, 5, 7))
        rays = oracle.gen_rays_counter(oracle.make_params(48, 27, 16, depth=8, mode=K, seed=SEED))
        f = np.float32
        ocx, ocy, ocz = tab[1, k] - rays[0], tab[2, k] - rays[1], tab[3, k] - rays[2]
        b = ocx * rays[3]
        b = b + ocy * rays[4]
        b = b + ocz * rays[5]
        c = ocx * ocx
        c = c + ocy * ocy
        c = c + ocz * ocz
        c = c - tab[0, k]
        assert b.dtype == f and c.dtype == f
        held = pr.cannot_hit(b, c, b * b - c)
        if name == "ball_behind":
            assert (b < 0).all() and (c > 0).all() and held.all()
        else:
            assert (c < 0).all() and not held.any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
def test_buffer_row_of_two_path_size(apt, oracle, mode):
    """2^20 paths: the smallest range render_do_ex hands to render_paths2_kernel (render_kernels.hip kTwoPathBufferMin)."""
    import torch
    p = oracle.make_params(512, 512, 1, depth=5, mode=mode, seed=SEED)
    rays = oracle.gen_rays_counter(p)
    assert rays.shape[1] == 1 << 20
    sph = oracle.gen_spheres()
    want, _ = oracle.render_paths(p, rays, sph, threads=oracle.max_threads())
    colors = torch.zeros(3 << 20, device="cuda")
    apt.render.render_do_ex(apt.make_params(512, 512, 1, depth=5, mode=mode, seed=SEED), None, torch.from_numpy(np.ascontiguousarray(rays).ravel()).cuda(),
                            torch.from_numpy(sph).cuda(), colors)
    torch.cuda.synchronize()
    ok, where = pr.same(colors.cpu().numpy().reshape(3, -1), want)
    assert ok, (mode, where)


@pytest.mark.gpu
def test_fused_mt_frame_of_one_group(apt):
    """13 x 6 = 78 pixels, one group of the fused MT19937 kernel, 16 samples: against gen_rays_mt -> render_do_ex -> decode_color."""
    import torch
    for mode in (apt.APT_MODE_ORACLE, apt.APT_MODE_KERNEL):
        fb, u8, _ = apt.render.render_reference_frame(13, 6, 16, depth=8, seed=0, mode=mode)
        fb_f, u8_f = apt.render.render_reference_frame_fused(13, 6, 16, depth=8, seed=0, mode=mode)
        torch.cuda.synchronize()
        assert torch.equal(fb.view(torch.int32), fb_f.view(torch.int32)) and torch.equal(u8, u8_f), mode


@pytest.mark.gpu
def test_exact_reruns_do_not_rise(apt, oracle):
    import torch
    sph = torch.from_numpy(oracle.gen_spheres()).cuda()
    with apt.render.TraceCounter() as tc:
        apt.render.render_frame(apt.make_params(48, 27, 16, depth=8, seed=SEED), sph)
    reruns = int(tc.buf[3].item())
    print("exact re-runs at 48x27:", reruns, "parent:", PARENT_EXACT_RERUNS_48x27)
    assert tc.value == 48 * 27 * 4 * 16 * 8
    assert reruns <= PARENT_EXACT_RERUNS_48x27
