"""The first bounce of a path pair is a form of its own (pt_trace2.h bounce2_ns8_first: throughput 1 and full alive masks are known, the
new throughput is the albedo entry itself), and the two-path bounce divides through the reciprocal refined from the square root's seed
(pt_core.h div3_seeded_packed2).  Frames through the two-path kernel against the oracle, bit for bit (fb and fb_u8), at the smallest
shapes that reach every edge of the new loop:

  S = 16: one pair per lane; S = 24: one pair, then the single-sample chain member and the tail
  depth 1: last only (as a first bounce); 2: first + last; 3: first + one step + last; 4: first + one loop turn + last; 8: the headline
  K- and O-mode; the reference table (shared planes) and the table with spheres 0 and 6 exchanged (the general form)
  eps outside the root-key range: the first bounce's exact form runs
  buffer mode at 2^20 paths, depth 3: render_paths2_kernel"""
import numpy as np
import pytest

import test_gpu_launch_matrix as lm

K, O = 0, 1
W, H = 16, 8
DEPTHS = (1, 2, 3, 4, 8)


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()                   # a no-op when the in-tree library is current
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.render, pkg.gen_data = render, gen_data
    return pkg


def _general_scene(oracle):
    """Spheres 0 and 6 exchanged, as bench.py's general_scene_ms builds it: the scene does not share planes, the general intersections run."""
    t = oracle.gen_spheres().copy()
    tab = t[:80].reshape(10, 8)
    tab[:, [0, 6]] = tab[:, [6, 0]]
    return t


def _frame_equals_oracle(apt, oracle, scene, s, depth, mode, eps=1e-4):
    import torch
    d_scene = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.float32)).cuda()
    fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(W, H, s, depth=depth, eps=eps, mode=mode, seed=11), scene,
                                           threads=oracle.max_threads())
    with apt.render.TraceCounter() as tc:
        fb, u8 = apt.render.render_frame(apt.make_params(W, H, s, depth=depth, eps=eps, mode=mode, seed=11), d_scene)
    torch.cuda.synchronize()
    ok, where = lm._same(fb.cpu().numpy(), fb_w)
    assert ok, (s, depth, mode, eps, where)
    assert np.array_equal(u8.cpu().numpy(), u8_w), (s, depth, mode, eps)
    return tc


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("scene", ("ref", "general"))
@pytest.mark.parametrize("depth", DEPTHS)
def test_two_path_frames_at_every_shape_of_the_peeled_loop(apt, oracle, depth, scene, mode):
    table = oracle.gen_spheres() if scene == "ref" else _general_scene(oracle)
    for s in (16, 24):
        _frame_equals_oracle(apt, oracle, table, s, depth, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", (1, 2, 3))
def test_first_bounce_in_the_exact_form(apt, oracle, depth, mode):
    """eps = 0: eps_allows_rootkey() is false, every bounce of the pair -- the first, which starts from no throughput registers, and the
    last, alone at depth 1 -- is the exact form; the statistics block counts those re-runs."""
    for s in (16, 24):
        tc = _frame_equals_oracle(apt, oracle, oracle.gen_spheres(), s, depth, mode, eps=0.0)
        assert tc.exact_reruns > 0, (s, depth, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
def test_buffer_mode_two_path_kernel_depth_3(apt, oracle, mode):
    """render_do_ex on exactly 2^20 paths: render_paths2_kernel (first + one step + last), the degenerate rays in both halves of a pair."""
    import torch
    row = dict(w=lm.BIG_W, h=lm.BIG_H, s=1, depth=3, eps=1e-4, mode=mode, flags=0, path_begin=0, path_count=lm.TWO_PATH_MIN, band=False)
    scene = oracle.gen_spheres()
    got, want, _ = lm._run_paths(apt, oracle, row, scene, 8, torch.from_numpy(scene).cuda())
    ok, where = lm._same(got, want)
    assert ok, (mode, where)
