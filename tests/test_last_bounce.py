"""The last bounce of a fully traced path is hit-only: nothing traces the ray it would produce, so the full-trace loops of the 8-sphere
scene (pt_trace2.h trace2_ns8_t, pt_trace.h trace_ns8 without retirement) end with the intersections, the alive mask and the albedo
product.  CPU: the headline kernel's ISA holds such blocks and stays within its register budget.  GPU: every kernel that runs one of the two
loops against the oracle, bit for bit, at the depths where the last bounce is the only one, follows an odd or an even number of full
bounces, or is redone in the exact form."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import test_gpu_launch_matrix as lm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascendpathtracing_amd", "csrc")
HEADLINE = "_ZN12_GLOBAL__N_119render_frame_kernelILi0ELi0ELi8ELb0ELb1EEEvPKfNS_9FrameArgsENS_9TraceArgsEN3apt8LeafProgE"
K, O = 0, 1
DEPTHS = (1, 2, 3, 4, 7, 8)


# ---- CPU: the ISA ----------------------------------------------------------------------------------------------------------------------
def _regions(lines):
    """Straight-line regions of a kernel's ISA (cut after every branch): per region the counts of the instructions that tell a full
    pair-bounce from a hit-only one."""
    out, cur = [], {"min3": 0, "rcp": 0, "rsq": 0, "ds_read": 0}
    for line in lines:
        s = line.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        op = s.split()[0]
        for key, prefix in (("min3", "v_min3_u32"), ("rcp", "v_rcp_f32"), ("rsq", "v_rsq_f32"), ("ds_read", "ds_read_b32")):
            if op.startswith(prefix):
                cur[key] += 1
        if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
            out.append(cur)
            cur = {"min3": 0, "rcp": 0, "rsq": 0, "ds_read": 0}
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_headline_kernel_has_hit_only_last_bounces_and_keeps_its_registers():
    subprocess.run(["make", "-s", "-C", CSRC, "asm"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(os.path.join(CSRC, "render_kernels.s")).read()
    begin = text.index("\n" + HEADLINE + ":")
    end = text.index(".end_amdhsa_kernel", begin)
    regions = _regions(text[begin:end].split("\n"))
    # a complete pair intersection is 16 v_min3_u32 (8 spheres, two paths); the shading step adds two v_rsq_f32 (|normal|), the six
    # ds_read_b32 of the hit centres and, behind the validity branch, the reciprocals
    pair = [r for r in regions if r["min3"] == 16]
    assert all(r["rcp"] == 0 for r in pair)
    hit_only = [r for r in pair if r["rsq"] == 16 and r["ds_read"] == 6]
    full = [r for r in pair if r["rsq"] == 18 and r["ds_read"] == 12]
    assert len(hit_only) + len(full) == len(pair), "a pair-bounce block that is neither the full nor the hit-only form"
    # one copy of the trace loop holds at most three full pair-bounces (two in the loop body, one when depth - 1 is odd): at least one
    # hit-only block per copy
    assert full and len(hit_only) >= 2 and 3 * len(hit_only) >= len(full), (len(hit_only), len(full))
    # the resource lines the assembler prints behind the kernel
    tail = text[end:end + 4000]
    res = {k: int(v) for k, v in re.findall(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)$", tail, re.M)[:3]}
    assert set(res) == {"NumVgprs", "ScratchSize", "Occupancy"}, res
    assert res["ScratchSize"] == 0 and res["NumVgprs"] <= 128 and res["Occupancy"] >= 4, res


# ---- GPU -------------------------------------------------------------------------------------------------------------------------------
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
    """Spheres 0 and 6 exchanged, as bench.py's general_scene_ms builds it: scene8_shares_planes() fails, the general form of the
    intersections runs."""
    t = oracle.gen_spheres().copy()
    tab = t[:80].reshape(10, 8)
    tab[:, [0, 6]] = tab[:, [6, 0]]
    return t


def _frame_equals_oracle(apt, oracle, scene, s, depth, mode, eps=1e-4, w=9, h=7, counter=False):
    import torch
    d_scene = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.float32)).cuda()
    fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(w, h, s, depth=depth, eps=eps, mode=mode, seed=9), scene,
                                           threads=oracle.max_threads())
    p = apt.make_params(w, h, s, depth=depth, eps=eps, mode=mode, seed=9)
    tc = None
    if counter:
        with apt.render.TraceCounter() as tc:
            fb, u8 = apt.render.render_frame(p, d_scene)
    else:
        fb, u8 = apt.render.render_frame(p, d_scene)
    torch.cuda.synchronize()
    ok, where = lm._same(fb.cpu().numpy(), fb_w)
    assert ok, (s, depth, mode, eps, where)
    assert np.array_equal(u8.cpu().numpy(), u8_w), (s, depth, mode, eps)
    return tc


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("scene", ("ref", "general"))
@pytest.mark.parametrize("depth", DEPTHS)
def test_frame_kernels_at_every_last_bounce_position(apt, oracle, depth, scene, mode):
    """S = 8: one path per lane (trace_ns8); S = 16: two paths per lane (trace2_ns8); S = 17: both in one kernel (the odd sample)."""
    table = oracle.gen_spheres() if scene == "ref" else _general_scene(oracle)
    for s in (8, 16, 17):
        _frame_equals_oracle(apt, oracle, table, s, depth, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", (2, 5))
def test_buffer_mode_two_path_loop(apt, oracle, depth, mode):
    """>= 2^20 paths: render_paths2_kernel, with the degenerate ray set in both halves of a lane pair."""
    import torch
    row = dict(w=lm.BIG_W, h=lm.BIG_H, s=1, depth=depth, eps=1e-4, mode=mode, flags=0, path_begin=0, path_count=0, band=False)
    scene = oracle.gen_spheres()
    got, want, _ = lm._run_paths(apt, oracle, row, scene, 8, torch.from_numpy(scene).cuda())
    ok, where = lm._same(got, want)
    assert ok, (depth, mode, where)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", (1, 2, 5, 8))
def test_buffer_mode_single_path_loop(apt, oracle, depth, mode):
    """< 2^20 paths: render_paths_kernel<mode, 0, false>."""
    import torch
    row = dict(w=16, h=16, s=4, depth=depth, eps=1e-4, mode=mode, flags=0, path_begin=7, path_count=3001, band=False)
    scene = oracle.gen_spheres()
    got, want, _ = lm._run_paths(apt, oracle, row, scene, 8, torch.from_numpy(scene).cuda())
    ok, where = lm._same(got, want)
    assert ok, (depth, mode, where)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", (3, 4))
def test_fused_mt19937_kernels_at_an_odd_and_an_even_depth(apt, oracle, depth, mode):
    import torch
    scene = oracle.gen_spheres()
    d_scene = torch.from_numpy(scene).cuda()
    for s, rng in ((8, None), (7, (41, 100))):       # render_frame_mt_kernel, render_frame_mt_any_kernel
        row = dict(w=23, h=11, s=s, range=rng, depth=depth, eps=1e-4, mode=mode, flags=0, counter=False)
        (fb, u8), (fb_w, u8_w), _ = lm._run_mt(apt, oracle, row, scene, d_scene)
        ok, where = lm._same(fb, fb_w)
        assert ok, (s, depth, mode, where)
        assert np.array_equal(u8, u8_w), (s, depth, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", (1, 3))
@pytest.mark.parametrize("eps", (0.0, 1e21))
def test_last_bounce_in_the_exact_form(apt, oracle, eps, depth, mode):
    """eps outside the root-key range: the wave redoes every bounce, the last one included, in the exact form and keeps its
    throughput and alive results only."""
    for s in (8, 16):
        _frame_equals_oracle(apt, oracle, oracle.gen_spheres(), s, depth, mode, eps=eps)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("depth", (1, 2))
def test_last_bounce_validity_on_degenerate_operands(apt, oracle, depth, mode):
    """The scene whose back wall has radius 2^31 and whose albedos are inf / NaN / 0: the last bounce's validity test sees the
    discriminants only."""
    scene, _ = lm._scene(apt, "nonfinite")
    for s in (8, 16):
        _frame_equals_oracle(apt, oracle, scene, s, depth, mode)
