"""GPU tests of the drop-in boundary itself (run with -m gpu): the reference's C++-linkage declaration called
through unmodified, the per-call error record, contexts used from several host threads, the host-pointer
(CPU-simulator shaped) entry and the one-process multi-GPU object.  All results bit-exact."""
import ctypes
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.render, pkg.gen_data = render, gen_data
    return pkg


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).ravel()).cuda()


def test_reference_cxx_declaration_calls_through(apt, golden, oracle, tmp_path):
    """A TU with src/main.cpp:9-10's declaration verbatim (C++ linkage), compiled by g++ and linked against the
    library unchanged, drives the GPU: same colours as the CPU restatement."""
    from test_host_abi import build_reference_decl_shim
    data, _ = golden
    shim = ctypes.CDLL(build_reference_decl_shim(apt, str(tmp_path)))
    shim.call_through_reference_declaration.restype = None
    rays, sph = dev(data["16x16_s1_rays"]), dev(data["spheres"])
    colors = torch.full((3 * 1024,), float("nan"), device="cuda")
    apt.render.set_default_params(apt.default_params())
    shim.call_through_reference_declaration(ctypes.c_uint32(8), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                            ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(sph.data_ptr()),
                                            ctypes.c_void_p(colors.data_ptr()))
    torch.cuda.synchronize()
    assert apt._lib.lib().apt_last_status() == 0
    want, _ = oracle.render_paths(oracle.make_params(16, 16, 1, depth=5, mode=oracle.MODE_K), data["16x16_s1_rays"],
                                  data["spheres"])
    assert np.array_equal(bits(colors), bits(want).ravel())


def test_failed_call_does_not_poison_the_next_render_do(apt, golden, oracle):
    """the error record was only ever set.  A rejected call followed by a good render_do on the same
    thread must succeed (the Python wrapper raises on a non-zero status)."""
    data, _ = golden
    rays, sph = dev(data["16x16_s1_rays"]), dev(data["spheres"])
    colors = torch.zeros(3 * 1024, device="cuda")
    with pytest.raises(apt.AptError):
        apt.render.render_do_ex(apt.make_params(16, 16, 1, path_begin=10 ** 9), None, rays, sph, colors)
    with pytest.raises(apt.AptError):
        apt.render.set_refill_lanes(0)
    apt.render.set_default_params(apt.default_params())
    apt.render.render_do(8, None, None, rays, sph, colors)         # must not raise
    torch.cuda.synchronize()
    want, _ = oracle.render_paths(oracle.make_params(16, 16, 1, depth=5), data["16x16_s1_rays"], data["spheres"])
    assert np.array_equal(bits(colors), bits(want).ravel())
    assert apt._lib.lib().apt_last_error() == b""


def test_contexts_render_different_sizes_from_two_threads(apt, golden, oracle):
    """Two host threads, two contexts with different parameters, each on its own stream, interleaved calls:
    every result equals the oracle's for ITS parameters (the process-wide defaults would race)."""
    data, _ = golden
    sph = dev(data["spheres"])
    jobs = {"a": ("16x16_s1", 16, 16, 1, 5), "b": ("32x32_s1", 32, 32, 1, 8)}
    out, errs = {}, []

    def work(tag):
        try:
            key, w, h, s, d = jobs[tag]
            rays = dev(data[f"{key}_rays"])
            ctx = apt.render.Context(apt.make_params(w, h, s, depth=d))
            stream = torch.cuda.Stream()
            res = []
            torch.cuda.synchronize()                      # rays / sph were made on the default stream
            with torch.cuda.stream(stream):               # buffers are zeroed on the stream the render runs on
                for _ in range(20):
                    colors = torch.zeros(3 * w * h * 4 * s, device="cuda")
                    ctx.render_do(8, None, stream, rays, sph, colors)
                    res.append(colors)
            stream.synchronize()
            out[tag] = res
            ctx.close()
        except Exception as e:   # noqa: BLE001
            errs.append((tag, repr(e)))

    ts = [threading.Thread(target=work, args=(t,)) for t in jobs]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for tag, (key, w, h, s, d) in jobs.items():
        want, _ = oracle.render_paths(oracle.make_params(w, h, s, depth=d), data[f"{key}_rays"], data["spheres"])
        for colors in out[tag]:
            assert np.array_equal(bits(colors), bits(want).ravel()), tag


def test_context_refill_knob_and_counter_are_private(apt, oracle):
    sph = dev(oracle.gen_spheres())
    p = apt.make_params(24, 10, 16, depth=8, flags=apt.APT_FLAG_RETIRE, seed=3)
    ref, ref8 = apt.render.render_frame(p, sph)
    ctx = apt.render.Context()
    ctx.set_refill_lanes(5)
    counter = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctx.set_trace_counter(counter)
    fb, u8 = ctx.render_frame(p, sph)
    torch.cuda.synchronize()
    assert torch.equal(fb.view(torch.int32), ref.view(torch.int32)) and torch.equal(u8, ref8)
    _, _, _, traced = oracle.render_frame(oracle.make_params(24, 10, 16, depth=8, flags=oracle.FLAG_RETIRE, seed=3),
                                          oracle.gen_spheres())
    assert int(counter[0]) == traced
    with apt.render.TraceCounter() as tc:        # the default context's counter saw nothing of ctx's launch
        pass
    assert tc.value == 0
    ctx.close()


def test_host_pointer_entry_cpu_simulator_shape(apt, golden, oracle):
    """apt_render_host: HOST buffers in and out, synchronous (the ICPU_RUN_KF(render, ...) shape, src/main.cpp:37)."""
    data, _ = golden
    rays = np.ascontiguousarray(data["16x16_s2_rays"], dtype=np.float32).ravel()
    sph = np.ascontiguousarray(data["spheres"], dtype=np.float32)
    colors = np.zeros(3 * 16 * 16 * 4 * 2, dtype=np.float32)
    apt.render.set_default_params(apt.make_params(16, 16, 2, depth=5, mode=apt.APT_MODE_ORACLE))
    apt.render.render_host(8, rays, sph, colors)
    apt.render.set_default_params(apt.default_params())
    assert np.array_equal(bits(colors), bits(data["16x16_s2_d5_soa"]).ravel())      # == the reference's test_soa.bin


@pytest.mark.parametrize("bands,stripes", [(1, 1), (2, 1), (3, 1), (2, 5), (4, 3)])
def test_one_process_multi_gpu_object(apt, oracle, bands, stripes):
    """apt_multi on ONE physical GPU (every band on device 0: separate streams, peer-copy path device 0 -> 0):
    contiguous bands and interleaved stripes give the single-launch frame bit for bit, uneven splits included."""
    sph_host = oracle.gen_spheres()
    p = apt.make_params(37, 23, 16, depth=6, seed=11)                  # 851 pixels: not divisible by 2, 3, 10 or 12
    ref, ref8 = apt.render.render_frame(p, dev(sph_host))
    mg = apt.render.MultiGpu(p, sph_host, [0] * bands, stripes=stripes)
    for _ in range(2):
        fb, u8 = mg.render()
        assert torch.equal(fb.view(torch.int32), ref.view(torch.int32)) and torch.equal(u8, ref8)
    assert len(mg.band_kernel_ms) == bands and all(ms >= 0 for ms in mg.band_kernel_ms)
    mg.close()
    with pytest.raises(apt.AptError):
        apt.render.MultiGpu(p, sph_host, [0, 99])


def test_host_pointer_entry_accepts_the_whole_range_and_rejects_strict_sub_ranges(apt, golden):
    """path_begin = 0 with path_count = N is the whole frame (valid, as path_count = 0 is); only a strict
    sub-range would copy back colours no kernel wrote and is refused with APT_ERR_ARG."""
    data, _ = golden
    rays = np.ascontiguousarray(data["16x16_s2_rays"], dtype=np.float32).ravel()
    sph = np.ascontiguousarray(data["spheres"], dtype=np.float32)
    n = 16 * 16 * 4 * 2
    try:
        colors = np.zeros(3 * n, dtype=np.float32)
        apt.render.set_default_params(apt.make_params(16, 16, 2, depth=5, mode=apt.APT_MODE_ORACLE, path_begin=0, path_count=n))
        apt.render.render_host(8, rays, sph, colors)
        assert np.array_equal(bits(colors), bits(data["16x16_s2_d5_soa"]).ravel())
        for b, c in ((1, 0), (0, n - 1), (5, 10)):
            apt.render.set_default_params(apt.make_params(16, 16, 2, depth=5, path_begin=b, path_count=c))
            with pytest.raises(apt.AptError):
                apt.render.render_host(8, rays, sph, colors)
            assert apt._lib.lib().apt_last_status() == 1          # APT_ERR_ARG
    finally:
        apt.render.set_default_params(apt.default_params())


def test_debug_knobs_are_context_state_not_environment(apt, oracle, monkeypatch):
    """kernels are selected through apt_context_set_debug, per context; nothing in a launch path reads the
    process environment.  Unknown keys and out-of-range values are APT_ERR_ARG; a knob set on one context does not leak into
    another (ppw = 1 on a private context gives the same frame and its own wave split)."""
    import os
    with pytest.raises(apt.AptError):
        apt.render.set_debug("no_such_knob", 1)
    with pytest.raises(apt.AptError):
        apt.render.set_debug("queue_ppw", 5000)
    with pytest.raises(apt.AptError):
        apt.render.set_debug("queue_nbuf", 1)
    sph = dev(oracle.gen_spheres())
    p = apt.make_params(24, 10, 16, depth=8, flags=apt.APT_FLAG_RETIRE, seed=3)
    monkeypatch.setenv("APT_QUEUE_PPW", "1")        # the default context exists already: the environment is not consulted again
    with apt.render.TraceCounter() as t_def:
        ref, ref8 = apt.render.render_frame(p, sph)
    monkeypatch.delenv("APT_QUEUE_PPW")
    ctx = apt.render.Context()
    ctx.set_debug("queue_ppw", 1)
    counter = torch.zeros(4, dtype=torch.int64, device="cuda")
    ctx.set_trace_counter(counter)
    fb, u8 = ctx.render_frame(p, sph)
    ctx.check()
    assert torch.equal(fb.view(torch.int32), ref.view(torch.int32)) and torch.equal(u8, ref8)
    # lane-slots of ray-generate (stats[2]): one batch of 64 per started batch -- with one pixel per wave every wave pads its last
    # batch, with the default split (4 pixels per wave at this size) fewer do: the two contexts ran different wave splits
    assert int(counter[0]) == t_def.stats[0] and int(counter[2]) >= t_def.stats[2]
    ctx.close()


def test_device_status_word_reports_a_tripped_loop_bound(apt, oracle, tmp_path):
    """VERDICT r3 item 3 (the reference asserts inside its kernel, src/render.cpp:68-73): a library built with
    -DAPT_TEST_TINY_GUARD (the loop bounds of the sample-queue kernels trip after three turns) must report APT_ERR_DEVICE
    through apt_check() -- sticky until checked, cleared by the check -- and apt_render_host / the normal library must not.
    Runs in a child process (a second copy of the library in one process would register its kernels twice)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    variant = os.path.join(root, "profiles", "microbench", "lib_tiny_guard.so")
    product = os.path.join(root, "ascendpathtracing_amd", "librender_mi355x.so")
    if not os.path.exists(variant) or os.path.getmtime(variant) < os.path.getmtime(product):   # a test build: made on demand, not by build()
        subprocess.run(["bash", os.path.join(root, "profiles", "build_variant.sh"), "tiny_guard", "-DAPT_TEST_TINY_GUARD"], check=True)
    code = r'''
import ctypes, sys, numpy as np, torch
sys.path.insert(0, %r)
import ascendpathtracing_amd as apt
from ascendpathtracing_amd import gen_data, render
sph = torch.from_numpy(gen_data.gen_spheres()).cuda()
lib = apt._lib.lib()
out = []
# 8-sphere queue, then the grid form: each trips its own bound
p = apt.make_params(24, 10, 16, depth=8, flags=apt.APT_FLAG_RETIRE, seed=3)
render.render_frame(p, sph)
rc1 = lib.apt_check(None); msg1 = lib.apt_last_error().decode()
rc1b = lib.apt_check(None)                       # cleared by the first check
scene = gen_data.gen_scene(300, seed=7)
grid = torch.from_numpy(gen_data.build_grid(scene, 300).view(np.int32)).cuda()
pg = apt.make_params(16, 12, 8, depth=6, num_spheres=300, seed=4, accel=grid.data_ptr())
render.render_frame(pg, torch.from_numpy(scene).cuda())
rc2 = lib.apt_check(None); msg2 = lib.apt_last_error().decode()
# a kernel without a loop bound reports nothing
render.render_frame(apt.make_params(24, 10, 16, depth=8, seed=3), sph)
rc3 = lib.apt_check(None)
print(rc1, rc1b, rc2, rc3, "|", msg1, "|", msg2)
''' % root
    def run(env_extra):
        env = dict(os.environ, **env_extra)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip().splitlines()[-1]
    tiny = run({"APT_LIB_PATH": variant})
    head, msg1, msg2 = [t.strip() for t in tiny.split("|")]
    assert head.split() == ["4", "0", "4", "0"], tiny                 # APT_ERR_DEVICE, cleared, APT_ERR_DEVICE, APT_OK
    assert "queue-loop-bound" in msg1 and "grid-walk-bound" in msg2, tiny
    normal = run({})
    assert normal.split("|")[0].split() == ["0", "0", "0", "0"], normal


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs (the driver's multi-GPU node)")
@pytest.mark.parametrize("stripes", [1, 3])
def test_one_process_multi_gpu_object_on_two_devices(apt, oracle, stripes):
    """apt_multi with bands on devices 0 AND 1 -- the peer-copy path between two devices, not 0 -> 0 --
    gives the single-launch frame bit for bit; the band on device 1 reports into ITS status word."""
    sph_host = oracle.gen_spheres()
    p = apt.make_params(37, 23, 16, depth=6, seed=11, flags=apt.APT_FLAG_RETIRE)
    ref, ref8 = apt.render.render_frame(p, dev(sph_host))
    mg = apt.render.MultiGpu(p, sph_host, [0, 1, 1, 0], stripes=stripes)
    for _ in range(2):
        fb, u8 = mg.render()
        assert fb.device.index == 0
        assert torch.equal(fb.view(torch.int32), ref.view(torch.int32)) and torch.equal(u8, ref8)
    mg.close()


def _run_sh(extra=()):
    """`bash run.sh -r gpu -v Ascend310P1 [-- ...]` as the reference's README runs it (README.md:30-31, run.sh:103-129):
    build -> gen_data -> ./render_gpu (render_do on the MI355X) -> data_visualization.  Returns (color.bin floats, color.ppm bytes)."""
    import os
    import subprocess
    from conftest import ROOT
    for f in ("output/color.bin", "output/color.ppm"):
        if os.path.exists(os.path.join(ROOT, f)):
            os.remove(os.path.join(ROOT, f))
    cmd = ["bash", os.path.join(ROOT, "run.sh"), "-r", "gpu", "-v", "Ascend310P1"] + (["--"] + list(extra) if extra else [])
    env = {k: v for k, v in os.environ.items() if k not in ("W", "H", "S", "D")}      # the reference defaults: 16x16, S=1, depth 5
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd="/", timeout=600)   # run.sh cds to its own directory (run.sh:2-5)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("compile op on gpu succeed", "execute op on gpu succeed", "Generate Result Image"):    # run.sh:115,124,130
        assert line in r.stdout, r.stdout
    rays = np.fromfile(os.path.join(ROOT, "input/rays.bin"), dtype=np.float32)
    sph = np.fromfile(os.path.join(ROOT, "input/spheres.bin"), dtype=np.float32)
    col = np.fromfile(os.path.join(ROOT, "output/color.bin"), dtype=np.float32)
    with open(os.path.join(ROOT, "output/color.ppm"), "rb") as f:
        ppm = f.read()
    return rays, sph, col, ppm


def test_run_sh_gpu_end_to_end_kernel_mode(apt, golden, oracle, tmp_path):
    """SURVEY 8(f)-4 / VERDICT r4 item 1: the reference's whole driver path on the GPU.  input/*.bin are the reference's own bytes,
    output/color.bin equals the CPU restatement in the kernel's arithmetic (K-mode, the default as in src/render.cpp) bit for bit,
    output/color.ppm is that buffer decoded as data_visualization.py:20-59 decodes it."""
    data, _ = golden
    rays, sph, col, ppm = _run_sh()
    assert np.array_equal(bits(rays), bits(data["16x16_s1_rays"])) and np.array_equal(bits(sph), bits(data["spheres"]))
    want, _ = oracle.render_paths(oracle.make_params(16, 16, 1, depth=5, mode=oracle.MODE_K), data["16x16_s1_rays"], data["spheres"])
    assert np.array_equal(bits(col), bits(want).ravel())
    _, _, u8 = oracle.decode_color(want.ravel(), 16, 16, 1)
    oracle.write_ppm(str(tmp_path / "want.ppm"), 16, 16, u8)
    assert ppm == (tmp_path / "want.ppm").read_bytes()


def test_run_sh_gpu_end_to_end_oracle_mode_equals_the_reference_files(apt, golden):
    """The same driver with `-- --mode o` (the NumPy oracle's arithmetic): color.bin IS the reference's test_soa.bin
    (gen_data.py:246-429, golden 16x16_s1_d5_soa) and color.ppm IS the reference's color.ppm for it, byte for byte."""
    data, _ = golden
    rays, sph, col, ppm = _run_sh(["--mode", "o"])
    assert np.array_equal(bits(rays), bits(data["16x16_s1_rays"])) and np.array_equal(bits(sph), bits(data["spheres"]))
    assert np.array_equal(bits(col), bits(data["16x16_s1_d5_soa"]))
    assert np.array_equal(bits(data["decode_soa16_color"]), bits(data["16x16_s1_d5_soa"]))   # the decode fixture was made from this buffer
    assert ppm == data["decode_soa16_ppm"].tobytes()


def _nccl_pipeline_worker(rank, world, port, out_path, frames):
    """One process per GPU (bench.py's shape): `frames` frames of DIFFERENT content through the double-buffered asynchronous gather."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # the repository root (a spawned child: no conftest here)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")   # (its own environment)
    import torch.distributed as dist
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import dist as apt_dist, gen_data, render
    sph = torch.from_numpy(gen_data.gen_spheres()).cuda()
    shard = apt_dist.FrameShard(pkg.make_params(96, 64, 64, depth=8), rank, world, slots=2, stripes=2)
    slots = shard.alloc_slots()
    got = []
    for k in range(frames):
        pk = pkg.make_params(96, 64, 64, depth=8, seed=100 + k)
        shard.render(slots[k % 2], sph, render.render_frame, params=pk, slot=k % 2)
        full = shard.alloc_full() if rank == 0 else (None, None)
        shard.gather_async(k % 2, *full)
        got.append(full)
    shard.finish()
    shard.drain()
    torch.cuda.synchronize()
    if rank == 0:
        np.savez(out_path, **{f"fb{k}": f[0].cpu().numpy() for k, f in enumerate(got)}, **{f"u8{k}": f[1].cpu().numpy() for k, f in enumerate(got)})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs (the driver's multi-GPU node)")
def test_two_ranks_over_rccl_pipelined_gather_of_different_frames(apt, oracle, tmp_path):
    """the root's packed buffer is the collective's send buffer; frame k must not be rendered into it while the gather of
    frame k - 2 still reads it.  Two ranks on two GPUs, six frames of different content, every gathered frame against the oracle."""
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    out = str(tmp_path / "frames.npz")
    mp.spawn(_nccl_pipeline_worker, args=(2, port, out, 6), nprocs=2, join=True)
    z = np.load(out)
    sph = oracle.gen_spheres()
    for k in range(6):
        fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(96, 64, 64, depth=8, seed=100 + k), sph, threads=oracle.max_threads())
        assert np.array_equal(bits(z[f"fb{k}"]), bits(fb_w)) and np.array_equal(z[f"u8{k}"], u8_w), k


@pytest.mark.parametrize("ns", [9, 60])
def test_device_grid_build_answers_a_size_query_a_small_capacity_and_a_build(apt, ns):
    """apt_build_grid_device's three answers on the two smallest generated scenes (without and with a populated cell grid): a size query
    returns the byte count and writes nothing; a capacity four bytes short is refused with that count in *out_bytes and the buffer
    untouched; the exact capacity gives apt_build_grid_host's bytes."""
    L = apt._lib.lib()
    scene = apt.gen_data.gen_scene(ns, seed=1)
    host = apt.gen_data.build_grid(scene, ns)
    d_scene = dev(scene)
    st = apt.render._stream_handle(None)
    nbytes = ctypes.c_size_t(0)
    assert L.apt_build_grid_device(d_scene.data_ptr(), ns, st, None, 0, ctypes.byref(nbytes)) == 0
    B = nbytes.value
    assert B == host.nbytes
    buf = torch.full((B,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nbytes.value = 0
    assert L.apt_build_grid_device(d_scene.data_ptr(), ns, st, buf.data_ptr(), B - 4, ctypes.byref(nbytes)) == 1    # APT_ERR_ARG
    assert b"capacity too small" in L.apt_last_error() and nbytes.value == B
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())
    nbytes.value = 0
    assert L.apt_build_grid_device(d_scene.data_ptr(), ns, st, buf.data_ptr(), B, ctypes.byref(nbytes)) == 0 and nbytes.value == B
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), host)


def test_multi_gpu_object_is_created_rendered_and_closed_repeatedly(apt, oracle):
    """apt_multi through create -> render -> close three times on device 0 ([0, 0], 2 stripes), with a refused create ([0, 99]) between
    the cycles: every frame is the single-launch frame bit for bit, the refusal is reported as apt_multi_create's, and no call moves
    the current device."""
    sph_host = oracle.gen_spheres()
    p = apt.make_params(37, 23, 16, depth=6, seed=11)
    ref, ref8 = apt.render.render_frame(p, dev(sph_host))
    cur = torch.cuda.current_device()
    for cycle in range(3):
        mg = apt.render.MultiGpu(p, sph_host, [0, 0], stripes=2)
        assert torch.cuda.current_device() == cur
        fb, u8 = mg.render()
        assert torch.cuda.current_device() == cur
        assert torch.equal(fb.view(torch.int32), ref.view(torch.int32)) and torch.equal(u8, ref8)
        mg.close()
        assert torch.cuda.current_device() == cur
        if cycle < 2:
            with pytest.raises(apt.AptError):
                apt.render.MultiGpu(p, sph_host, [0, 99])
            assert apt._lib.lib().apt_last_error().startswith(b"apt_multi_create:")
            assert torch.cuda.current_device() == cur
