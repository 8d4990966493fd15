"""GPU: every kernel that walks a pairwise-sum plan (ascendpathtracing_amd/csrc/pt_leaf.h), at the deep end of what the contract admits.

The other GPU tests stop at 136 samples for most frame kernels (2 leaves, stack depth 2), 1000 for the fused MT19937 frame and 300 for
the decode.  Here: plan_ref.DEEP = 257, 521, 1025, 4096, 4199 and 7688 samples -- stack depths 3 to 7 of the kernels' 8 entries, leaves of
128 samples next to leaves with an n % 8 tail, a power of two (the decode's exact reciprocal), 44 leaves (the most a frame with a camera
takes: its words ride behind them) and 64 leaves (the contract's limit).  Frames are 4 x 3 pixels -- in the kernels with one lane group
per sub-pixel a whole 8-pixel workgroup and a partial one -- and pixels [3, 10) of them; the float framebuffer is compared as uint32
and the 8-bit image exactly, against the CPU oracle (mirror renderer) or the NumPy restatements (material renderer).

Scenes, depths, gains and seeds are tests/plan_ref.py's: tests/test_deep_plans_cpu.py holds each to the condition that a wrong
summation order over the same samples changes the frame, so these rows see the order in which a kernel summed."""
import ctypes
import functools

import numpy as np
import pytest

import plan_ref as pr
from gpu_harness import apt, dev  # noqa: F401

pytestmark = pytest.mark.gpu

K, O, RETIRE, RR = pr.K, pr.O, pr.RETIRE, pr.RR
NPIX = pr.W * pr.H
RANGES = (None, pr.SUB)


def _assert_same(got, want, what):
    fb, u8 = np.asarray(got[0], dtype=np.float32), np.asarray(got[1])
    fb_w, u8_w = np.ascontiguousarray(want[0], dtype=np.float32), np.asarray(want[1])
    diff = np.argwhere(fb.view(np.uint32) != fb_w.view(np.uint32))
    assert diff.size == 0, (what, diff.shape, diff[:5], fb[tuple(diff[0])], fb_w[tuple(diff[0])])
    assert np.array_equal(u8, u8_w), what


def _cut(frame, rng):
    """(fb [3][npix], u8 [npix][3]) of the whole frame -> of the pixel range (decode_color does not depend on where a pixel lies)."""
    if rng is None:
        return frame
    b, c = rng
    return frame[0][:, b:b + c], frame[1][b:b + c]


# ---- mirror renderer ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mirror_want(scene, mode, flags, s):
    """The oracle's whole frame and traced-segment count of a plan_ref mirror case, computed once."""
    from oracle import oracle
    assert (scene, mode, flags, s) in _CASES
    sph, _ = pr.mirror_scene(oracle, scene)
    fb, u8, _, traced = oracle.render_frame(pr.mirror_params(oracle, scene, mode, flags, s), sph, threads=oracle.max_threads())
    return (fb, u8), int(traced)


_CASES = set(pr.mirror_cases())
_DEV = {}


def _mirror_dev(apt, scene):
    """-> (device table, device grid or None)"""
    if scene not in _DEV:
        import torch
        from oracle import oracle
        sph, ns = pr.mirror_scene(oracle, scene)
        grid = None
        if scene == "grid":
            grid = torch.from_numpy(apt.gen_data.build_grid(sph, ns).view(np.int32)).cuda()
            assert int(grid[26]) != 0           # off_cellslot: the grid carries the pair-slot tables of the sample-queue kernel's grid form
        _DEV[scene] = (dev(sph), grid)
    return _DEV[scene]


def _mirror_frame(apt, scene, mode, flags, s, rng=None, counter=False, knob=None):
    """One render_frame launch of a plan_ref mirror case into poisoned buffers, its status word checked -> ((fb, u8), traced or None)."""
    import torch
    c = pr.MIRROR[scene]
    d_sph, grid = _mirror_dev(apt, scene)
    p = apt.make_params(pr.W, pr.H, s, depth=c["depth"], num_spheres=c["ns"], gain=c["gain"], mode=mode, flags=flags, seed=c["seed"],
                        rr_start=c["rr_start"], accel=grid.data_ptr() if grid is not None else 0)
    pb, pc = rng or (0, NPIX)
    fb = torch.full((3, pc), float("nan"), dtype=torch.float32, device="cuda")
    u8 = torch.full((pc, 3), 77, dtype=torch.uint8, device="cuda")

    def go():
        if not counter:
            apt.render.render_frame(p, d_sph, pixel_begin=pb, pixel_count=pc, fb=fb, fb_u8=u8)
            return None
        with apt.render.TraceCounter() as tc:
            apt.render.render_frame(p, d_sph, pixel_begin=pb, pixel_count=pc, fb=fb, fb_u8=u8)
        return tc.value

    if knob:
        with apt.render.debug_knob(*knob):
            traced = go()
    else:
        traced = go()
    torch.cuda.synchronize()
    apt.render.check_device_status()
    return (fb.cpu().numpy(), u8.cpu().numpy()), traced


@pytest.mark.parametrize("s", pr.DEEP)
@pytest.mark.parametrize("mode", [K, O], ids=["K", "O"])
@pytest.mark.parametrize("rr", [False, True], ids=["two-path", "one-path-rr"])
def test_frame_kernel_8_spheres(apt, rr, mode, s):
    """render_frame_kernel<m, kScene8, 8, false, TWO>: the headline's two-paths-per-lane form (no flags) and the one-path form
    (APT_FLAG_RR): the leaf loop and the LDS stack."""
    flags = RR if rr else 0
    want, _ = _mirror_want("ref", mode, flags, s)
    for rng in RANGES:
        got, _ = _mirror_frame(apt, "ref", mode, flags, s, rng)
        _assert_same(got, _cut(want, rng), (rr, mode, s, rng))


@pytest.mark.parametrize("s", pr.DEEP)
@pytest.mark.parametrize("mode", [K, O], ids=["K", "O"])
@pytest.mark.parametrize("rr", [False, True], ids=["retire", "retire-rr"])
def test_sample_queue_kernel_8_spheres(apt, rr, mode, s):
    """render_frame_queue8_kernel<m, rr>: unit cursors over up to 64 leaves, colour buffers sized by maxleaf = 128, the
    [kMaxStack][3][4] stack.  Where the count has no n % 8 tail the traced-segment counter is the oracle's too."""
    flags = RETIRE | (RR if rr else 0)
    want, traced_w = _mirror_want("ref", mode, flags, s)
    for rng in RANGES:
        got, traced = _mirror_frame(apt, "ref", mode, flags, s, rng, counter=rng is None and s % 8 == 0)
        _assert_same(got, _cut(want, rng), (rr, mode, s, rng))
        if rng is None and s % 8 == 0:
            assert traced == traced_w > 0, (rr, mode, s, traced, traced_w)


_TILE_ROWS = [(rt, m, s) for s in pr.TILE_SAMPLES for m in pr.mode_of("tiles", s) for rt in (False, True)]


@pytest.mark.parametrize("retire,mode,s", _TILE_ROWS, ids=["%s-%s-s%d" % ("retire" if r[0] else "full", "KO"[r[1]], r[2]) for r in _TILE_ROWS])
def test_lds_tile_form(apt, retire, mode, s):
    """render_frame_kernel<m, kSceneTiles, 8, RETIRE>: a 40-sphere scene traversed by brute force over LDS tiles.

    With APT_FLAG_RETIRE the launch asks for the 3072-byte stack and the per-wave colour queue [4][3][8 * maxleaf] floats of dynamic
    LDS: from 256 samples on (maxleaf = 128) that is 3072 + 49 152 = 52 224 bytes, on top of the 16 776 bytes of static LDS the
    kernel's descriptor carries (.amdhsa_group_segment_fixed_size of both modes' instantiations in this build): 69 000 bytes, the
    library's only launch above 64 KiB.  A workgroup of an MI355X may hold 160 KiB, and the runtime takes the launch as issued: the
    frame is rendered (the buffers are poisoned beforehand: an accepted launch that wrote nothing would show), bit for bit the
    oracle's, and no error is returned."""
    flags = RETIRE if retire else 0
    assert pr.stats(s)["maxleaf"] == 128
    want, _ = _mirror_want("tiles", mode, flags, s)
    for rng in RANGES:
        got, _ = _mirror_frame(apt, "tiles", mode, flags, s, rng)
        _assert_same(got, _cut(want, rng), (retire, mode, s, rng))


_GRID_ROWS = [(m, s) for s in pr.GRID_SAMPLES for m in pr.mode_of("grid", s)]


@pytest.mark.parametrize("mode,s", _GRID_ROWS, ids=["%s-s%d" % ("KO"[r[0]], r[1]) for r in _GRID_ROWS])
def test_grid_forms(apt, mode, s):
    """A 300-sphere room behind a grid: the sample-queue kernel's grid form (render_frame_queue8_kernel<m, rr, kSceneGrid, stats>)
    plain and with RETIRE | RR, and the nested walk of render_frame_kernel<m, kSceneGrid, 8, rt> behind the grid_walk = 1 knob --
    each the oracle's brute-force frame, the two walks with equal traced-segment counters."""
    for flags in (0, RETIRE | RR):
        want, traced_w = _mirror_want("grid", mode, flags, s)
        queue, traced_q = _mirror_frame(apt, "grid", mode, flags, s, counter=True)
        nested, traced_n = _mirror_frame(apt, "grid", mode, flags, s, counter=True, knob=("grid_walk", 1))
        _assert_same(queue, want, ("queue", mode, s, flags))
        _assert_same(nested, want, ("nested", mode, s, flags))
        assert traced_q == traced_n > 0, (mode, s, flags, traced_q, traced_n, traced_w)
        part, _ = _mirror_frame(apt, "grid", mode, flags, s, pr.SUB)
        _assert_same(part, _cut(want, pr.SUB), ("queue", mode, s, flags, pr.SUB))
        part, _ = _mirror_frame(apt, "grid", mode, flags, s, pr.SUB, knob=("grid_walk", 1))
        _assert_same(part, _cut(want, pr.SUB), ("nested", mode, s, flags, pr.SUB))


# ---- material renderer -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mat_want(name, mode, s, camera=False):
    """The restatement's whole frame of a plan_ref material case: *_ref.trace -> oracle.decode_color (with a camera: camera_ref's rays,
    the call tests/test_gpu_camera.py test_fused_frames_are_the_restatement_bit_for_bit holds its frames to)."""
    from ascendpathtracing_amd import gen_data
    from oracle import oracle
    L = pr.mat_colours(oracle, gen_data, name, mode, s, cam=pr.lens_camera(gen_data) if camera else None)
    _, fb, u8 = oracle.decode_color(L, pr.W, pr.H, s)
    return fb, u8


_MAT_DEV = {}


def _mat_dev(apt, name):
    if name not in _MAT_DEV:
        import torch
        sph, mat, ns, light, table = pr.mat_scene(apt.gen_data, name)
        hgrid = apt.gen_data.build_grid(sph, ns)
        assert apt.gen_data.grid_flags(hgrid, ns) == apt.APT_FLAG_GRID_SLOTS
        _MAT_DEV[name] = dict(sph=dev(sph), mat=dev(mat, np.int32), ns=ns, light=light, table=None if table is None else dev(table.view(np.int32)),
                              grid=torch.from_numpy(hgrid.view(np.int32)).cuda())
    return _MAT_DEV[name]


def _mat_frame(apt, name, mode, s, rng=None, grid=False, cam=None):
    """One material launch through the default context (with `cam` set, or no camera) into poisoned buffers, its status word checked."""
    import torch
    d = _mat_dev(apt, name)
    flags = (apt.APT_FLAG_NEE if mode == "nee" else 0) | (apt.APT_FLAG_GRID_SLOTS if grid else 0)
    p = apt.make_params(pr.W, pr.H, s, depth=pr.MAT_DEPTH, num_spheres=d["ns"], light_index=d["light"], seed=pr.MAT_SEED, flags=flags,
                        accel=d["grid"].data_ptr() if grid else 0)
    pb, pc = rng or (0, NPIX)
    fb = torch.full((3, pc), float("nan"), dtype=torch.float32, device="cuda")
    u8 = torch.full((pc, 3), 77, dtype=torch.uint8, device="cuda")
    apt.render.set_camera(cam)
    try:
        apt.render.render_frame(p, d["sph"], pixel_begin=pb, pixel_count=pc, fb=fb, fb_u8=u8, materials=d["mat"],
                                lights=d["table"] if mode == "table" else None)
        torch.cuda.synchronize()
        apt.render.check_device_status()
    finally:
        apt.render.set_camera(None)
    return fb.cpu().numpy(), u8.cpu().numpy()


@pytest.mark.parametrize("s", pr.MAT_SAMPLES)
@pytest.mark.parametrize("mode", ["plain", "nee"])
def test_material_frame_8_spheres(apt, mode, s):
    """render_frame_mat_kernel's 8-sphere form, plain and with APT_FLAG_NEE, against materials_ref."""
    want = _mat_want("diff8", mode, s)
    for rng in RANGES:
        _assert_same(_mat_frame(apt, "diff8", mode, s, rng), _cut(want, rng), (mode, s, rng))


@pytest.mark.parametrize("s", pr.MAT_SAMPLES)
def test_material_frame_light_table_by_tiles_and_through_the_grid(apt, s):
    """The demo scene with the lamp and a light table, against materials_ref: the tile form and the grid form, the same frame."""
    want = _mat_want("demo9lamp", "table", s)
    for grid in (False, True):
        for rng in RANGES:
            _assert_same(_mat_frame(apt, "demo9lamp", "table", s, rng, grid=grid), _cut(want, rng), (s, grid, rng))


def test_material_frame_with_a_lens_camera_at_the_44_leaf_limit(apt):
    """4199 samples, 44 leaves: the contract's 44-leaf limit with a camera.  A thin-lens camera, the light
    table, by tiles and through the grid."""
    s = pr.CAMERA_SAMPLES
    assert pr.stats(s)["leaves"] == 44 and pr.stats(s + 1)["leaves"] == 45
    cam = pr.lens_camera(apt.gen_data)
    assert cam.aperture > 0
    want = _mat_want("demo9lamp", "table", s, camera=True)
    assert want[0].max() > 0                                   # the camera sees something
    assert not np.array_equal(want[0], _mat_want("demo9lamp", "table", s)[0])
    for grid in (False, True):
        for rng in RANGES:
            _assert_same(_mat_frame(apt, "demo9lamp", "table", s, rng, grid=grid, cam=cam), _cut(want, rng), (grid, rng))


# ---- the fused MT19937 frame -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", pr.MT_SAMPLES)
def test_mt_frame_any_sample_count(apt, oracle, s):
    """render_frame_mt_any_kernel<O>: per-run stacks that carry over from round to round.  10 x 9 pixels are two 78-pixel groups, the
    second partial.  Against MT19937 gen_rays -> O-mode render_paths -> decode_color on the CPU, and up to 1025 samples against the
    device's three-kernel pipeline as well."""
    import torch
    from ascendpathtracing_amd import _lib
    w, h = pr.MT_W, pr.MT_H
    _, fb_w, u8_w = oracle.decode_color(pr.mt_colours(oracle, s), w, h, s)
    d_sph = dev(apt.gen_data.gen_spheres())
    p = apt.make_params(w, h, s, depth=pr.MT_DEPTH, mode=apt.APT_MODE_ORACLE, gain=pr.MT_GAIN)
    for rng in (None, pr.MT_SUB):
        pb, pc = rng or (0, w * h)
        ck, g_lo = apt.render.mt_group_checkpoints(w, h, s, 0, pb, pc)
        ck_d = torch.from_numpy(ck.view(np.int32)).cuda()
        fb = torch.full((3, pc), float("nan"), dtype=torch.float32, device="cuda")
        u8 = torch.full((pc, 3), 77, dtype=torch.uint8, device="cuda")
        _lib.check(_lib.lib().apt_render_frame_mt(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                                  ctypes.c_void_p(ck_d.data_ptr()), ctypes.c_uint64(ck_d.shape[0]), ctypes.c_uint64(g_lo),
                                                  ctypes.c_void_p(d_sph.data_ptr()), ctypes.c_uint64(pb), ctypes.c_uint64(pc),
                                                  ctypes.c_void_p(fb.data_ptr()), ctypes.c_void_p(u8.data_ptr())), "apt_render_frame_mt")
        torch.cuda.synchronize()
        apt.render.check_device_status()
        _assert_same((fb.cpu().numpy(), u8.cpu().numpy()), _cut((fb_w, u8_w), rng), (s, rng))
    if s <= 1025:
        rays = apt.gen_data.gen_rays_device(w, h, s, seed=0)
        colors = apt.render.render_paths(p, rays.reshape(-1), d_sph)
        fb3, u83 = apt.render.decode_color_device(p, colors)
        torch.cuda.synchronize()
        apt.render.check_device_status()
        _assert_same((fb3.cpu().numpy(), u83.cpu().numpy()), (fb_w, u8_w), (s, "three kernels"))


# ---- the decode kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", pr.DEEP)
def test_decode_color_device_and_band(apt, oracle, s):
    """decode_color_kernel8's stack and frame_decode's exact reciprocal (4096 is a power of two), on random colours of mixed magnitude:
    12 pixels through apt_decode_color_device, and a band of 7 pixels that starts at pixel 3 through apt_decode_color_band."""
    import torch
    from ascendpathtracing_amd import _lib
    col = pr.decode_colors(s)
    _, fb_w, u8_w = oracle.decode_color(col, pr.W, pr.H, s)
    assert 0 < (fb_w == 1).sum() < fb_w.size // 3
    p = apt.make_params(pr.W, pr.H, s)
    fb, u8 = apt.render.decode_color_device(p, dev(col))
    torch.cuda.synchronize()
    _assert_same((fb.cpu().numpy(), u8.cpu().numpy()), (fb_w, u8_w), (s, "device"))
    b, c = pr.SUB
    band = dev(col.reshape(3, NPIX * 4 * s)[:, b * 4 * s:(b + c) * 4 * s])
    assert band.is_contiguous() and band.numel() == 3 * c * 4 * s
    fb_b = torch.full((3, c), float("nan"), dtype=torch.float32, device="cuda")
    u8_b = torch.full((c, 3), 77, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().apt_decode_color_band(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                                ctypes.c_void_p(band.data_ptr()), ctypes.c_uint64(c), ctypes.c_void_p(fb_b.data_ptr()),
                                                ctypes.c_void_p(u8_b.data_ptr())), "apt_decode_color_band")
    torch.cuda.synchronize()
    apt.render.check_device_status()
    _assert_same((fb_b.cpu().numpy(), u8_b.cpu().numpy()), _cut((fb_w, u8_w), pr.SUB), (s, "band"))
