"""GPU: frames through the two-paths-per-lane kernel's shortened ray-generate (the tent filter from the generator's bits), packed
colour-times-gain and the once-per-wave-half decode (pt_frame.h frame_decode, shared with the material renderer), against
oracle.render_frame bit for bit -- the framebuffer as uint32, and the 8-bit image -- at the smallest shapes that reach each path:

  7 x 5 = 35 pixels: a partial workgroup of the 8-pixel kind (invalid lanes, the byte-store path); 16 x 8: the packed dword path
  pixels [3, 24) of the 16 x 8 image, with fb_u8 on and off a dword boundary; fb_u8 absent
  S = 8: one sample per lane through the one-ray form; 16: one pair; 20: a pair and the n % 8 tail; 24: a pair and the chain's odd
  member; 64: the headline's four pairs, a power-of-two count; 136: two leaves through the LDS stack, a mean by a non-power of two
  depth 1, 2, 3; K- and O-mode; the reference scene and the one with spheres 0 and 6 exchanged; a gain that clips at 1 and gain 0
  a material-renderer frame at 7 x 5, S = 16, against tests/materials_ref.py"""
import ctypes

import numpy as np
import pytest

import materials_ref as mr

pytestmark = pytest.mark.gpu

K, O = 0, 1
SAMPLES = (8, 16, 20, 24, 64, 136)
DEPTHS = (1, 2, 3)
SHAPES = ((7, 5), (16, 8))


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
    if name == "general":       # spheres 0 and 6 exchanged: the scene does not share planes, the general intersections run
        tab = t[:80].reshape(10, 8)
        tab[:, [0, 6]] = tab[:, [6, 0]]
    return t


def _frame_gpu(apt, p, scene, pixel_begin=0, pixel_count=None, u8="aligned"):
    """render_frame through the C entry, so that fb_u8 can be absent or off a dword boundary.  -> (fb, u8 or None)"""
    import torch
    L = apt._lib.lib()
    pc = p.width * p.height - pixel_begin if pixel_count is None else pixel_count
    d_scene = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.float32)).cuda()
    fb = torch.full((3, pc), float("nan"), dtype=torch.float32, device="cuda")
    raw = torch.full((pc * 3 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    off = {"aligned": 0, "misaligned": 1, "null": 0}[u8]
    u8_ptr = None if u8 == "null" else ctypes.c_void_p(raw.data_ptr() + off)
    rc = L.render_frame(ctypes.byref(p), None, ctypes.c_void_p(d_scene.data_ptr()), ctypes.c_uint64(pixel_begin), ctypes.c_uint64(pc),
                        ctypes.c_void_p(fb.data_ptr()), u8_ptr)
    apt._lib.check(rc, "render_frame")
    torch.cuda.synchronize()
    raw = raw.cpu().numpy()
    if u8 == "null":
        assert (raw == 0xA5).all()
        return fb.cpu().numpy(), None
    assert (raw[:off] == 0xA5).all() and (raw[off + 3 * pc:] == 0xA5).all()          # nothing written around the image
    return fb.cpu().numpy(), raw[off:off + 3 * pc].reshape(pc, 3)


def _check(apt, oracle, scene, w, h, s, depth, mode, gain=12.0, pixel_begin=0, pixel_count=None, u8="aligned"):
    kw = dict(depth=depth, mode=mode, seed=11, gain=gain)
    fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(w, h, s, **kw), scene, pixel_begin, pixel_count, threads=oracle.max_threads())
    fb, got8 = _frame_gpu(apt, apt.make_params(w, h, s, **kw), scene, pixel_begin, pixel_count, u8)
    what = (w, h, s, depth, mode, gain, pixel_begin, pixel_count, u8)
    assert np.array_equal(fb.view(np.uint32), fb_w.view(np.uint32)), (what, np.argwhere(fb.view(np.uint32) != fb_w.view(np.uint32))[:5])
    if got8 is not None:
        assert np.array_equal(got8, u8_w), (what, np.argwhere(got8 != u8_w)[:5])
    return fb_w, u8_w


@pytest.mark.parametrize("mode", (K, O), ids=("K", "O"))
@pytest.mark.parametrize("scene", ("ref", "general"))
@pytest.mark.parametrize("depth", DEPTHS)
def test_frames_at_every_sample_count_and_shape(apt, oracle, depth, scene, mode):
    table = _scene(oracle, scene)
    for w, h in SHAPES:
        for s in SAMPLES:
            _check(apt, oracle, table, w, h, s, depth, mode)


@pytest.mark.parametrize("u8", ("aligned", "misaligned", "null"))
def test_pixel_range_and_the_forms_of_fb_u8(apt, oracle, u8):
    """Pixels [3, 24) of the 16 x 8 image: two whole workgroups and a partial one.  On a dword boundary the whole ones pack their bytes;
    off it none does; without fb_u8 nothing is written but the framebuffer."""
    table = _scene(oracle, "ref")
    for s in SAMPLES:
        for mode in (K, O):
            _check(apt, oracle, table, 16, 8, s, 2, mode, pixel_begin=3, pixel_count=21, u8=u8)
    _check(apt, oracle, table, 7, 5, 64, 3, K, u8=u8)


@pytest.mark.parametrize("gain,expect", ((1.0e6, "clipped"), (0.0, "black")))
def test_gain_that_clips_and_gain_zero(apt, oracle, gain, expect):
    table = _scene(oracle, "ref")
    for w, h in SHAPES:
        for s in (16, 24, 64, 136):
            fb_w, u8_w = _check(apt, oracle, table, w, h, s, 2, K, gain=gain)
            if expect == "clipped":
                assert (fb_w == 1.0).any() and (u8_w == 255).any()           # the case is what it says
            else:
                assert not fb_w.any() and not u8_w.any()


def test_material_frame_through_the_shared_decode(apt):
    """render_frame_mat_kernel<.., 8> at 7 x 5, S = 16: a partial workgroup through the same frame_decode."""
    import torch
    from oracle import oracle
    L = apt._lib.lib()
    sph, mat = apt.gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    p = apt.make_params(7, 5, 16, depth=3, num_spheres=8, light_index=7, seed=5)
    for u8 in ("aligned", "misaligned"):
        d_sph = torch.from_numpy(np.ascontiguousarray(sph, dtype=np.float32)).cuda()
        d_mat = torch.from_numpy(mat).cuda()
        fb = torch.full((3, 35), float("nan"), dtype=torch.float32, device="cuda")
        raw = torch.zeros(35 * 3 + 8, dtype=torch.uint8, device="cuda")
        off = 1 if u8 == "misaligned" else 0
        rc = L.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(d_sph.data_ptr()), ctypes.c_void_p(d_mat.data_ptr()),
                                          ctypes.c_uint64(0), ctypes.c_uint64(35), ctypes.c_void_p(fb.data_ptr()),
                                          ctypes.c_void_p(raw.data_ptr() + off))
        apt._lib.check(rc, "apt_render_frame_materials")
        torch.cuda.synchronize()
        fb_w, u8_w, bad, _ = mr.render_frame(oracle.Params.from_buffer_copy(bytes(p)), sph, mat)
        assert not bad.any()
        assert np.array_equal(fb.cpu().numpy().view(np.uint32), fb_w.view(np.uint32))
        assert np.array_equal(raw[off:off + 105].cpu().numpy().reshape(35, 3), u8_w)
