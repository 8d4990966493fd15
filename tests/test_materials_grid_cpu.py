"""CPU-only: what the material renderer's grid form (include/render_mi355x.h "per-sphere materials": accel with APT_FLAG_GRID_SLOTS)
needs checked without a GPU -- the argument rule, the scene's material-code helper, and that the frames tests/test_gpu_materials_grid.py
renders exercise the grid (hits on binned spheres of every code, skip spheres among them) rather than the walls alone."""
import ctypes

import numpy as np
import pytest

import materials_ref as mr

U = np.uint64


@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import gen_data
    pkg.gen_data = gen_data
    return pkg


def test_grid_argument_validation_needs_no_gpu(apt):
    L = apt._lib.lib()
    one = ctypes.c_void_p(16)      # never dereferenced: validation fails first, and an empty range launches nothing
    u64 = ctypes.c_uint64
    frame = lambda q, mat=one, b=0, c=10, fb=one: L.apt_render_frame_materials(q, None, one, mat, u64(b), u64(c), fb, None)
    paths = lambda q, mat=one: L.apt_render_paths_materials(q, None, one, one, mat, one)
    kw = dict(num_spheres=9, accel=4096, flags=apt.APT_FLAG_GRID_SLOTS)
    g = apt.make_params(16, 16, 1, **kw)
    assert frame(ctypes.byref(g), c=0) == 0                                                   # a vouched grid passes the checks:
    assert paths(ctypes.byref(apt.make_params(16, 16, 1, path_begin=1024, **kw))) == 0        # empty ranges are no-ops
    assert frame(ctypes.byref(g), mat=None) == 1 and b"materials" in L.apt_last_error()
    assert paths(ctypes.byref(g), mat=None) == 1
    o = apt.make_params(16, 16, 1, mode=apt.APT_MODE_ORACLE, **kw)
    assert frame(ctypes.byref(o)) == 1 and b"APT_MODE_KERNEL" in L.apt_last_error()
    assert paths(ctypes.byref(o)) == 1
    assert frame(ctypes.byref(g), fb=None) == 1
    assert frame(ctypes.byref(g), b=0, c=10 ** 9) == 1                                        # pixel range beyond the image
    for flags in (0, apt.APT_FLAG_RR | apt.APT_FLAG_RETIRE):                                  # without the caller's word: refused, as before
        n = apt.make_params(16, 16, 1, num_spheres=9, accel=4096, flags=flags)
        assert frame(ctypes.byref(n), c=0) == 1 and b"accel" in L.apt_last_error()
        assert paths(ctypes.byref(n)) == 1 and b"accel" in L.apt_last_error()
    n8 = apt.make_params(16, 16, 1, num_spheres=8, accel=4096)                               # also for the 8-sphere scene, which ignores a vouched grid
    assert frame(ctypes.byref(n8), c=0) == 1 and frame(ctypes.byref(n8.copy(flags=apt.APT_FLAG_GRID_SLOTS)), c=0) == 0
    ctx = L.apt_context_create()
    try:
        assert L.apt_context_render_frame_materials(ctypes.c_void_p(ctx), ctypes.byref(g), None, one, one, u64(0), u64(0), one, None) == 0
        assert L.apt_context_render_paths_materials(ctypes.c_void_p(ctx), ctypes.byref(g.copy(flags=0)), None, one, one, one, one) == 1
    finally:
        L.apt_context_destroy(ctypes.c_void_p(ctx))


def _codes(ns, seed):
    """apt_gen_scene_materials_host restated: walls and light DIFF, sphere i (splitmix64(seed + i) >> 32) % 3."""
    i = np.arange(ns, dtype=U)
    with np.errstate(over="ignore"):
        c = ((mr.splitmix64(U(seed) + i) >> U(32)) % U(3)).astype(np.int32)
    c[:6] = mr.DIFF
    c[ns - 1] = mr.DIFF
    return c


@pytest.mark.parametrize("ns", [8, 9, 2000])
def test_scene_materials_helper(apt, ns):
    for seed in (0, 5, 2 ** 64 - 3):                       # the last: seed + i wraps around
        sph, mat = apt.gen_data.gen_scene_materials(ns, seed=seed)
        assert mat.dtype == np.int32 and mat.shape == (ns,)
        assert np.array_equal(mat, _codes(ns, seed))
        assert np.array_equal(sph, apt.gen_data.gen_scene(ns, seed=seed))
    if ns == 2000:
        counts = np.bincount(apt.gen_data.gen_scene_materials(ns, seed=5)[1][6:ns - 1], minlength=3)
        assert counts.sum() == ns - 7 and (counts > (ns - 7) / 4).all()


def test_scene_materials_helper_refusals(apt):
    L = apt._lib.lib()
    buf = (ctypes.c_uint32 * 16)()
    assert L.apt_gen_scene_materials_host(ctypes.c_uint32(9), ctypes.c_uint64(0), None) == 1
    assert L.apt_gen_scene_materials_host(ctypes.c_uint32(7), ctypes.c_uint64(0), buf) != 0 and b"num_spheres" in L.apt_last_error()
    assert L.apt_gen_scene_materials_host(ctypes.c_uint32(0), ctypes.c_uint64(0), buf) != 0
    assert L.apt_gen_scene_materials_host(ctypes.c_uint32(8), ctypes.c_uint64(0), buf) == 0
    with pytest.raises(apt.AptError):
        apt.gen_data.gen_scene_materials(7)


# The two frames the GPU tests compare against the restatement: (Ns, width, height, samples); scene and codes of seed 5, render seed 3, depth 6.
COVERAGE_FRAMES = [(2000, 24, 16, 2), (10000, 16, 12, 1)]


@pytest.mark.parametrize("ns,w,h,s_", COVERAGE_FRAMES)
def test_gpu_frames_exercise_the_grid(apt, monkeypatch, ns, w, h, s_):
    """Of all segments of the frame: >= 25 % hit a binned sphere (index 6..Ns-2), each material code has >= 5 % through binned spheres,
    >= 10 % start with a binned skip sphere, none misses (so every path is alive at every depth and each row of _intersect is a segment)."""
    from oracle import oracle
    sph, mat = apt.gen_data.gen_scene_materials(ns, seed=5)
    seen = []
    inner = mr._intersect

    def recording(o, d, geo, eps, skip):
        tmin, idx = inner(o, d, geo, eps, skip)
        seen.append((idx.copy(), np.array(skip, copy=True)))
        return tmin, idx

    monkeypatch.setattr(mr, "_intersect", recording)
    p = oracle.make_params(w, h, s_, depth=6, num_spheres=ns, light_index=ns - 1, seed=3)
    _, _, bad, _ = mr.render_frame(p, sph, mat)
    assert not bad.any()
    idx = np.concatenate([a for a, _ in seen])
    skip = np.concatenate([b for _, b in seen])
    assert idx.size == w * h * 4 * s_ * 6
    binned = (idx >= 6) & (idx <= ns - 2)
    share = [float((binned & (mat[np.maximum(idx, 0)] == c)).mean()) for c in (mr.SPEC, mr.DIFF, mr.REFR)]
    skipped = float(((skip >= 6) & (skip <= ns - 2)).mean())
    print(f"Ns={ns}: binned {binned.mean():.3f}, by code {share}, binned skip {skipped:.3f}, misses {(idx < 0).sum()}")
    assert (idx >= 0).all()
    assert binned.mean() >= 0.25
    assert min(share) >= 0.05
    assert skipped >= 0.10
