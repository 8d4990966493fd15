"""The material kernels on scenes that break intersection and light-sampling code (tests/degenerate_scenes.py: coincident spheres of
different material, glass inside glass, NaN / inf members and albedos, lights with twins, a 40-sphere cluster, twins across the LDS tile
boundary, and the same inside exactly 8 spheres), held to the restatement bit for bit.  tests/test_degenerate_scenes_cpu.py shows on
the restatement alone that these scenes reach the rules in question and that five wrong renderers would change the image.

Per scene of more than 8 spheres, every combination of grid (none: LDS tiles; host-built; device-built), light mode (plain,
APT_FLAG_NEE, table) and roulette (off; rr_start 2): buffer mode on the scene's 4096 aimed rays at depth 6, and a 24 x 16 frame of 3
samples at depth 5 from a pinhole and from a lens inside the room -- fb and colours bit for bit (a NaN in the same place counts as equal,
whatever its payload), fb_u8, the trace counter against the restatement's segments, a clean status word, and the gridded frame against
the tile frame.  Per 8-sphere scene the same without the grid axis, and the reference camera, an odd pixel range and fb_u8 = NULL.
Then, per scene, a row with an environment and a row of two film passes; the feature planes of `twins`; `twins` through a grid
whose header lacks the pair-slot tables (mat_hit_grid's vector-load branch); and the device-built grids against the host's bytes."""
import ctypes

import numpy as np
import pytest

import camera_ref as cr
import degenerate_scenes as ds
import features_ref as ft
import film_ref as fr
import materials_ref as mr
from gpu_harness import Scene, apt, assert_bits_equal, inside_lens, inside_pinhole, oracle_params, same, sky_and_sun  # noqa: F401

F, U = np.float32, np.uint64
W, H, S, FRAME_DEPTH, PATH_DEPTH = 24, 16, 3, 5, 6
GRIDS = ("none", "host", "device")
MODES = ("plain", "nee", "table")
RANGE = (5, 101)                                                  # an odd begin, a partial last workgroup

_SCENES, _SHARED = {}, {}


def scene(apt, name, grid="none"):
    """The Scene of `name` behind `grid`; the three of one scene share the restatement's cache (a grid changes no image)."""
    if (name, grid) not in _SCENES:
        if name not in _SHARED:
            _SHARED[name] = (ds.build(apt.gen_data, name), {})
        d, ref = _SHARED[name]
        sc = Scene(apt, d.sph, d.mat, d.ns, d.lights, d.light, grid=grid != "none", builder=grid)
        sc.ref, sc.rays = ref, d.rays
        _SCENES[name, grid] = sc
    return _SCENES[name, grid]


def same_or_nan(got, want):
    """(fb[, u8[, traced]]) twice, as gpu_harness.same holds them; where the expectation holds NaN: the same bits, or a NaN on both sides."""
    if not np.isnan(want[0]).any():
        return same(got, want) if min(len(got), len(want)) > 1 else assert_bits_equal(got[0], want[0])
    g, w = np.ascontiguousarray(got[0], dtype=F), np.ascontiguousarray(want[0], dtype=F)
    assert g.shape == w.shape, (g.shape, w.shape)
    diff = np.argwhere((g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w)))
    assert diff.size == 0, (diff.shape[0], diff[:5], g[tuple(diff[0])], w[tuple(diff[0])])
    assert min(len(got), len(want)) < 2 or np.array_equal(got[1], want[1])
    assert min(len(got), len(want)) < 3 or got[2] == want[2], (got[2], want[2])


def paths_ref(sc, p, mode):
    """materials_ref.trace of the scene's aimed rays for the launch `p` -> colours [3][n], computed once."""
    q = oracle_params(p)
    key = ("paths", bytes(q), mode == "table")
    if key not in sc.ref:
        L, bad, _ = mr.trace_params(q, sc.rays, sc.sph, sc.mat, table=sc.table if mode == "table" else None)
        assert not bad.any()
        sc.ref[key] = L
    return sc.ref[key]


def check_paths(sc, mode, rr, grid):
    n = sc.rays.shape[1]
    p = sc.params(n // 4, 1, 1, PATH_DEPTH, mode=mode, rr=rr, grid=grid)
    assert p.width * p.height * 4 * p.samples == n
    got = sc.paths(p, sc.rays, mode)
    want = paths_ref(sc, p, mode)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    same_or_nan((got,), (want,))


def check_frames(apt, sc, mode, rr, grid, tile=None):
    for cam in (inside_pinhole(apt, W, H), inside_lens(apt, W, H)):
        p = sc.params(W, H, S, FRAME_DEPTH, mode=mode, rr=rr, grid=grid)
        got = sc.frame(p, mode, cam=cam, count=True)
        same_or_nan(got, sc.frame_ref(p, mode, cam))
        if tile is not None:                                      # the gridded frame equals the tile frame
            same_or_nan(got, tile.frame(tile.params(W, H, S, FRAME_DEPTH, mode=mode, rr=rr), mode, cam=cam, count=True))


@pytest.mark.gpu
@pytest.mark.parametrize("rr", [False, True], ids=["norr", "rr2"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", ds.MANY)
def test_degenerate_scene_equals_the_restatement(apt, name, grid, mode, rr):
    sc = scene(apt, name, grid)
    check_paths(sc, mode, rr, grid != "none")
    check_frames(apt, sc, mode, rr, grid != "none", tile=scene(apt, name) if grid != "none" else None)


def _frame_without_u8(apt, sc, p, mode, cam):
    """The C entries themselves with fb_u8 = NULL -> (fb, segments traced)."""
    import torch
    n = p.width * p.height
    fb = torch.full((3, n), -9.0, dtype=torch.float32, device="cuda")
    L = apt._lib.lib()
    args = (ctypes.byref(p), None, ctypes.c_void_p(sc.d_sph.data_ptr()), ctypes.c_void_p(sc.d_mat.data_ptr()))
    tail = (ctypes.c_uint64(0), ctypes.c_uint64(n), ctypes.c_void_p(fb.data_ptr()), None)

    def fn():
        rc = (L.apt_render_frame_lights(*args, ctypes.c_void_p(sc.d_table.data_ptr()), *tail) if mode == "table"
              else L.apt_render_frame_materials(*args, *tail))
        assert rc == 0, L.apt_last_error()
    _, traced = sc._launch(cam, None, True, True, fn)
    return fb.cpu().numpy(), traced


@pytest.mark.gpu
@pytest.mark.parametrize("rr", [False, True], ids=["norr", "rr2"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ds.EIGHT)
def test_degenerate_8_sphere_scene_equals_the_restatement(apt, name, mode, rr):
    sc = scene(apt, name)
    check_paths(sc, mode, rr, False)
    check_frames(apt, sc, mode, rr, False)
    p = sc.params(W, H, S, FRAME_DEPTH, mode=mode, rr=rr)
    want = sc.frame_ref(p, mode)                                   # the reference camera
    same_or_nan(sc.frame(p, mode, count=True), want)
    b, c = RANGE
    same_or_nan(sc.frame(p, mode, pixel_begin=b, pixel_count=c), (want[0][:, b:b + c], want[1][b:b + c]))
    cam = inside_pinhole(apt, W, H)
    fb, traced = _frame_without_u8(apt, sc, p, mode, cam)
    want = sc.frame_ref(p, mode, cam)
    same_or_nan((fb, want[1], traced), want)


@pytest.mark.gpu
@pytest.mark.parametrize("i,name", list(enumerate(ds.NAMES)), ids=ds.NAMES)
def test_degenerate_scene_under_a_sky_with_a_sampled_sun(apt, i, name):
    """A closed room hides the sky and the sun: the image stays the room's, and what the environment adds is the sun's shadow segment
    after every DIFF bounce, through the same hit routines, each one counted."""
    sc = scene(apt, name, "host" if name in ds.MANY else "none")
    mode, rr, grid = MODES[i % 3], i % 2 == 1, name in ds.MANY
    env, cam = sky_and_sun(apt), inside_pinhole(apt, W, H)
    p = sc.params(W, H, S, FRAME_DEPTH, mode=mode, rr=rr, grid=grid)
    same_or_nan(sc.frame(p, mode, cam=cam, env=env, count=True), sc.frame_ref(p, mode, cam, env))


@pytest.mark.gpu
@pytest.mark.parametrize("i,name", list(enumerate(ds.NAMES)), ids=ds.NAMES)
def test_degenerate_scene_as_two_film_passes(apt, i, name):
    sc = scene(apt, name, "device" if name in ds.MANY else "none")
    mode, rr, grid = MODES[(i + 1) % 3], i % 2 == 0, name in ds.MANY
    cam = inside_lens(apt, W, H)
    p = sc.params(W, H, S, FRAME_DEPTH, mode=mode, rr=rr, grid=grid)
    snaps, traced = sc.film_passes(p, mode, None, cam, 2, checkpoints=(1, 2))
    rec = cr.from_ctypes(cam)
    planes, segs = zip(*[fr.render_pass(oracle_params(p), sc.sph, sc.mat, table=sc.table if mode == "table" else None, pass_index=k,
                                        rays=lambda seed: cr.rays(rec, W, H, S, seed=seed)) for k in (0, 1)])
    same_or_nan((snaps[1],), (planes[0],))
    same_or_nan((snaps[2],), (fr.accumulate(planes),))
    assert traced == list(segs), (traced, segs)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", GRIDS)
def test_feature_planes_are_the_lowest_twins(apt, grid):
    """A camera that looks at the ten coincident spheres of `twins`: the albedo under those pixels is sphere 10's, the lowest index."""
    sc = scene(apt, "twins", grid)
    tab = sc.sph[:10 * sc.ns].reshape(10, sc.ns)
    cam = apt.gen_data.camera(width=W, height=H, eye=(30.0, 30.0, 100.0), target=tuple(float(x) for x in tab[1:4, 10]), up=(0.0, 1.0, 0.0),
                              vfov_deg=30.0, offset=0.0)
    p = sc.params(W, H, S, FRAME_DEPTH, grid=grid != "none")
    want = ft.planes(cr.from_ctypes(cam), W, H, S, p.seed, sc.sph, sc.ns, p.eps)
    alb = want[ft.ALBEDO:ft.ALBEDO + 3]
    assert int((alb == tab[7:10, 10][:, None]).all(axis=0).sum()) >= 8
    assert not any((alb == tab[7:10, k][:, None]).all(axis=0).any() for k in range(11, 20))
    assert_bits_equal(sc.features(p, cam), want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_grid_without_pair_slots_renders_the_same_image(apt, mode):
    """A device copy of the grid of `twins` with header word 26 (off_cellslot) cleared: the header refuses a grid for a wrong magic or
    sphere count alone, so the launch reads the always-tested list by vector loads and renders the image of the tile form."""
    sc = scene(apt, "twins", "host")
    assert sc.hgrid[26] != 0
    bare = sc.grid.clone()
    bare[26] = 0
    cam = inside_pinhole(apt, W, H)
    p = sc.params(W, H, S, FRAME_DEPTH, mode=mode, rr=True, grid=True)
    with_slots = sc.frame(p, mode, cam=cam, count=True)
    p.accel = bare.data_ptr()
    got = sc.frame(p, mode, cam=cam, count=True)
    same_or_nan(got, sc.frame_ref(p, mode, cam))
    same_or_nan(got, with_slots)
    n = sc.rays.shape[1]
    q = sc.params(n // 4, 1, 1, PATH_DEPTH, mode=mode, rr=True, grid=True)
    q.accel = bare.data_ptr()
    same_or_nan((sc.paths(q, sc.rays, mode),), (paths_ref(sc, q, mode),))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ds.MANY)
def test_device_built_grid_has_the_host_builds_bytes(apt, name):
    """cluster40 has a cell list above kGridSortInline, which the device builder hands to the host sort; `values` has members that are not finite."""
    host, device = scene(apt, name, "host"), scene(apt, name, "device")
    assert host.hgrid.dtype == device.hgrid.dtype == np.uint32 and np.array_equal(host.hgrid, device.hgrid)
    if name == "cluster40":
        cells = host.hgrid[host.hgrid[9]:host.hgrid[9] + host.hgrid[5] + 1]      # GridHeader: off_cells, ncells
        assert int(np.diff(cells.astype(np.int64)).max()) > 32
