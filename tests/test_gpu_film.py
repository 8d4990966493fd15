"""GPU: the film (include/render_mi355x.h "film") through the C-ABI, bit for bit against the NumPy restatement tests/film_ref.py with
the status word clean.

  passes    the film after pass 0, after 2 and after 5 against film_ref.accumulate, and pass 0 clipped against the fb of the frame
            entry on the same launch parameters; the trace counter of a pass against the frame entry's with the pass's seed: the three
            scene forms (the open 8-sphere scene, 40 open spheres by tiles, 220 through the grid with grid film == tile film) x
            {plain, APT_FLAG_NEE, a light table}, over samples 1 / 3 (GROUP 1), 8, 9 (a tail lane) and 16 (the power-of-two mean), depth
            1 / 2 / 5, an environment with the sun sampled / none at all, no camera / a thin lens, with and without roulette; the closed
            demo scene with its lamp in the three light modes; a 16 x 8 frame at the smallest count whose plan has two leaves.
  buffer    pass 0 over a film of NaN; a mid-image pixel range inside a guard-filled allocation; a grid that is not the scene's; the
            entry's own refusals.
  resolve   apt_film_resolve_device against apt_film_resolve_host bit for bit on the CPU test's values and ragged sizes, at every byte
            offset of the 8-bit image, and on a real 5-pass film.
  Film      render.Film end to end: three passes, mean, resolve, reset.

On the parent every test here fails: the entries do not exist."""
import ctypes

import numpy as np
import pytest

import camera_ref as cr
import film_ref as fr
import materials_ref as mr
from gpu_harness import Scene, apt, assert_bits_equal, dev, lens, scene, sky_and_sun  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
W, H = 48, 32
SIZE = {"open220": (24, 16)}            # the restatement tests every path against every sphere: a quarter of the pixels for 220 of them


def _pass_ref(sc, p, mode, env, cam, k):
    """film_ref's pass k of the launch `p` -> (planes, segments); computed once (the grid changes no image: not part of the key)."""
    key = ("pass", p.width, p.height, p.samples, p.depth, p.seed, mode, p.flags & (2 | 32 | 64), p.rr_start, None if cam is None else bytes(cam),
           None if env is None else bytes(env), k)
    if key not in sc.ref:
        from oracle import oracle
        rays = None if cam is None else (lambda seed: cr.rays(cr.from_ctypes(cam), p.width, p.height, p.samples, seed=seed))
        planes, seg = fr.render_pass(oracle.Params.from_buffer_copy(bytes(p)), sc.sph, sc.mat, env=None if env is None else mr.Env.from_ctypes(env),
                                     table=sc.table if mode == "table" else None, pass_index=k, rays=rays)
        planes.setflags(write=False)
        sc.ref[key] = (planes, seg)
    return sc.ref[key]


_demo9 = []


def _scene(apt, name):
    """The catalogue's open8 / open40 / open220; demo9: the closed demo scene with smallpt's lamp and a second emitter."""
    if name != "demo9":
        return scene(apt, name)
    if not _demo9:
        gd = apt.gen_data
        sph, mat = gd.gen_spheres_materials()
        sph = gd.with_lamp(sph, 9, 7)                                        # emission 400: far above 1 wherever it is seen
        sph = gd.with_lamps(sph, 9, [6], radius=[16.5], emission=[(3.0, 2.0, 1.0)])
        mat = np.array(mat, dtype=np.int32)
        mat[6] = mr.DIFF
        _demo9.append(Scene(apt, sph, mat, 9, [7, 6], 7))
    return _demo9[0]


def _check_passes(sc, p, mode, env, cam, checkpoints, grid=False):
    """The film at every checkpoint against the restatement, pass 0 clipped against the frame entry, the trace counter of every pass against
    the restatement's segments and pass 1's against the frame entry's with that pass's seed."""
    upto = max(checkpoints)
    snaps, traced = sc.film_passes(p, mode, env, cam, upto, checkpoints=checkpoints)
    refs = [_pass_ref(sc, p, mode, env, cam, k) for k in range(upto)]
    for k in checkpoints:
        assert_bits_equal(snaps[k], fr.accumulate([r[0] for r in refs[:k]]))
    assert traced == [r[1] for r in refs], (traced, [r[1] for r in refs])
    fb, _, seg = sc.frame(p, mode, cam, env, count=True)
    with np.errstate(invalid="ignore"):
        assert_bits_equal(np.clip(snaps[1], F(0), F(1)) if 1 in snaps else np.clip(refs[0][0], F(0), F(1)), fb)
    assert seg == traced[0]
    if upto > 1:
        q = p.copy(seed=fr.pass_seed(p.seed, 1))
        assert sc.frame(q, mode, cam, env, count=True)[2] == traced[1]
    if grid:                                                                     # the grid form is the tile form
        tiles = sc.params(p.width, p.height, p.samples, p.depth, mode=mode, rr=bool(p.flags & 2), seed=p.seed)
        assert tiles.accel == 0 and p.accel != 0
        other, _ = sc.film_passes(tiles, mode, env, cam, upto, checkpoints=(upto,))
        assert_bits_equal(other[upto], snaps[upto])
    return snaps


FORMS = [("open8", False), ("open40", False), ("open220", True)]
FORM_IDS = ["8", "tiles40", "grid220"]
MODES = ["plain", "nee", "table"]
# (samples, depth, environment, lens, roulette) per light mode: every sample count, depth, both environments, both cameras and roulette
# meet every scene form; the two launches of a mode differ in GROUP
LAUNCHES = {"plain": [(1, 5, True, False, False), (9, 2, False, True, True)],
            "nee": [(3, 2, False, True, False), (16, 5, True, False, True)],
            "table": [(8, 5, True, True, False), (3, 1, False, False, False)]}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,grid", FORMS, ids=FORM_IDS)
def test_film_passes_equal_the_restatement(apt, name, grid, mode):
    sc = _scene(apt, name)
    w, h = SIZE.get(name, (W, H))
    for s_, depth, with_env, with_lens, rr in LAUNCHES[mode]:
        p = sc.params(w, h, s_, depth, mode=mode, rr=rr, seed=50 + s_, grid=grid)
        snaps = _check_passes(sc, p, mode, sky_and_sun(apt) if with_env else None, lens(apt, w, h) if with_lens else None, (1, 2), grid)
        assert snaps[2].max() > (1.0 if with_env else 0.0)                       # with the sky: radiance the frame entries clip


@pytest.mark.parametrize("mode", MODES)
def test_the_closed_demo_scene_with_its_lamp(apt, mode):
    sc = _scene(apt, "demo9")
    s_, depth = {"plain": (8, 5), "nee": (9, 5), "table": (1, 2)}[mode]
    snaps = _check_passes(sc, sc.params(W, H, s_, depth, mode=mode, seed=7), mode, None, None, (1, 2))
    assert snaps[2].max() > 1.0


def test_five_passes(apt):
    sc = _scene(apt, "open8")
    _check_passes(sc, sc.params(W, H, 9, 2, mode="nee", seed=11), "nee", sky_and_sun(apt), None, (1, 2, 5))


def test_a_plan_of_two_leaves(apt):
    """16 x 8 at 129 samples, the smallest count whose pairwise plan has two leaves (64 + 65): the LDS stack, and a tail lane in the second."""
    import plan_ref
    assert len(plan_ref.plan(128)) == 1 and len(plan_ref.plan(129)) == 2
    sc = _scene(apt, "open8")
    _check_passes(sc, sc.params(16, 8, 129, 2, seed=13), "plain", sky_and_sun(apt), None, (1, 2))


def test_pass_zero_stores_over_nan(apt):
    import torch
    sc = _scene(apt, "open8")
    for s_ in (3, 8):
        p = sc.params(W, H, s_, 2, seed=17)
        film = torch.full((3, W * H), float("nan"), dtype=torch.float32, device="cuda")
        snaps, _ = sc.film_passes(p, "plain", sky_and_sun(apt), None, 1, film=film, checkpoints=(1,))
        want = _pass_ref(sc, p, "plain", sky_and_sun(apt), None, 0)[0]
        assert_bits_equal(snaps[1], want)
        assert not np.isnan(want).any() and not np.isnan(snaps[1]).any()


@pytest.mark.parametrize("s_", [3, 9])
def test_a_pixel_range_inside_guards(apt, s_):
    """Pixels [37, 37 + 1001): not a multiple of a workgroup's 64 (GROUP 1) or 8 (GROUP 8) pixels; the film is exactly that long."""
    import torch
    sc = _scene(apt, "open40")
    b, c, guard = 37, 1001, 64
    p = sc.params(W, H, s_, 2, mode="table", seed=19)
    block = torch.full((guard + 3 * c + guard,), -9.0, dtype=torch.float32, device="cuda")
    film = block[guard:guard + 3 * c].view(3, c)
    env = sky_and_sun(apt)

    with sc.view(env=env):
        for k in range(2):
            apt.render.render_frame_film(p, sc.d_sph, sc.d_mat, film=film, pass_index=k, lights=sc.d_table, pixel_begin=b, pixel_count=c)
        torch.cuda.synchronize()
    apt.render.check_device_status()
    host = block.cpu().numpy()
    assert (host[:guard] == -9.0).all() and (host[guard + 3 * c:] == -9.0).all()
    want = fr.accumulate([_pass_ref(sc, p, "table", env, None, k)[0][:, b:b + c] for k in range(2)])
    assert_bits_equal(host[guard:guard + 3 * c].reshape(3, c), want)


def test_a_grid_that_is_not_the_scenes_leaves_the_film_untouched(apt):
    import torch
    sc = _scene(apt, "open220")
    other = apt.gen_data.build_grid(apt.gen_data.gen_scene_open(100, seed=9)[0], 100)
    d_other = torch.from_numpy(other.view(np.int32)).cuda()
    apt.render.check_device_status()                                             # nothing pending
    for s_, k in ((1, 0), (8, 1)):
        p = sc.params(W, H, s_, 3, seed=2)
        p.flags |= apt.APT_FLAG_GRID_SLOTS
        p.accel = d_other.data_ptr()
        film = torch.full((3, W * H), -2.0, dtype=torch.float32, device="cuda")
        apt.render.render_frame_film(p, sc.d_sph, sc.d_mat, film=film, pass_index=k)
        torch.cuda.synchronize()
        assert (film.cpu().numpy() == -2.0).all()
        with pytest.raises(apt.AptError, match="grid-mismatch"):
            apt.render.check_device_status()                                     # reads and clears the word


def test_the_entrys_own_refusals(apt):
    import torch
    sc = _scene(apt, "open8")
    L = apt._lib.lib()
    p = sc.params(W, H, 8, 2)
    film = torch.full((3, W * H), -2.0, dtype=torch.float32, device="cuda")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda q, mat, fl, n=W * H: L.apt_render_frame_film(ctypes.byref(q), None, ptr(sc.d_sph), mat, None, ctypes.c_uint64(0), ctypes.c_uint64(n), fl,
                                                              ctypes.c_uint32(0))
    assert call(p, ptr(sc.d_mat), None) == 1 and b"film" in L.apt_last_error()
    assert call(p, None, ptr(film)) == 1 and b"materials" in L.apt_last_error()
    assert call(p, None, None) == 1 and b"materials" in L.apt_last_error()       # the frame entries' refusals come first
    assert call(p.copy(samples=4200), ptr(sc.d_mat), ptr(film)) == 1 and b"44 leaves" in L.apt_last_error()
    assert call(p.copy(samples=4200), ptr(sc.d_mat), None) == 1 and b"44 leaves" in L.apt_last_error()
    assert call(p, ptr(sc.d_mat), ptr(film), W * H + 1) == 1 and b"pixel range" in L.apt_last_error()
    bad = p.copy()
    bad.struct_size = 8
    assert call(bad, ptr(sc.d_mat), ptr(film)) == 2
    torch.cuda.synchronize()
    assert (film.cpu().numpy() == -2.0).all()
    with pytest.raises(apt.AptError, match="film"):
        apt.render.render_frame_film(p, sc.d_sph, sc.d_mat, film=torch.zeros((3, 5), dtype=torch.float32, device="cuda"))


# ---- resolve -----------------------------------------------------------------------------------------------------------------------------
def resolve_device(apt, film, passes, exposure, tonemap, inv_white2, d_table, offset=0, want_out=True, want_u8=True):
    """apt_film_resolve_device on a host [3][n] film -> (out, u8, guards intact); the 8-bit image sits `offset` bytes into an allocation."""
    import torch
    L = apt._lib.lib()
    n = film.shape[1]
    d_film = dev(film)
    rec = apt._lib.film_resolve_record(passes, exposure, tonemap, inv_white2)
    out = torch.full((3, n), -7.0, dtype=torch.float32, device="cuda")
    block = torch.full((3 * n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert block.data_ptr() % 4 == 0
    rc = L.apt_film_resolve_device(ctypes.byref(rec), None, ctypes.c_void_p(d_film.data_ptr()), ctypes.c_uint64(n), ctypes.c_void_p(d_table.data_ptr()),
                                   ctypes.c_void_p(out.data_ptr()) if want_out else None, ctypes.c_void_p(block.data_ptr() + offset) if want_u8 else None)
    assert rc == 0, L.apt_last_error()
    torch.cuda.synchronize()
    hb = block.cpu().numpy()
    guards = np.all(hb[:offset] == 0xA5) and np.all(hb[offset + 3 * n:] == 0xA5)
    return out.cpu().numpy(), hb[offset:offset + 3 * n].reshape(n, 3).copy(), guards


@pytest.mark.parametrize("curve", [fr.CURVE_LINEAR, fr.CURVE_SRGB], ids=["linear", "srgb"])
@pytest.mark.parametrize("tonemap", [fr.TONEMAP_CLIP, fr.TONEMAP_REINHARD], ids=["clip", "reinhard"])
def test_resolve_device_equals_the_host_twin(apt, tonemap, curve):
    tables = [apt.gen_data.film_curve(c) for c in (fr.CURVE_LINEAR, fr.CURVE_SRGB)]
    table, d_table = tables[curve], dev(tables[curve])
    pool = fr.value_pool(tables)
    pool = np.concatenate([pool, np.zeros(-len(pool) % 3, dtype=F)])
    whole = pool.reshape(3, -1)                                                  # more than two workgroups of pixels
    assert whole.shape[1] > 512
    for passes, exposure, iw in ((1, 1.0, 0.0), (3, 0.25, 1.0 / 16.0), (1000, 7.5, 1.0 / 16.0), (3, 7.5, 0.0)):
        out, u8, guards = resolve_device(apt, whole, passes, exposure, tonemap, iw, d_table)
        rc, want_out, want_u8, _ = fr.resolve_host(apt, whole, passes, exposure, tonemap, iw, table)
        assert rc == 0 and guards
        assert_bits_equal(out, want_out)
        assert np.array_equal(u8, want_u8)
    for n in (1, 2, 3, 5, 64, 257):
        for offset in range(4):
            film = np.resize(np.roll(pool, n + offset), (3, n))
            out, u8, guards = resolve_device(apt, film, 3, 7.5, tonemap, 1.0 / 16.0, d_table, offset)
            rc, want_out, want_u8, _ = fr.resolve_host(apt, film, 3, 7.5, tonemap, 1.0 / 16.0, table)
            assert guards
            assert_bits_equal(out, want_out)
            assert np.array_equal(u8, want_u8)
    film = np.resize(pool, (3, 300))
    rc, want_out, want_u8, _ = fr.resolve_host(apt, film, 1, 1.0, tonemap, 0.0, table)
    out, u8, _ = resolve_device(apt, film, 1, 1.0, tonemap, 0.0, d_table, want_u8=False)
    assert_bits_equal(out, want_out)
    assert np.all(u8 == 0xA5)
    out, u8, _ = resolve_device(apt, film, 1, 1.0, tonemap, 0.0, d_table, offset=1, want_out=False)
    assert np.all(out == -7.0) and np.array_equal(u8, want_u8)


def test_resolve_device_refusals_write_nothing(apt):
    import torch
    L = apt._lib.lib()
    d_table = dev(apt.gen_data.film_curve("srgb"))
    film = torch.full((3, 5), 0.5, dtype=torch.float32, device="cuda")
    out = torch.full((3, 5), -7.0, dtype=torch.float32, device="cuda")
    u8 = torch.full((5, 3), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    good = lambda **kw: apt._lib.film_resolve_record(**{**dict(passes=2, exposure=1.0, tonemap=0, inv_white2=0.0), **kw})
    call = lambda rec, f=film, t=d_table, o=out, u=u8: L.apt_film_resolve_device(None if rec is None else ctypes.byref(rec), None, ptr(f), ctypes.c_uint64(5),
                                                                                 ptr(t), ptr(o), ptr(u))
    assert call(None) == 1 and call(good(), f=None) == 1 and call(good(), t=None) == 1 and call(good(), o=None, u=None) == 1
    assert call(good(passes=0)) == 1 and call(good(tonemap=2)) == 1 and call(good(exposure=-1.0)) == 1 and call(good(inv_white2=float("nan"))) == 1
    rec = good()
    rec.struct_size = 20
    assert call(rec) == 2
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (u8.cpu().numpy() == 0xA5).all()


def test_resolve_of_a_real_film(apt):
    sc = _scene(apt, "open8")
    p = sc.params(W, H, 9, 2, mode="nee", seed=11)                               # test_five_passes' launch: its restatement is shared
    env = sky_and_sun(apt)
    snaps, _ = sc.film_passes(p, "nee", env, None, 5, checkpoints=(5,))
    assert_bits_equal(snaps[5], fr.accumulate([_pass_ref(sc, p, "nee", env, None, k)[0] for k in range(5)]))
    for tonemap, curve, exposure, iw in ((fr.TONEMAP_CLIP, "srgb", 1.0, 0.0), (fr.TONEMAP_REINHARD, "srgb", 0.5, 1.0 / 64.0), (fr.TONEMAP_REINHARD, "linear", 2.0, 0.0)):
        table = apt.gen_data.film_curve(curve)
        out, u8, guards = resolve_device(apt, snaps[5], 5, exposure, tonemap, iw, dev(table), offset=3)
        rc, want_out, want_u8, _ = fr.resolve_host(apt, snaps[5], 5, exposure, tonemap, iw, table)
        assert rc == 0 and guards
        assert_bits_equal(out, want_out)
        assert np.array_equal(u8, want_u8)
        ref_out, ref_u8 = fr.resolve(snaps[5], 5, exposure, tonemap, iw, table)
        assert_bits_equal(out, ref_out)
        assert np.array_equal(u8, ref_u8) and len(np.unique(u8)) > 50


# ---- render.Film ---------------------------------------------------------------------------------------------------------------------------
def test_film_object_end_to_end(apt, tmp_path):
    import torch
    sc = _scene(apt, "open8")
    p = sc.params(W, H, 9, 2, mode="nee", seed=11)
    env = sky_and_sun(apt)
    refs = [_pass_ref(sc, p, "nee", env, None, k)[0] for k in range(3)]
    ctx = apt.render.Context()
    try:
        ctx.set_environment(env)
        film = apt.render.Film(W, H)
        for _ in range(3):
            film.add_pass(p, sc.d_sph, sc.d_mat, context=ctx)
        torch.cuda.synchronize()
        ctx.check()
        assert film.passes == 3
        total = fr.accumulate(refs)
        assert_bits_equal(film.buffer.cpu().numpy(), total)
        assert_bits_equal(film.mean().cpu().numpy(), total / F(3))
        u8, out = film.resolve(exposure=0.5, tonemap="reinhard", white=8.0, curve="srgb", want_float=True)
        torch.cuda.synchronize()
        rc, want_out, want_u8, _ = fr.resolve_host(apt, total, 3, 0.5, fr.TONEMAP_REINHARD, 1.0 / 64.0, apt.gen_data.film_curve("srgb"))
        assert rc == 0
        assert_bits_equal(out.cpu().numpy(), want_out)
        assert np.array_equal(u8.cpu().numpy(), want_u8)
        assert np.array_equal(film.resolve().cpu().numpy(), fr.resolve(total, 3, 1.0, fr.TONEMAP_CLIP, 0.0, apt.gen_data.film_curve("srgb"))[1])
        path = tmp_path / "film.pfm"
        film.write_pfm(path)
        data = open(path, "rb").read()
        assert data.startswith(b"PF\n48 32\n-1.0\n") and len(data) == 14 + W * H * 12
        px = np.frombuffer(data[14:], dtype="<f4").reshape(H, W, 3)
        assert_bits_equal(px[5, 7], (total / F(3))[:, 7 * H + 5])
        film.reset()
        film.add_pass(p, sc.d_sph, sc.d_mat, context=ctx)
        torch.cuda.synchronize()
        assert film.passes == 1
        assert_bits_equal(film.buffer.cpu().numpy(), refs[0])
        got = ctx.render_frame_film(p, sc.d_sph, sc.d_mat)                       # the thin wrapper: a film of its own, pass 0
        torch.cuda.synchronize()
        assert_bits_equal(got.cpu().numpy(), refs[0])
    finally:
        ctx.close()
