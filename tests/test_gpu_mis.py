"""APT_FLAG_MIS on the GPU (include/render_mi355x.h "Multiple importance sampling"): every kernel of mis.hip -- 24 frame kernels (3 scene
forms x APT_FLAG_NEE / a light table x 2 groups, each with the decode tail and with the film tail) and 6 buffer kernels -- reached
through the entry and the parameters that select it and held to the NumPy restatement tests/materials_ref.py: fb bit for bit, fb_u8 exactly,
the trace counter against the restatement's segments, the status word clean.  Every row's image must also differ from the same launch
without the flag, so a router that silently ignores the bit fails.

The rows are generated below; mat_rows.mat_kernel() restates the routing (materials.hip, pt_mat_launch.h) and names a row's kernel as
the ISA names it.  One row per kernel (`k` rows), rotating over them: samples 1 / 7 (GROUP 1) and 8 / 9 (GROUP 8), depth 2 / 3 / 4, roulette,
the reference camera / a pinhole / a thin lens, no environment / a sky with the sampled sun, and the scenes -- the 8-sphere lamp room
whose rough ball is itself a listed light, the 9-sphere room by tiles and behind its grid (built on the host and on the device), the
1030-sphere scene by tiles and behind its grid.  On top of them the rows that are about one rule: depth 1, a one-light table against
APT_FLAG_NEE, a table without gloss words, a two-leaf plan, a camera inside a listed light, a table of another scene.

The CPU tests hold the rows to mis.s's kernel list (names only) and to these classes."""
import numpy as np
import pytest

import film_ref as fr
import lights_ref as lr
import materials_ref as mr
from gpu_harness import Scene, apt, assert_bits_equal, bits_equal, dev, host, inside_lens, inside_pinhole, oracle_params, same, scene, sky_and_sun  # noqa: F401
from mat_rows import code_object_kernels, mat_kernel, needs_hipcc, rays_of

F = np.float32
MODES = ("nee", "table")
SAMPLES = {1: (1, 7), 8: (8, 9)}
TWO_LEAVES = 136
NS = {"gloss8-lamp": 8, "gloss9-lamp": 9, "big1030g": 1030, "furnace3": 3}
FORM_SCENE = ("gloss8-lamp", "gloss9-lamp", "gloss9-lamp")
KERNELS = 30
BIG_ROWS = 6                                  # rows on the 1030-sphere scene: the budget of tests/test_gpu_material_matrix.py


def _row(var, entry, scene_name, mode, grid=False, s=1, depth=3, rr=False, cam=None, env=None, seed=3, w=16, h=8, builder="host", **extra):
    r = dict(var=var, entry=entry, scene=scene_name, mode=mode, grid=grid, s=s, depth=depth, rr=rr, cam=cam, env=env, seed=seed, w=w, h=h,
             builder=builder, kernel=mat_kernel(entry, NS[scene_name], grid, mode, s, mis=True)[1], **extra)
    r["id"] = "|".join(str(x) for x in (r["kernel"], var, scene_name + ("+grid" + ("-dev" if builder == "device" else "") if grid else ""), mode,
                                        f"s{s}", f"d{depth}" + ("rr" if rr else ""), cam or "ref", env or "noenv"))
    return r


def _rows():
    rows, i = [], 0
    cams, envs = (None, "lens", "pin"), (None, "sun")
    for entry in ("frame", "film", "paths"):
        for form in (0, 1, 2):
            for mode in MODES:
                for group in ((1,) if entry == "paths" else (1, 8)):
                    big = form > 0 and entry != "paths" and group == 8 and mode == ("nee" if entry == "frame" else "table")
                    name = "big1030g" if big else FORM_SCENE[form]
                    rows.append(_row("k", entry, name, mode, form == 2, s=3 if entry == "paths" else SAMPLES[group][(i // 2) % 2], depth=2 + i % 3,
                                     rr=i % 4 == 1, cam=None if entry == "paths" else cams[i % 3], env=envs[(i // 3) % 2], seed=3 + i % 5,
                                     w=8 if big else 16, builder="device" if form == 2 and not big and mode == "table" else "host"))
                    i += 1
    # the rows about one rule
    rows.append(_row("depth1", "frame", "gloss8-lamp", "nee", s=7, depth=1))
    rows.append(_row("depth1", "frame", "gloss9-lamp", "table", True, s=8, depth=1))
    rows.append(_row("one-light", "frame", "gloss8-lamp", "table", s=9, depth=4, one_light=True))
    rows.append(_row("one-light", "paths", "gloss9-lamp", "table", s=3, depth=3, one_light=True))
    rows.append(_row("no-gloss-words", "frame", "gloss9-lamp", "table", s=7, depth=4, plain=True))
    rows.append(_row("leaf2", "frame", "gloss8-lamp", "table", s=TWO_LEAVES, depth=2, w=4, h=2))
    rows.append(_row("inside-a-light", "frame", "furnace3", "table", s=8, depth=4, eps=0.5))
    return rows


ROWS = _rows()
K_ROWS = [r for r in ROWS if r["var"] == "k"]


# ---- CPU: the rows -----------------------------------------------------------------------------------------------------------------------
def test_rows_are_well_formed():
    assert len({r["id"] for r in ROWS}) == len(ROWS)
    assert len(K_ROWS) == len({r["kernel"] for r in K_ROWS}) == KERNELS
    assert {r["kernel"] for r in ROWS} == {r["kernel"] for r in K_ROWS}
    frames = [r for r in K_ROWS if r["entry"] != "paths"]
    assert {r["s"] for r in frames} == {1, 7, 8, 9} and {r["depth"] for r in K_ROWS} == {2, 3, 4}
    assert {r["cam"] for r in frames} == {None, "lens", "pin"} and {r["env"] for r in K_ROWS} == {None, "sun"}
    assert any(r["rr"] for r in frames) and any(r["rr"] for r in K_ROWS if r["entry"] == "paths")
    assert {r["builder"] for r in K_ROWS if r["grid"]} == {"host", "device"}
    assert sum(NS[r["scene"]] == 1030 for r in ROWS) <= BIG_ROWS and {r["grid"] for r in ROWS if NS[r["scene"]] == 1030} == {False, True}
    assert all(r["w"] * r["h"] <= 128 for r in ROWS)


@needs_hipcc
def test_every_kernel_of_mis_s_has_exactly_one_row():
    """Kernel names only: no instruction is looked at."""
    names = code_object_kernels("mis")
    render = sorted(n for n in names if n.startswith(("render_frame_mat_kernel", "render_paths_mat_kernel")))
    assert names - set(render) == {"gen_rays_camera_kernel"}
    assert render == sorted(r["kernel"] for r in K_ROWS) and len(render) == KERNELS


# ---- what a row expects ------------------------------------------------------------------------------------------------------------------
_SCENES = {}


def _scene(pkg, r, launch=False):
    """The row's scene: the harness's, the same table behind a grid built on the device (launch=True only: the restatement knows no
    grid and needs no device), its one-light table, or the furnace."""
    key = (r["scene"], r["builder"] if r["grid"] and launch else "host", bool(r.get("one_light")))
    if key not in _SCENES:
        if r["scene"] == "furnace3":           # the camera sits inside sphere 0, a listed light; a lamp; a rough ball in front of the camera
            sph = lr.table_of([[1000.0, 50.0, 52.0, 295.6, 0.25, 0.25, 0.25, 0.5, 0.5, 0.5], [20.0, 120.0, 200.0, -100.0, 30.0, 20.0, 10.0, 0, 0, 0],
                               [30.0, 50.0, 40.0, 100.0, 0, 0, 0, 0.9, 0.8, 0.7]])
            sc = Scene(pkg, sph, np.array([mr.DIFF, mr.DIFF, pkg.gen_data.gloss(0.3)], dtype=np.int32), 3, [0, 1], 1)
        else:
            base = scene(pkg, r["scene"])
            sc = base
            if key[1] == "device":
                sc = Scene(pkg, base.sph, base.mat, base.ns, base.lights, base.light, grid=True, builder="device")
            elif key[2]:
                sc = Scene(pkg, base.sph, base.mat, base.ns, [base.light], base.light, grid=base.hgrid is not None)
        _SCENES[key] = sc
    return _SCENES[key]


def _camera(pkg, r):
    return None if r["cam"] is None else (inside_lens if r["cam"] == "lens" else inside_pinhole)(pkg, r["w"], r["h"])


def _env(pkg, r):
    return None if r["env"] is None else sky_and_sun(pkg, True)


def _params(pkg, sc, r, grid=False, mis=True, mode=None):
    kw = dict(eps=r["eps"]) if "eps" in r else {}
    return sc.params(r["w"], r["h"], r["s"], r["depth"], mode=mode or r["mode"], rr=r["rr"], seed=r["seed"], grid=grid,
                     flags=pkg.APT_FLAG_MIS if mis else 0, **kw)


_WANT = {}


def want(pkg, r, mis=True, mode=None):
    """The restatement's expectation of the row (mis=False: of the same launch without the flag; mode: of another light mode), computed
    once: frame (fb, u8, segments); film ([planes of pass 0, of pass 1], [segments], the frame entry's fb); paths (L, segments)."""
    key = (r["id"], mis, mode)
    if key in _WANT:
        return _WANT[key]
    sc = _scene(pkg, r)
    mode = mode or r["mode"]
    p = _params(pkg, sc, r, mis=mis, mode=mode)
    q = oracle_params(p)
    mat = sc.plain if r.get("plain") else sc.mat
    cam, env = _camera(pkg, r), _env(pkg, r)
    menv = None if env is None else mr.Env.from_ctypes(env)
    table = sc.table if mode == "table" else None
    if r["entry"] == "paths":
        L, bad, seg = mr.trace_params(q, rays_of(q, cam, q.seed), sc.sph, mat, menv, table)
        assert not bad.any()
        out = (L, seg)
    elif r["entry"] == "frame":
        out = sc.frame_ref(p, mode, cam, env, gloss=not r.get("plain"))
    else:
        rays = None if cam is None else (lambda seed: rays_of(q, cam, seed))
        passes = [fr.render_pass(q, sc.sph, mat, menv, table, pass_index=k, rays=rays) for k in (0, 1)]
        out = ([planes for planes, _ in passes], [seg for _, seg in passes], sc.frame_ref(p, mode, cam, env, gloss=not r.get("plain"))[0])
    _WANT[key] = out
    return out


def _image(r, w):
    return w[0][0] if r["entry"] == "film" else w[0]


def test_the_restatement_of_every_row_differs_from_the_flagless_launch(host):
    """On the restatement alone: a row's expectation is not the flagless image (depth 1 and a table without gloss words: it is)."""
    for r in ROWS:
        a, b = _image(r, want(host, r)), _image(r, want(host, r, mis=False))
        assert np.isfinite(a).all(), r["id"]
        if r["var"] in ("depth1", "no-gloss-words"):
            assert bits_equal(a, b), r["id"]
        else:
            assert not bits_equal(a, b), r["id"]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def _launch(apt, r, mis=True, mode=None):
    """The row's launch -> what want() returns for it."""
    import torch
    sc = _scene(apt, r, launch=True)
    mode = mode or r["mode"]
    p = _params(apt, sc, r, grid=r["grid"], mis=mis, mode=mode)
    cam, env, gloss = _camera(apt, r), _env(apt, r), not r.get("plain")
    if r["entry"] == "frame":
        return sc.frame(p, mode, cam, env, gloss=gloss, count=True)
    if r["entry"] == "film":
        nan = torch.full((3, r["w"] * r["h"]), float("nan"), dtype=torch.float32, device="cuda")     # pass 0 stores over NaN
        snaps, traced = sc.film_passes(p, mode, env, cam, 2, film=nan, checkpoints=(1, 2))
        return [snaps[1], snaps[2]], traced
    rays = rays_of(oracle_params(p), cam, p.seed)
    colors = torch.full((3 * rays.shape[1],), float("nan"), dtype=torch.float32, device="cuda")
    d_rays = dev(rays.ravel())
    _, traced = sc._launch(None, env, True, True, lambda: apt.render.render_do_ex(
        p, None, d_rays, sc.d_sph, colors, materials=sc.d_mat, lights=sc.d_table if mode == "table" else None))
    return colors.cpu().numpy().reshape(3, -1), traced


def _same(r, got, w):
    if r["entry"] == "frame":
        same(got, w)
    elif r["entry"] == "film":
        assert_bits_equal(got[0][0], w[0][0])
        assert_bits_equal(got[0][1], fr.accumulate(w[0]))
        assert_bits_equal(np.clip(got[0][0], F(0), F(1)), w[2])                    # clip(pass 0) is the frame entry's fb
        assert got[1] == w[1], (got[1], w[1])
    else:
        assert_bits_equal(got[0], w[0])
        assert got[1] == w[1], (got[1], w[1])


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_mis_kernel_equals_the_restatement(apt, row):
    r = row
    got = _launch(apt, r)
    _same(r, got, want(apt, r))
    flagless = _launch(apt, r, mis=False)
    _same(r, flagless, want(apt, r, mis=False))                                    # the flagless launch is still materials_ref's image
    if r["var"] in ("depth1", "no-gloss-words"):
        assert bits_equal(_image(r, got), _image(r, flagless)), r["id"]
    else:
        assert not bits_equal(_image(r, got), _image(r, flagless)), r["id"]
    if r.get("one_light"):                                                         # the one-light table IS APT_FLAG_NEE with that light
        _same(r, _launch(apt, r, mode="nee"), want(apt, r))


@pytest.mark.gpu
def test_a_table_of_another_scene_is_reported_and_nothing_is_written(apt):
    import torch
    sc, other = scene(apt, "gloss9-lamp"), scene(apt, "gloss8-lamp")
    p = sc.params(16, 8, 8, 3, mode="table", flags=apt.APT_FLAG_MIS)
    fb = torch.full((3, 128), -3.0, dtype=torch.float32, device="cuda")
    u8 = torch.full((128, 3), 0xA5, dtype=torch.uint8, device="cuda")
    apt.render.render_frame(p, sc.d_sph, fb=fb, fb_u8=u8, materials=sc.d_mat, lights=other.d_table)
    torch.cuda.synchronize()
    with pytest.raises(apt.AptError, match="lights-mismatch"):
        apt.render.check_device_status()
    assert (fb.cpu().numpy() == -3.0).all() and (u8.cpu().numpy() == 0xA5).all()
