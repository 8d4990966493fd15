"""List passes on the GPU (APT_FLAG_PIXEL_LIST; include/render_mi355x.h "List passes"): every kernel of film_list.hip -- 18 film
kernels (3 scene forms x 3 light modes x 2 groups) and their 12 APT_FLAG_MIS forms -- reached through the entry and the parameters that
select it, and held bit for bit to the restatement: film_ref's pass of the WHOLE frame with the same pass index, gathered at the listed
pixels (tests/adaptive_ref.py), with the status word clean, the trace counter equal to the restatement's segments of the listed
pixels' paths, the scratch stored over NaN and the floats after 3 * count untouched.

The rows are generated below; mat_rows.mat_kernel() restates the routing (materials.hip, pt_mat_launch.h) and names a row's kernel as
the ISA names it.  One row per kernel (`k` rows) rotating over the lists of adaptive_ref.gpu_lists -- every pixel in order, one entry, 17 and
1001 strided entries that wrap round the image, a descending list, a list with repeated entries --, samples 3 (GROUP 1) and 8 / 9
(GROUP 8), depth 1 / 3 / 5, roulette, the reference camera / the context's camera with a lens, no environment / the sun sampled / not
sampled, pass index 0 / 2; frames are 48 x 32, 24 x 16 on the 220-sphere scene.  On top of them the rows about one rule: 129 samples
(a plan of two leaves), the 220 spheres by tiles against their grid, an entry beyond the image, the refusals, and the whole image as a
list against the plain film entry.

The CPU tests hold the rows to film_list.s's kernel list (names only) and to these classes; tests/test_adaptive_cpu.py holds the lists
to telling a list pass from three wrong renderers."""
import ctypes

import numpy as np
import pytest

import adaptive_ref as ar
import film_ref as fr
import materials_ref as mr
from gpu_harness import apt, assert_bits_equal, bits_equal, dev, inside_lens, oracle_params, scene, sky_and_sun  # noqa: F401
from mat_rows import code_object_kernels, mat_kernel, needs_hipcc, rays_of

F, U, U32 = np.float32, np.uint64, np.uint32
MODES = ("plain", "nee", "table")
NS = {"gloss8-lamp": 8, "gloss9-lamp": 9, "open8": 8, "open40": 40, "open220": 220}
CLOSED, OPEN = ("gloss8-lamp", "gloss9-lamp", "gloss9-lamp"), ("open8", "open40", "open220")
LISTS = ("all", "one", "strided17", "many", "descending", "repeat")
KERNELS = 30
GUARD = 8
APT_ERR_ARG = 1


def _row(var, scene_name, mode, grid=False, mis=False, s=3, depth=3, rr=False, cam=None, env=None, seed=3, lst="strided17", k=0):
    w, h = (24, 16) if scene_name == "open220" or s > 100 else (48, 32)
    r = dict(var=var, scene=scene_name, mode=mode, grid=grid, mis=mis, s=s, depth=depth, rr=rr, cam=cam, env=env, seed=seed, list=lst, k=k, w=w, h=h,
             kernel=mat_kernel("film", NS[scene_name], grid, mode, s, mis=mis, listed=True)[1])
    r["id"] = "|".join(str(x) for x in (r["kernel"], var, scene_name + ("+grid" if grid else ""), mode + ("+mis" if mis else ""), f"s{s}",
                                        f"d{depth}" + ("rr" if rr else ""), cam or "ref", env or "noenv", lst, f"pass{k}"))
    return r


def _rows():
    rows, i = [], 0
    for mis in (False, True):
        for form in (0, 1, 2):
            for mode in MODES[1:] if mis else MODES:
                for group in (1, 8):
                    # (group alternates with i: what rotates is counted in kernel pairs, shifted by the group.  Depth 1 sees emitters
                    # only: it meets the lists that hold many pixels, so that no row lists black pixels alone)
                    pair, g = i // 2, i % 2
                    env = (None, "sun", "nosun")[(pair // 2 + g) % 3]
                    # the MIS kernels need gloss words and a light: the 8-sphere room has both, open8 has no gloss words
                    name = OPEN[form] if env and not (mis and form == 0) else CLOSED[form]
                    rows.append(_row("k", name, mode, form == 2, mis, s=3 if group == 1 else (8, 9)[pair % 2], depth=(1, 3, 5)[pair % 3],
                                     rr=(pair + 2 * g) % 4 == 1, cam=(None, "lens")[(pair // 3 + g) % 2], env=env, seed=3 + i % 5,
                                     lst=LISTS[(pair + 3 * g) % 6], k=(0, 2)[(pair // 2) % 2]))
                    i += 1
    rows.append(_row("leaf2", "gloss8-lamp", "nee", s=129, depth=3, lst="strided17", k=2))
    for grid in (False, True):                      # the same launch by tiles and through the grid
        rows.append(_row("tiles-grid", "open220", "table", grid, s=9, depth=5, env="sun", cam="lens", lst="many", k=2))
    return rows


ROWS = _rows()
K_ROWS = [r for r in ROWS if r["var"] == "k"]


# ---- CPU: the rows -----------------------------------------------------------------------------------------------------------------------
def test_rows_are_well_formed():
    assert len({r["id"] for r in ROWS}) == len(ROWS)
    assert len(K_ROWS) == len({r["kernel"] for r in K_ROWS}) == KERNELS
    assert {r["kernel"] for r in ROWS} == {r["kernel"] for r in K_ROWS}
    assert {r["s"] for r in ROWS} == {3, 8, 9, 129} and {r["depth"] for r in K_ROWS} == {1, 3, 5}
    assert {r["cam"] for r in K_ROWS} == {None, "lens"} and {r["env"] for r in K_ROWS} == {None, "sun", "nosun"}
    assert {r["list"] for r in K_ROWS} == set(LISTS) and {r["k"] for r in K_ROWS} == {0, 2}
    for name in LISTS:                              # every list meets both groups
        assert {r["s"] >= 8 for r in K_ROWS if r["list"] == name} == {False, True}, name
    assert any(r["rr"] for r in K_ROWS if r["s"] < 8) and any(r["rr"] for r in K_ROWS if r["s"] >= 8)
    assert {m for r in K_ROWS for m in [r["mode"] + ("+mis" if r["mis"] else "")]} == {"plain", "nee", "table", "nee+mis", "table+mis"}
    assert {(r["w"], r["h"]) for r in ROWS if r["scene"] == "open220"} == {(24, 16)}
    assert {r["grid"] for r in ROWS if r["scene"] == "open220" and r["var"] == "tiles-grid"} == {False, True}
    for npix in (48 * 32, 24 * 16):
        lists = _lists(npix)
        assert lists["all"].size == npix and lists["one"].size == 1 and lists["one"][0] != 0 and lists["strided17"].size == 17
        assert lists["many"].size == min(1001, npix - npix // 4 - 1) and lists["many"].size % 64 != 0 and np.unique(lists["many"]).size == lists["many"].size
        assert np.all(np.diff(lists["descending"].astype(np.int64)) < 0) and np.unique(lists["repeat"]).size < lists["repeat"].size
        assert all(v.max() < npix for v in lists.values())


@needs_hipcc
def test_every_kernel_of_film_list_s_has_exactly_one_row():
    """Kernel names only: no instruction is looked at."""
    names = code_object_kernels("film_list")
    render = sorted(n for n in names if n.startswith("render_frame_mat_kernel"))
    assert names - set(render) == {"gen_rays_camera_kernel"}
    assert render == sorted(r["kernel"] for r in K_ROWS) and len(render) == KERNELS


# ---- what a row expects ------------------------------------------------------------------------------------------------------------------
def _lists(npix):
    lists = ar.gpu_lists(npix)
    many = [k for k in lists if k.startswith("strided") and k != "strided17"]
    assert len(many) == 1
    lists["many"] = lists.pop(many[0])
    return lists


def _camera(pkg, r):
    return None if r["cam"] is None else inside_lens(pkg, r["w"], r["h"])


def _env(pkg, r):
    return None if r["env"] is None else sky_and_sun(pkg, r["env"] == "sun")


def _params(pkg, sc, r, grid=False):
    return sc.params(r["w"], r["h"], r["s"], r["depth"], mode=r["mode"], rr=r["rr"], seed=r["seed"], grid=grid,
                     flags=pkg.APT_FLAG_MIS if r["mis"] else 0)


_WHOLE = {}


def _inputs(pkg, r):
    """What the restatement reads of the row -> (the launch as an oracle.Params, spheres, words, camera record, Env, table)."""
    sc = scene(pkg, r["scene"])
    q = oracle_params(_params(pkg, sc, r))
    assert not r["mis"] or (q.flags & mr.FLAG_GLOSS and r["mode"] != "plain")
    env = None if r["env"] is None else mr.Env.from_ctypes(_env(pkg, r))
    return q, sc.sph, sc.mat, _camera(pkg, r), env, sc.table if r["mode"] == "table" else None


def whole(pkg, r, k):
    """The planes [3][W * H] of pass k of the row's whole frame, and its segments: film_ref.render_pass, computed once."""
    key = (r["scene"], r["mode"], r["mis"], r["s"], r["depth"], r["rr"], r["cam"], r["env"], r["seed"], r["w"], r["h"], k)
    if key not in _WHOLE:
        q, sph, mat, cam, env, table = _inputs(pkg, r)
        _WHOLE[key] = fr.render_pass(q, sph, mat, env, table, pass_index=k, rays=None if cam is None else (lambda seed: rays_of(q, cam, seed)))
    return _WHOLE[key]


def listed_segments(pkg, r, lst, k):
    """The segments of the paths of the listed pixels inside the image, an entry counted as often as it is listed: what the trace
    counter of a list launch holds.  Their colours are traced again on the way: they must be the whole frame's."""
    from oracle import oracle
    q, sph, mat, cam, env, table = _inputs(pkg, r)
    seed = fr.pass_seed(q.seed, k)
    inside = lst[lst < r["w"] * r["h"]].astype(np.int64)
    per = 4 * r["s"]
    paths = (inside[:, None] * per + np.arange(per)[None, :]).ravel()
    L, bad, seg = mr.trace_params(q, rays_of(q, cam, seed)[:, paths], sph, mat, env, table, paths=paths.astype(U), seed=seed)
    assert not bad.any()
    pre = oracle.decode_color(L, inside.size, 1, r["s"])[0]
    assert_bits_equal(np.ascontiguousarray(pre.T).astype(F), whole(pkg, r, k)[0][:, inside])
    return seg


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
def launch(apt, r, lst, k, fill=float("nan"), check=True):
    """The row's list launch of pass k -> (scratch [3][len(lst)], the GUARD floats after it, segments traced)."""
    import torch
    sc = scene(apt, r["scene"])
    p = _params(apt, sc, r, grid=r["grid"])
    m = lst.size
    buf = torch.full((3 * m + GUARD,), fill, dtype=torch.float32, device="cuda")
    d_list = dev(lst.astype(U32).view(np.int32))
    _, traced = sc._launch(_camera(apt, r), _env(apt, r), check, True, lambda: apt.render.render_frame_film(
        p, sc.d_sph, sc.d_mat, film=buf[:3 * m], pass_index=k, lights=sc.d_table if r["mode"] == "table" else None, pixel_list=d_list))
    out = buf.cpu().numpy()
    return out[:3 * m].reshape(3, m), out[3 * m:], traced


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_list_kernel_equals_the_restatement(apt, row):
    r = row
    lst = _lists(r["w"] * r["h"])[r["list"]]
    planes, seg_whole = whole(apt, r, r["k"])
    got, guard, traced = launch(apt, r, lst, r["k"])                               # over NaN: the launch stores, whatever the pass index
    assert_bits_equal(got, ar.list_pass(planes, lst))
    assert np.isnan(guard).all() and got.any()                                     # (a list of black pixels would show nothing)
    assert traced == listed_segments(apt, r, lst, r["k"]), (traced, seg_whole)
    if r["list"] == "all":
        assert traced == seg_whole
    if r["var"] == "tiles-grid" and r["grid"]:                                     # the grid changes which spheres are tested, never the bits
        tiles = next(x for x in ROWS if x["var"] == "tiles-grid" and not x["grid"])
        assert_bits_equal(got, launch(apt, tiles, lst, r["k"])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("s", [3, 9])
def test_the_whole_image_as_a_list_is_the_plain_film_pass(apt, s):
    """Device against device, and both against the restatement: pass 0 as the film entry stores it, and pass 2 as it adds it to a
    zeroed film."""
    import torch
    r = _row("whole", "gloss8-lamp", "nee", s=s, depth=3, seed=4, lst="all")
    sc = scene(apt, r["scene"])
    p = _params(apt, sc, r)
    n = r["w"] * r["h"]
    lst = _lists(n)["all"]
    for k in (0, 2):
        film = torch.zeros((3, n), dtype=torch.float32, device="cuda")
        sc._launch(None, None, True, False, lambda: apt.render.render_frame_film(p, sc.d_sph, sc.d_mat, film=film, pass_index=k))
        got, _, _ = launch(apt, r, lst, k)
        assert_bits_equal(got, film.cpu().numpy())
        assert_bits_equal(got, whole(apt, r, k)[0])
    assert not bits_equal(whole(apt, r, 0)[0], whole(apt, r, 2)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("s", [3, 8])
def test_an_entry_beyond_the_image_is_skipped_and_reported(apt, s):
    """Its slot is untouched, every other slot is right, APT_DEV_LIST_RANGE is reported and cleared; with entry 0 itself beyond the
    image the other entries are still right."""
    r = _row("beyond", "gloss8-lamp", "table", s=s, depth=3, seed=5)
    n = r["w"] * r["h"]
    for lst in (np.array([700, n, 31, 0xFFFFFFFF, 702, n + 5, 40], dtype=U32), np.array([n, 700, 31], dtype=U32),
                np.concatenate([_lists(n)["strided17"], [n], _lists(n)["many"][:90]]).astype(U32)):
        got, guard, traced = launch(apt, r, lst, 2, fill=-5.0, check=False)
        with pytest.raises(apt.AptError, match="list-range"):
            apt.render.check_device_status()
        apt.render.check_device_status()                                           # reported once: the word is clean again
        inside = lst < n
        assert (got[:, ~inside] == F(-5)).all() and (guard == F(-5)).all()
        assert_bits_equal(got[:, inside], ar.list_pass(whole(apt, r, 2)[0], lst)[:, inside])
        assert traced == listed_segments(apt, r, lst, 2)


@pytest.mark.gpu
def test_refusals_of_a_list_launch(apt):
    """What replaces the range check: a list address that is 0 or not 4-byte aligned, more entries than pixels; an empty list is
    APT_OK and launches nothing; the film entry's own refusals stay (a NULL film comes last)."""
    import torch
    L = apt._lib.lib()
    r = _row("refuse", "gloss8-lamp", "nee", s=3)
    sc = scene(apt, r["scene"])
    n = r["w"] * r["h"]
    p = _params(apt, sc, r)
    p = p.copy(flags=p.flags | apt.APT_FLAG_PIXEL_LIST)
    d_list = dev(np.arange(n + 1, dtype=np.int32))
    film = torch.full((3 * (n + 1),), -5.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(address, count, film_ptr=film.data_ptr(), params=p):
        return L.apt_render_frame_film(ctypes.byref(params), st, sc.d_sph.data_ptr(), sc.d_mat.data_ptr(), None, address, count, film_ptr, 1)

    assert call(0, 4) == APT_ERR_ARG and b"pixel list" in L.apt_last_error()
    for off in (1, 2, 3):
        assert call(d_list.data_ptr() + off, 4) == APT_ERR_ARG
    assert call(d_list.data_ptr(), n + 1) == APT_ERR_ARG
    assert call(d_list.data_ptr(), 4, params=p.copy(width=1 << 17, height=1 << 16)) == APT_ERR_ARG and b"2^32" in L.apt_last_error()
    assert call(d_list.data_ptr(), 0) == 0                                         # nothing launched
    assert call(d_list.data_ptr(), 4, film_ptr=None) == APT_ERR_ARG and b"film" in L.apt_last_error()
    assert call(d_list.data_ptr(), 4, params=p.copy(samples=0)) != 0               # check_params' refusals come first, as ever
    torch.cuda.synchronize()
    assert (film.cpu().numpy() == F(-5)).all()
    apt.render.check_device_status()
    # every other entry ignores the bit: a frame with it is the frame without it
    q = _params(apt, sc, r)
    a = sc.frame(q, "nee")
    b = sc.frame(q.copy(flags=q.flags | apt.APT_FLAG_PIXEL_LIST), "nee")
    assert_bits_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    with pytest.raises(apt.AptError):                                              # the Python entry sets the flag itself
        apt.render.render_frame_film(p, sc.d_sph, sc.d_mat)
