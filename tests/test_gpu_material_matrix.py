"""Every kernel instantiation of the material renderer -- the render_frame_mat_kernel<SCN, GROUP> and render_paths_mat_kernel<SCN> of
materials.hip, environment.hip and film.hip, and features.hip's features_kernel<SC> -- each reached through the entry and the parameters
that select it and compared with the NumPy restatements (materials_ref, film_ref, features_ref): fb bit for bit, fb_u8 exactly, the trace
counter against the restatement's segments, the status word clean, and a grid launch against the same launch without its grid.

The rows are generated below.  mat_rows.mat_kernel() restates the routing of materials.hip and pt_mat_launch.h and names, for a row's
parameters, the kernel as the ISA names it; the rows are made by walking every (code object, scene form, light mode, GROUP, camera,
gloss) and asking it for the name, so every kernel has

  a carrier   a whole frame at an odd depth >= 3 whose expected image is non-trivial and changes in bits when one of the row's own axes
              is taken away (test_carrier_rows_would_show_a_failure, on the restatement alone);
  an rr row   roulette (rr_start 2) at an even depth, over a pixel range with an odd begin and a partial last workgroup, band-relative
              inside guard values, with the byte frame NULL, misaligned by one byte or whole; NEE kernels with smallpt's small lamp;

and the edges that rotate over the kernels by an index, so that every edge meets every family without multiplying the rows --

  M1  samples 1 / 3 / 7 (GROUP 1) and 8 / 13 / 16 (GROUP 8); 136 samples, a plan of two leaves, once per (code object, scene form)
  M2  the range and byte-frame forms above; films: pass 0 over a film of NaN and pass 1 adding; buffers: a path range of whole buffers,
      a band buffer, path_count 0 with path_begin > 0
  M3  depth 0 and 1 (extra rows, never carriers), an even depth, an odd depth >= 3, roulette
  M4  APT_FLAG_NEE with with_lamp's lamp; tables of two lights
  M5  environment kernels: the sun sampled and not, a gloss table and a gloss-free one
  M6  camera kernels: a look-at pinhole and a thin lens whose eye is inside the closed room
  and the 8-sphere scene launched with another scene's grid in accel (scene form 0 whatever accel holds), once per light mode.

A buffer row has no fb: its colours are compared per path, and for the carrier conditions a pixel is its 4 * S consecutive paths.

The CPU tests hold the rows to the kernel lists of the four code objects (a kernel added without a row fails the suite), to these
classes, and the carriers to their two conditions."""
import ctypes
import time

import numpy as np
import pytest

import camera_ref as cr
import features_ref as ft
import film_ref as fr
import materials_ref as mr
from gpu_harness import Scene, apt, assert_bits_equal, bits_equal, dev, host, inside_lens, inside_pinhole, oracle_params, scene, sky_and_sun  # noqa: F401
from mat_rows import code_object_kernels, mat_kernel, needs_hipcc, rays_of

F, U = np.float32, np.uint64

MODES = ("plain", "nee", "table")
M1 = {1: (1, 3, 7), 8: (8, 13, 16)}
TWO_LEAVES = 136
W, H = 16, 12                                # 192 pixels: 3 workgroups of GROUP 1 (64 pixels), 24 of GROUP 8 (8 pixels)
FW, FH = 24, 16                              # features_kernel: one lane per pixel, 256 per workgroup
RANGE = (5, 101)                             # an odd begin; 101 = 64 + 37 = 12 * 8 + 5: the last workgroup partial in both groups
FRANGE = (5, 300)                            # features: 256 + 44
U8_FORMS = ("null", "mis", "whole")
PATH_FORMS = (("range", 7, 1001), ("band", 7, 1001), ("band0", 1001, 0))     # 2304 paths (S = 3): a partial last workgroup each
NS = {"gloss8-stock": 8, "gloss8-lamp": 8, "gloss9-stock": 9, "gloss9-lamp": 9, "big1030g": 1030, "open8": 8, "open40": 40, "open220": 220}
CLOSED, OPEN = ("gloss8", "gloss9", "gloss9"), ("open8", "open40", "open220")   # by scene form; form 2: the same table behind its grid
COUNTS = {"materials": 90, "environment": 27, "film": 18, "features": 3}
# kernels of the four code objects that are not render kernels (no row needed)
NOT_RENDER_KERNELS = {"gen_rays_camera_kernel", "selftest_direction_kernel", "film_resolve_kernel"}


# ---- the rows ----------------------------------------------------------------------------------------------------------------------------
def _row(var, entry, scene_name, mode="plain", grid=False, gloss=True, cam=None, env=None, s=1, depth=5, rr=False, rng=None, u8="whole",
         paths="whole", seed=3, w=W, h=H, accel8=False):
    """accel8: the 8-sphere scene launched with another scene's grid in accel, which the 8-sphere form ignores."""
    assert not accel8 or (NS[scene_name] == 8 and not grid and entry == "frame")
    co, kernel = mat_kernel(entry, NS[scene_name], grid or accel8, mode, s, gloss, cam is not None, env is not None)
    r = dict(var=var, entry=entry, scene=scene_name, mode=mode, grid=grid, gloss=gloss, cam=cam, env=env, s=s, depth=depth, rr=rr, range=rng,
             u8=u8, paths=paths, seed=seed, w=w, h=h, accel8=accel8, co=co, kernel=kernel, group=8 if s >= 8 else 1)
    rid = f"{co}|{kernel}|{var}|{scene_name}{'+grid' if grid else ''}|{mode}|s{s}|d{depth}{'rr' if rr else ''}"
    rid += ("|gloss" if gloss else "") + (f"|{cam}" if cam else "") + (f"|{env}" if env else "")
    if rng:
        rid += f"|px{rng[0]}+{rng[1]}|u8{u8}"
    if entry == "paths":
        rid += "|" + (paths if isinstance(paths, str) else "%s%d+%d" % paths)
    r["id"] = rid + ("|accel8" if accel8 else "")
    return r


def _extras(rows, i, **kw):
    """M3's depth 0 and depth 1, rotating over the kernels of a family: extra rows, never carriers."""
    if i % 4 == 0:
        rows.append(_row("d0", depth=0, **kw))
    elif i % 4 == 2:
        rows.append(_row("d1", depth=1, **kw))


def _materials_frame_rows():
    rows, i = [], 0
    for form in (0, 1, 2):
        j = {1: 0, 8: 0}
        for mi, mode in enumerate(MODES):
            for group in (1, 8):
                for cam_on in (False, True):
                    for gloss in (False, True):
                        kinds = ("pin", "lens") if (i + i // 4 + i // 8) % 2 == 0 else ("lens", "pin")
                        base = dict(entry="frame", mode=mode, grid=form == 2, gloss=gloss, seed=3 + i % 5)
                        rows.append(_row("carrier", scene_name=CLOSED[form] + "-stock", cam=kinds[0] if cam_on else None, s=M1[group][i % 3],
                                         depth=5, **base))
                        rows.append(_row("rr", scene_name=CLOSED[form] + ("-lamp" if mode == "nee" else "-stock"), cam=kinds[1] if cam_on else None,
                                         s=M1[group][(i + 1) % 3], depth=4, rr=True, rng=RANGE, u8=U8_FORMS[j[group] % 3], **base))
                        _extras(rows, i + mi + form, scene_name=CLOSED[form] + "-stock", cam=kinds[0] if cam_on else None, s=M1[group][(i + 2) % 3], **base)
                        j[group] += 1
                        i += 1
        # two leaves: the LDS stack beside the camera record
        rows.append(_row("leaf2", "frame", CLOSED[form] + "-stock", MODES[form], form == 2, form % 2 == 0, "lens", s=TWO_LEAVES, depth=2, seed=5))
        if form == 0:                                                             # scene form 0 whatever accel holds
            for mi, mode in enumerate(MODES):
                rows.append(_row("accel8", "frame", "gloss8-stock", mode, False, mi % 2 == 0, None, s=(7, 8, 3)[mi], depth=3, seed=6, accel8=True))
        # 1030 spheres: two LDS tiles, and a grid with binned spheres
        if form:
            for mi, mode in enumerate(MODES):
                rows.append(_row("big", "frame", "big1030g", mode, form == 2, (mi + form) % 2 == 0, None, s=13, depth=3, seed=7))
    return rows


def _environment_frame_rows():
    rows, i = [], 0
    cams = (None, "pin", "lens")
    for form in (0, 1, 2):
        for mi, mode in enumerate(MODES):
            for gi, group in enumerate((1, 8)):
                sun, gloss = (form + mi + gi) % 2 == 0, (form + mi // 2 + gi) % 2 == 0
                base = dict(entry="frame", scene_name=OPEN[form], mode=mode, grid=form == 2, seed=3 + i % 5)
                rows.append(_row("carrier", gloss=gloss, cam=cams[i % 3], env="sun" if sun else "nosun", s=M1[group][i % 3],
                                 depth=3 if form == 2 else 5, **base))
                rows.append(_row("rr", gloss=not gloss, cam=cams[(i + 1) % 3], env="nosun" if sun else "sun", s=M1[group][(i + 1) % 3], depth=4,
                                 rr=True, rng=RANGE, u8=U8_FORMS[mi], **base))
                _extras(rows, 2 * i, gloss=gloss, cam=cams[(i + 2) % 3], env="sun", s=M1[group][(i + 2) % 3], **base)
                i += 1
        rows.append(_row("leaf2", "frame", OPEN[form], MODES[(form + 1) % 3], form == 2, True, "lens", "sun", s=TWO_LEAVES, depth=2, seed=5))
    return rows


def _film_rows():
    """A film row is two passes: pass 0 over a film of NaN, pass 1 adding.  With an environment on the open scenes, without one (the
    all-zero record) in the closed rooms."""
    rows, i = [], 0
    cams = (None, "lens", "pin")
    for form in (0, 1, 2):
        for mi, mode in enumerate(MODES):
            for gi, group in enumerate((1, 8)):
                with_env = i % 2 == 0
                a = dict(scene_name=OPEN[form], env="sun" if (i // 2) % 2 else "nosun")
                b = dict(scene_name=CLOSED[form] + ("-lamp" if mode == "nee" else "-stock"), env=None)
                base = dict(entry="film", mode=mode, grid=form == 2, seed=3 + i % 5)
                rows.append(_row("carrier", gloss=i % 3 != 0, cam=cams[i % 3], s=M1[group][i % 3], depth=3, **base, **(a if with_env else b)))
                rows.append(_row("rr", gloss=i % 3 != 1, cam=cams[(i + 1) % 3], s=M1[group][(i + 1) % 3], depth=4, rr=True, rng=RANGE,
                                 **base, **(b if with_env else a)))
                _extras(rows, 2 * i, gloss=True, cam=cams[(i + 2) % 3], s=M1[group][(i + 2) % 3], **base, **a)
                i += 1
        rows.append(_row("leaf2", "film", OPEN[form], MODES[(form + 2) % 3], form == 2, True, "pin", "sun", s=TWO_LEAVES, depth=2, seed=5))
    return rows


def _paths_rows():
    """Buffer mode: S = 3, 2304 paths, the rays of the reference camera."""
    rows, i = [], 0
    for form in (0, 1, 2):
        for mi, mode in enumerate(MODES):
            for gloss in (False, True):                                           # materials.hip
                base = dict(entry="paths", mode=mode, grid=form == 2, gloss=gloss, s=3, seed=3 + i % 5)
                rows.append(_row("carrier", scene_name=CLOSED[form] + "-stock", depth=5, **base))
                rows.append(_row("rr", scene_name=CLOSED[form] + ("-lamp" if mode == "nee" else "-stock"), depth=4, rr=True, paths=PATH_FORMS[i % 3], **base))
                _extras(rows, i + form, scene_name=CLOSED[form] + "-stock", paths=PATH_FORMS[(i + 1) % 3], **base)
                i += 1
            sun, gloss = (form + mi) % 2 == 0, (form + mi // 2) % 2 == 0          # environment.hip: gloss is data
            base = dict(entry="paths", scene_name=OPEN[form], mode=mode, grid=form == 2, s=3, seed=3 + i % 5)
            rows.append(_row("carrier", gloss=gloss, env="sun" if sun else "nosun", depth=3 if form == 2 else 5, **base))
            rows.append(_row("rr", gloss=not gloss, env="nosun" if sun else "sun", depth=4, rr=True, paths=PATH_FORMS[(form + mi) % 3], **base))
            _extras(rows, 2 * (form + mi), gloss=gloss, env="sun", paths=PATH_FORMS[(form + mi + 1) % 3], **base)
    return rows


def _features_rows():
    """features_kernel reads the table, the camera and the grid alone: no light mode, depth, roulette or material word."""
    rows = []
    for form, name in enumerate(("gloss8-stock", "open40", "open220")):
        base = dict(entry="features", scene_name=name, grid=form == 2, w=FW, h=FH, depth=5)
        rows.append(_row("carrier", cam="pin", s=(3, 8, 13)[form], seed=4 + form, **base))
        rows.append(_row("range", cam="lens", s=(16, 1, 7)[form], rng=FRANGE, seed=5 + form, **base))
        rows.append(_row("nocam", cam=None, s=(7, 13, 1)[form], rng=FRANGE, seed=6 + form, **base))
        rows.append(_row("leaf2", cam="lens", s=TWO_LEAVES, seed=7, **{**base, "w": W, "h": H}))
    return rows


ROWS = _materials_frame_rows() + _environment_frame_rows() + _film_rows() + _paths_rows() + _features_rows()
CARRIERS = [r for r in ROWS if r["var"] == "carrier"]


def claimed_dispatches():
    """The material kernels the GPU test below launches, in order, by the rows' own claim: a grid row launches again without its grid
    (the tile form's kernel), a film row two passes.  profiles/kernel_coverage.py --rows holds a kernel trace of the file to this list."""
    out = []
    for r in ROWS:
        for grid in ((True, False) if r["grid"] else (False,)):
            k = mat_kernel(r["entry"], NS[r["scene"]], grid, r["mode"], r["s"], r["gloss"], r["cam"] is not None, r["env"] is not None)[1]
            out += [k] * (2 if r["entry"] == "film" else 1)
    return out


def _template(r):
    return r["kernel"].split("<")[0]


def _form(r):
    return 0 if NS[r["scene"]] == 8 else (2 if r["grid"] else 1)


# ---- CPU: the rows ---------------------------------------------------------------------------------------------------------------------
def test_rows_are_well_formed():
    ids = [r["id"] for r in ROWS]
    assert len(ids) == len(set(ids))
    # every kernel: exactly one carrier, which is a whole frame at an odd depth >= 3 without roulette, and an rr row at an even depth
    kernels = sorted({(r["co"], r["kernel"]) for r in ROWS})
    assert len(kernels) == sum(COUNTS.values()) == 138
    for key in kernels:
        kr = [r for r in ROWS if (r["co"], r["kernel"]) == key]
        car = [r for r in kr if r["var"] == "carrier"]
        assert len(car) == 1 and car[0]["depth"] >= 3 and car[0]["depth"] % 2 == 1 and not car[0]["rr"] and car[0]["range"] is None, key
        assert car[0]["paths"] == "whole" and car[0]["u8"] == "whole", key
        if key[0] != "features":
            assert any(r["rr"] and r["depth"] >= 2 and r["depth"] % 2 == 0 for r in kr), key
        assert all(r["group"] == int(key[1].split(", ")[1][:-1]) for r in kr if _template(r) == "render_frame_mat_kernel"), key
        # M1: the samples of a kernel's rows are its GROUP's
        assert all(r["s"] in M1[r["group"]] + (TWO_LEAVES,) for r in kr), key
    # per family (code object, kernel template): every class of the module docstring
    families = sorted({(r["co"], _template(r)) for r in ROWS})
    assert len(families) == 6
    for fam in families:
        fr_ = [r for r in ROWS if (r["co"], _template(r)) == fam]
        co, tmpl = fam
        assert {r["s"] for r in fr_} >= ({1, 3, 7, 8, 13, 16} if tmpl != "render_paths_mat_kernel" else {3}), fam                          # M1
        assert {_form(r) for r in fr_} == {0, 1, 2}, fam
        if tmpl == "features_kernel":
            assert {r["cam"] for r in fr_} == {None, "pin", "lens"} and any(r["range"] for r in fr_) and any(r["s"] == TWO_LEAVES for r in fr_)
            continue
        assert {0, 1} <= {r["depth"] for r in fr_} and any(r["rr"] for r in fr_), fam                                                      # M3
        assert {r["mode"] for r in fr_} == set(MODES), fam                                                                                 # M4
        if co in ("materials", "film"):
            assert any(r["mode"] == "nee" and r["scene"].endswith("-lamp") for r in fr_), fam
        if co == "environment":                                                                                                            # M5
            assert {(r["env"], r["gloss"]) for r in fr_} == {(e, g) for e in ("sun", "nosun") for g in (False, True)}, fam
        if co == "film":
            assert {r["env"] for r in fr_} == {None, "sun", "nosun"}, fam
        if tmpl == "render_frame_mat_kernel":
            assert {r["cam"] for r in fr_} == {None, "pin", "lens"}, fam                                                                   # M6
            for form in (0, 1, 2):
                ff = [r for r in fr_ if _form(r) == form]
                assert any(r["s"] == TWO_LEAVES and r["group"] == 8 for r in ff), (fam, form)                                              # M1
                for group in (1, 8):                                                                                                       # M2
                    fg = [r for r in ff if r["group"] == group]
                    assert any(r["range"] and r["range"][0] % 2 and r["range"][1] % (64 if group == 1 else 8) for r in fg), (fam, form, group)
                    if co != "film":
                        assert {r["u8"] for r in fg if r["range"]} == set(U8_FORMS) and any(r["u8"] == "whole" and not r["range"] for r in fg), (fam, form, group)
        else:
            assert {r["paths"] for r in fr_} == {"whole"} | set(PATH_FORMS), fam                                                           # M2
    # M6 on every camera kernel of materials.hip: both cameras
    for key in kernels:
        kr = [r for r in ROWS if (r["co"], r["kernel"]) == key]
        if key[0] == "materials" and _template(kr[0]) == "render_frame_mat_kernel" and int(key[1].split("<")[1].split(",")[0]) & 16:
            assert {"pin", "lens"} <= {r["cam"] for r in kr}, key
    assert {r["mode"] for r in ROWS if r["accel8"]} == set(MODES)
    # the big scene only where two LDS tiles or binned spheres are the point
    assert sum(NS[r["scene"]] == 1030 for r in ROWS) == 6


@needs_hipcc
def test_every_material_kernel_of_the_code_objects_has_a_row():
    """Kernel names only: no instruction is looked at."""
    other = set()
    for co, count in COUNTS.items():
        names = code_object_kernels(co)
        render = {n for n in names if n.startswith(("render_frame_mat_kernel", "render_paths_mat_kernel", "features_kernel"))}
        other |= names - render
        rowset = {r["kernel"] for r in ROWS if r["co"] == co}
        assert render == rowset, (co, {"without a row": sorted(render - rowset), "rows naming no kernel": sorted(rowset - render)})
        assert len(render) == count, co
    assert other == NOT_RENDER_KERNELS, "a kernel that is neither a render kernel nor in the exclusion list"


# ---- what a row expects: the restatements ------------------------------------------------------------------------------------------------
def _camera(pkg, r, aperture=None):
    """aperture: instead of the lens's own."""
    if r["cam"] is None:
        return None
    if r["cam"] == "lens" and aperture is None:
        return inside_lens(pkg, r["w"], r["h"])
    return inside_pinhole(pkg, r["w"], r["h"], aperture=aperture or 0.0)


def _env(pkg, r):
    return None if r["env"] is None else sky_and_sun(pkg, r["env"] == "sun")


def _params(sc, r, grid=False, **kw):
    """grid=False: what the restatements read (they know no grid, and the host half of a Scene has no device)."""
    assert sc.ns == NS[r["scene"]] and sc.mat_flags == sc.apt.APT_FLAG_GLOSS
    return sc.params(r["w"], r["h"], r["s"], r["depth"], mode=r["mode"], rr=r["rr"], seed=r["seed"], grid=grid, gloss=r["gloss"], **kw)


def _trace_pixels(sc, p, r, cam, env, seed, b, c):
    """materials_ref.trace over the paths of pixels [b, b + c) alone -> (L [3][all paths], zero outside the range; the range's segments)."""
    q = oracle_params(p)
    rays = rays_of(q, cam, seed)
    lo, hi = b * 4 * q.samples, (b + c) * 4 * q.samples
    part, bad, seg = mr.trace_params(q, rays[:, lo:hi], sc.sph, sc.mat if r["gloss"] else sc.plain, None if env is None else mr.Env.from_ctypes(env),
                                     sc.table if r["mode"] == "table" else None, paths=np.arange(lo, hi, dtype=U), seed=seed)
    assert not bad.any()
    L = np.zeros((3, rays.shape[1]), dtype=F)
    L[:, lo:hi] = part
    return L, seg


_WANT = {}


def want(pkg, r, **change):
    """The restatement of row `r` (with `change`: of the row with these fields changed), computed once:
    frame (fb, u8, segments); film ([planes of pass 0, of pass 1], [segments]); features planes; paths (L of the range, segments)."""
    r = {**r, **change}
    aperture = r.pop("aperture", None)
    one_light = r.pop("one_light", False)
    key = (r["id"], tuple(sorted(change.items())))
    if key in _WANT:
        return _WANT[key]
    from oracle import oracle
    sc = scene(pkg, r["scene"])
    if one_light:                                                             # the same scene, its table listing the first light alone
        sc = Scene(pkg, sc.sph, sc.mat, sc.ns, sc.lights[:1], sc.light)
    cam = _camera(pkg, r, aperture)
    env = _env(pkg, r)
    p = _params(sc, r)
    w, h, s_ = r["w"], r["h"], r["s"]
    b, c = r["range"] or (0, w * h)
    if r["entry"] == "frame":
        if r["range"] is None:
            out = sc.frame_ref(p, r["mode"], cam, env, r["gloss"])
        else:
            L, seg = _trace_pixels(sc, p, r, cam, env, p.seed, b, c)
            _, fb, u8 = oracle.decode_color(L, w, h, s_)
            out = (fb[:, b:b + c], u8[b:b + c], seg)
    elif r["entry"] == "film":
        planes, segs = [], []
        for k in (0, 1):
            seed = fr.pass_seed(p.seed, k)
            L, seg = _trace_pixels(sc, p, r, cam, env, seed, b, c)
            pre = oracle.decode_color(L, w, h, s_)[0]                         # float64 [W * H][3]: the mean before the clip
            assert pre.dtype == np.float64
            planes.append(np.ascontiguousarray(pre.T).astype(F)[:, b:b + c])
            segs.append(seg)
        out = (planes, segs)
    elif r["entry"] == "features":
        rec = cr.default_record(w, h) if cam is None else cr.from_ctypes(cam)
        out = ft.planes(rec, w, h, s_, p.seed, sc.sph, sc.ns, p.eps, b, c)
    else:
        n = w * h * 4 * s_
        pb, pc = _path_range(r, n)
        q = oracle_params(p)
        rays = rays_of(q, None, q.seed)
        L, bad, seg = mr.trace_params(q, rays[:, pb:pb + pc], sc.sph, sc.mat if r["gloss"] else sc.plain, None if env is None else mr.Env.from_ctypes(env),
                                      sc.table if r["mode"] == "table" else None, paths=np.arange(pb, pb + pc, dtype=U))
        assert not bad.any()
        out = (L, seg)
    _WANT[key] = out
    return out


def _path_range(r, n):
    """-> (path_begin, the count the launch covers)"""
    if r["paths"] == "whole":
        return 0, n
    _, pb, pc = r["paths"]
    return pb, pc or n - pb


def _image(r, w):
    """The planes of a row's expectation that the carrier conditions look at: [planes][pixels or paths]."""
    return {"frame": lambda: w[0], "film": lambda: w[0][0], "features": lambda: w, "paths": lambda: w[0]}[r["entry"]]()


def _pixels(r, img):
    """-> per pixel, whether the expectation is non-zero there.  A buffer row has no fb: its paths are the frame's, 4 * S consecutive
    ones per pixel, and a pixel is non-zero when one of its paths is -- what the decode would make of them."""
    nz = (img != 0).any(axis=0)
    return nz.reshape(-1, 4 * r["s"]).any(axis=1) if r["entry"] == "paths" else nz


def test_carrier_rows_would_show_a_failure(host):
    """On the restatement alone, for the carrier of every kernel: the expected image is non-trivial -- at least half of its pixels
    non-zero, at least 64 distinct values -- and sensitive to the row's own axes: it differs in bits from the restatement of the
    neighbouring instantiation, or of the launch whose data did not reach the kernel."""
    t0 = time.time()
    for r in CARRIERS:
        img = _image(r, want(host, r))
        nonzero = float(_pixels(r, img).mean())
        assert nonzero >= 0.5 and np.unique(img).size >= 64, (r["id"], nonzero, np.unique(img).size)
        others = {}
        if r["co"] == "materials" and r["gloss"]:
            others["the gloss words read as mirrors"] = dict(gloss=False)
        if r["cam"]:
            others["without the camera"] = dict(cam=None)
        if r["cam"] == "lens":
            others["the aperture 0"] = dict(aperture=0.0)
        if r["mode"] == "nee":
            others["NEE off"] = dict(mode="plain")
        if r["mode"] == "table":
            others["the one-light table"] = dict(one_light=True)
        if r["env"]:
            others["without the environment"] = dict(env=None)
        if r["entry"] == "features":
            assert others
        for what, change in others.items():
            assert not bits_equal(img, _image(r, want(host, r, **change))), (r["id"], what)
        if r["entry"] == "film":
            planes = want(host, r)[0]
            assert not bits_equal(fr.accumulate(planes), fr.accumulate([planes[0], planes[0]])), r["id"]
    print("carrier conditions: %d rows, %.1f s" % (len(CARRIERS), time.time() - t0))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
GUARD, FILL, BYTE = 64, -9.0, 0xA5


def _guarded(planes, c, inside=FILL):
    """A [planes][c] float32 tensor inside guard values -> (the allocation, the view)."""
    import torch
    block = torch.full((GUARD + planes * c + GUARD,), FILL, dtype=torch.float32, device="cuda")
    block[GUARD:GUARD + planes * c] = inside
    return block, block[GUARD:GUARD + planes * c].view(planes, c)


def _unguard(block, planes, c):
    host_ = block.cpu().numpy()
    assert (host_[:GUARD] == FILL).all() and (host_[GUARD + planes * c:] == FILL).all(), "written outside the band"
    return host_[GUARD:GUARD + planes * c].reshape(planes, c).copy()


def _launch_frame(apt, sc, r, grid):
    """-> (fb, u8 or None, segments traced): band-relative output inside guards, the byte frame in the row's form."""
    import torch
    p = _params(sc, r, grid)
    if r["accel8"]:                                                           # a vouched grid of another scene: not read
        p.accel, p.flags = scene(apt, "gloss9-stock").grid.data_ptr(), p.flags | apt.APT_FLAG_GRID_SLOTS
    b, c = r["range"] or (0, r["w"] * r["h"])
    block, fb = _guarded(3, c)
    raw = torch.full((16 + 3 * c + 16,), BYTE, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 4 == 0
    off = 17 if r["u8"] == "mis" else 16
    u8 = None if r["u8"] == "null" else raw[off:off + 3 * c].view(c, 3)
    mat = sc.d_mat if r["gloss"] else sc.d_plain
    table = sc.d_table if r["mode"] == "table" else None
    if u8 is None:                                                            # the C entries themselves: fb_u8 NULL
        L = apt._lib.lib()
        args = (ctypes.byref(p), None, ctypes.c_void_p(sc.d_sph.data_ptr()), ctypes.c_void_p(mat.data_ptr()))
        tail = (ctypes.c_uint64(b), ctypes.c_uint64(c), ctypes.c_void_p(fb.data_ptr()), None)

        def fn():
            rc = L.apt_render_frame_lights(*args, ctypes.c_void_p(table.data_ptr()), *tail) if table is not None else L.apt_render_frame_materials(*args, *tail)
            assert rc == 0, L.apt_last_error()
    else:
        def fn():
            apt.render.render_frame(p, sc.d_sph, pixel_begin=b, pixel_count=c, fb=fb, fb_u8=u8, materials=mat, lights=table)
    _, traced = sc._launch(_camera(apt, r), _env(apt, r), True, True, fn)
    hb = raw.cpu().numpy()
    assert (hb[:off] == BYTE).all() and (hb[off + (0 if u8 is None else 3 * c):] == BYTE).all(), "bytes written outside the byte frame"
    return _unguard(block, 3, c), None if u8 is None else hb[off:off + 3 * c].reshape(c, 3), traced


def _launch_film(apt, sc, r, grid):
    """-> ([the film after pass 0, after pass 1], [segments traced per pass]): pass 0 stores over NaN."""
    p = _params(sc, r, grid)
    b, c = r["range"] or (0, r["w"] * r["h"])
    block, film = _guarded(3, c, inside=float("nan"))
    snaps, traced = [], []
    for k in (0, 1):
        _, seg = sc._launch(_camera(apt, r), _env(apt, r), True, True, lambda: apt.render.render_frame_film(
            p, sc.d_sph, sc.d_mat if r["gloss"] else sc.d_plain, film=film, pass_index=k, lights=sc.d_table if r["mode"] == "table" else None,
            pixel_begin=b, pixel_count=c))
        snaps.append(_unguard(block, 3, c))
        traced.append(seg)
    return snaps, traced


def _launch_features(apt, sc, r, grid):
    p = _params(sc, r, grid)
    b, c = r["range"] or (0, r["w"] * r["h"])
    block, buf = _guarded(8, c, inside=float("nan"))
    sc.features(p, _camera(apt, r), features=buf, pixel_begin=b, pixel_count=c)
    return _unguard(block, 8, c)


def _launch_paths(apt, sc, r, grid):
    """-> (colours of the range [3][count], segments traced); whole buffers: nothing written outside the range."""
    import torch
    from oracle import oracle
    n = r["w"] * r["h"] * 4 * r["s"]
    pb, pc = _path_range(r, n)
    band = r["paths"] != "whole" and r["paths"][0].startswith("band")
    kw = {} if r["paths"] == "whole" else dict(path_begin=pb, path_count=r["paths"][2])
    p = _params(sc, r, grid, flags=apt.APT_FLAG_BAND_BUFFERS if band else 0, **kw)
    rays = oracle.gen_rays_counter(oracle_params(_params(sc, r)))
    m = pc if band else n
    d_rays = dev((rays[:, pb:pb + pc] if band else rays).ravel())
    colors = torch.full((3 * m,), -7.0, dtype=torch.float32, device="cuda")
    _, traced = sc._launch(None, _env(apt, r), True, True, lambda: apt.render.render_do_ex(
        p, None, d_rays, sc.d_sph, colors, materials=sc.d_mat if r["gloss"] else sc.d_plain, lights=sc.d_table if r["mode"] == "table" else None))
    got = colors.cpu().numpy().reshape(3, m)
    if band:
        return got, traced
    assert (got[:, :pb] == -7.0).all() and (got[:, pb + pc:] == -7.0).all(), "written outside the path range"
    return got[:, pb:pb + pc], traced


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_material_kernel_equals_the_restatement(apt, row):
    r = row
    sc = scene(apt, r["scene"])
    w = want(apt, r)
    for grid in ((True, False) if r["grid"] else (False,)):                   # a grid row: the same launch without it, held to the same
        if r["entry"] == "frame":
            fb, u8, traced = _launch_frame(apt, sc, r, grid)
            assert_bits_equal(fb, w[0])
            assert u8 is None or np.array_equal(u8, w[1]), r["id"]
            assert traced == w[2], (r["id"], traced, w[2])
        elif r["entry"] == "film":
            snaps, traced = _launch_film(apt, sc, r, grid)
            assert_bits_equal(snaps[0], w[0][0])
            assert_bits_equal(snaps[1], fr.accumulate(w[0]))
            assert traced == w[1], (r["id"], traced, w[1])
        elif r["entry"] == "features":
            assert_bits_equal(_launch_features(apt, sc, r, grid), w)
        else:
            got, traced = _launch_paths(apt, sc, r, grid)
            assert_bits_equal(got, w[0])
            assert traced == w[1], (r["id"], traced, w[1])
