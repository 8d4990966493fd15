"""Every render kernel instantiation of the library, each reached through the entry point and the parameters that select it, against the
CPU oracle run with the row's own flags, bit for bit (NaN on both sides counts as equal; fb_u8 exactly).  The rows are generated below: for
every arm and both arithmetic modes, the numeric edges that apply to it --

  E1  eps outside the root-key range (0 < eps < 1e20): 0, -1, 1e21 and NaN (the exact fallback of every fast kernel; grid routing)
  E2  APT_FLAG_EMISSION with a coloured light
  E3  negative, -0, +inf and NaN albedos next to zero albedos, without roulette, in a scene whose back wall has radius 2^31: |hit - centre|
      then lies beyond the fast sequences' range (len2 <= 2^58, pt_trace.h kFastMin), so that the fast kernels really request exact
      re-runs.  (A wall of radius 2^41 is never hit from inside the room: in fp32 its c = |o - centre|^2 - r^2 rounds to 0.)
  E4  depth 0, 1 and odd depths >= 3 (the odd tail of the two-bounce loops)
  E5  buffer arms: the degenerate ray set (NaN / inf / zero directions, all-miss rays) at both halves of a lane pair, in every run of a
      render_paths2_kernel thread, in a partial last run without a B half; path ranges and band-relative buffers
  E6  frame arms: sample counts on both sides of 8 and 16, a count with two pairwise leaves (136), a pixel sub-range with an odd start

The CPU test checks that the rows name exactly the render kernels the code object holds, so that a kernel added later without a row fails
the CPU suite."""
import ctypes

import numpy as np
import pytest

from mat_rows import code_object_kernels, needs_hipcc

K, O = 0, 1
RETIRE, RR, EMISSION, BAND, GRID_SLOTS = 1, 2, 4, 8, 16
E1_EPS = (0.0, -1.0, 1e21, float("nan"))
TWO_PATH_MIN = 1 << 20                       # render_kernels.hip kTwoPathBufferMin
BLOCK, PAIRS = 256, 2                        # kBlock, kPaths2Pairs (pt_kernels.h): a run of render_paths2_kernel is 2 * kBlock paths
BIG_W, BIG_H = 512, 520                      # 1 064 960 paths, S = 1
GRID_NS, TILE_NS = 300, 40

# kernels of the code object that are not render kernels (no row needed)
NOT_RENDER_KERNELS = {
    "decode_color_kernel", "decode_color_kernel4", "decode_color_kernel8", "gen_rays_kernel", "gen_rays_mt_kernel",
    "grid_classify_kernel", "grid_count_kernel", "grid_fill_kernel", "grid_geom_kernel", "grid_slots_kernel", "grid_sort_cells_kernel",
    "scan_add_kernel", "scan_blocks_kernel", "scan_sums_kernel", "selftest_div3_kernel", "selftest_sqrt_kernel", "test_scene_kernel",
}


def _b(v):
    return "true" if v else "false"


# ---- the rows --------------------------------------------------------------------------------------------------------------------------
# A row: kernel (as the ISA names it), entry ("paths" / "frame" / "mt"), mode, scene, depth, eps, flags, and the entry's own parameters.
# Variants: e1 (eps out of range, odd depth), emit (coloured light, depth 1), neg / nonfinite (E3, odd depths), d0 (depth 0).
def _variants(mode, arm, depth0=True, e1=True, scene8=True):
    """The edge variants of one arm in one mode.  `arm` (an index) rotates the E1 value, so that every value meets several arms."""
    sc = (lambda k: k) if scene8 else (lambda k: "grid_" + k if k != "ref" else "grid")
    v = []
    if e1:
        v.append(dict(var="e1", scene=sc("ref"), depth=5, eps=E1_EPS[(arm + mode) % 4], flags=0))
    v.append(dict(var="emit", scene=sc("emit"), depth=1, eps=1e-4, flags=EMISSION))
    v.append(dict(var="neg", scene=sc("neg"), depth=3, eps=1e-4, flags=0, reruns=scene8))
    v.append(dict(var="nonfinite", scene=sc("nonfinite"), depth=7, eps=1e-4, flags=0, reruns=scene8))
    if depth0:
        v.append(dict(var="d0", scene=sc("ref"), depth=0, eps=1e-4, flags=0))
    return v


def _buffer_rows():
    rows = []
    arm = 0
    for m in (K, O):
        # render_paths2_kernel: the reference-sized scene, no RETIRE / RR, >= 2^20 paths.  Ranges: the whole image, an odd range whose last
        # run has no B half, band-relative buffers (path_count 0 with path_begin > 0 among them)
        ranges = [(0, 0, False), (3, TWO_PATH_MIN + 100, False), (1000, 0, True), (5, TWO_PATH_MIN + 7, True), (2, TWO_PATH_MIN + 300, False)]
        for i, v in enumerate(_variants(m, arm)):
            b, c, band = ranges[i % len(ranges)]
            v["reruns"] = v.get("reruns", False)
            rows.append(dict(kernel=f"render_paths2_kernel<{m}>", entry="paths", mode=m, w=BIG_W, h=BIG_H, s=1, path_begin=b, path_count=c,
                             band=band, **{**v, "flags": v["flags"] | (BAND if band else 0)}))
        arm += 1
        # small ranges of the 8-sphere scene: the queue kernel (RETIRE, with and without RR) and the one-path kernel (with RR or not)
        small = [(0, 0, False), (7, 3001, False), (129, 0, True), (64, 1500, True), (1, 4000, False)]
        for kern, extra in ((f"render_paths_queue_kernel<{m}>", RETIRE), (f"render_paths_kernel<{m}, 0, false>", 0)):
            for i, v in enumerate(_variants(m, arm)):
                b, c, band = small[i % len(small)]
                fl = v["flags"] | extra | (BAND if band else 0) | (RR if i == 0 else 0)
                # (render_paths_queue_kernel keeps no exact re-run statistic)
                rows.append(dict(kernel=kern, entry="paths", mode=m, w=16, h=16, s=4, path_begin=b, path_count=c, band=band,
                                 **{**v, "flags": fl, "reruns": v.get("reruns", False) and extra != RETIRE}))
            arm += 1
        # any other scene: LDS tiles (no accel) and the grid walk (accel), with and without RETIRE
        for sc_i, kind in ((1, "tiles"), (2, "grid")):
            for rt in (False, True):
                for i, v in enumerate(_variants(m, arm, scene8=False)):
                    b, c, band = small[i % len(small)]
                    fl = v["flags"] | (RETIRE if rt else 0) | (BAND if band else 0)
                    scene = v["scene"] if kind == "grid" else v["scene"].replace("grid", "tiles")
                    rows.append(dict(kernel=f"render_paths_kernel<{m}, {sc_i}, {_b(rt)}>", entry="paths", mode=m, w=16, h=16, s=4,
                                     path_begin=b, path_count=c, band=band, accel="grid" if kind == "grid" else None,
                                     **{**v, "flags": fl, "scene": scene}))
                arm += 1
    return rows


# E6 frame shapes: (samples, pixel_begin, pixel_count) on a 9 x 7 frame; None = the whole frame
def _shapes(samples):
    out = []
    for i, s in enumerate(samples):
        out.append((s, None) if i % 2 == 0 else (s, (5, 23)))   # odd start, a partial last wave / workgroup
    return out


def _frame_rows():
    rows = []
    arm = 100
    for m in (K, O):
        def add(kernel, samples, extra=0, depth0=True, e1=True, scene8=True, accel=None, counter=False, knob=None):
            nonlocal arm
            sh = _shapes(samples)
            for i, v in enumerate(_variants(m, arm, depth0=depth0, e1=e1, scene8=scene8)):
                s, rng = sh[i % len(sh)]
                scene = v["scene"] if scene8 or accel else v["scene"].replace("grid", "tiles")
                rows.append(dict(kernel=kernel, entry="frame", mode=m, w=9, h=7, s=s, range=rng, accel=accel, counter=counter or v.get("reruns", False) and scene8,
                                 knob=knob, **{**v, "flags": v["flags"] | extra, "scene": scene}))
            arm += 1

        # 8-sphere scene
        for rr in (False, True):
            add(f"render_frame_queue8_kernel<{m}, {_b(rr)}, 0, false>", (8, 136, 15, 16), RETIRE | (RR if rr else 0), depth0=False)
        add(f"render_frame_kernel<{m}, 0, 8, false, true>", (16, 136, 17, 64))
        add(f"render_frame_kernel<{m}, 0, 8, false, false>", (8, 15, 12, 9))
        add(f"render_frame_kernel<{m}, 0, 8, false, false>", (16, 136), RR)                    # roulette without RETIRE
        # RETIRE at depth 0: the sample-queue kernel is not launched, nothing to retire
        rows.append(dict(kernel=f"render_frame_kernel<{m}, 0, 8, false, false>", entry="frame", mode=m, w=9, h=7, s=16, range=(5, 23),
                         accel=None, counter=False, knob=None, var="d0_retire", scene="emit", depth=0, eps=1e-4, flags=RETIRE | EMISSION))
        for rt in (False, True):
            add(f"render_frame_kernel<{m}, 0, 1, {_b(rt)}, false>", (7, 1, 4, 7), RETIRE if rt else 0)
        # LDS tiles
        for g in (1, 8):
            for rt in (False, True):
                add(f"render_frame_kernel<{m}, 1, {g}, {_b(rt)}, false>", (7, 3, 1) if g == 1 else (8, 15, 16, 136), RETIRE if rt else 0, scene8=False)
        # the grid: the sample-queue kernel's grid form (eps in range, depth > 0, S >= 8), with and without a TraceCounter (STATS)
        for rr in (False, True):
            for stats in (False, True):
                add(f"render_frame_queue8_kernel<{m}, {_b(rr)}, 2, {_b(stats)}>", (8, 136, 15, 16), (RETIRE if stats else 0) | (RR if rr else 0),
                    depth0=False, e1=False, scene8=False, accel="grid", counter=stats)
        # render_frame_kernel's grid walk: S < 8; S >= 8 through eps out of range, a grid without slot tables, the grid_walk knob, depth 0
        for rt in (False, True):
            add(f"render_frame_kernel<{m}, 2, 1, {_b(rt)}, false>", (7, 2, 1), RETIRE if rt else 0, scene8=False, accel="grid")
            fl = RETIRE if rt else 0
            k8 = f"render_frame_kernel<{m}, 2, 8, {_b(rt)}, false>"
            for i, eps in enumerate(E1_EPS):      # eps out of range: the queue kernel returns at once, this one renders (vouched or not)
                rows.append(dict(kernel=k8, entry="frame", mode=m, w=9, h=7, s=(8, 16, 15, 136)[i], range=(5, 23) if i % 2 else None,
                                 accel="grid", counter=i == 3, knob=None, var=f"e1_{i}", scene="grid", depth=5, eps=eps,
                                 flags=fl | (GRID_SLOTS if i in (0, 2) else 0)))
            add(k8, (8, 136), fl, e1=False, scene8=False, accel="bare")
            add(k8, (16, 15), fl, e1=False, depth0=False, scene8=False, accel="grid", knob=("grid_walk", 1))
    return rows


def _mt_rows():
    rows = []
    arm = 200
    for m in (K, O):
        for kern, samples in ((f"render_frame_mt_kernel<{m}>", (8, 16, 32, 8, 256)), (f"render_frame_mt_any_kernel<{m}>", (7, 136, 1, 20, 3))):
            for i, v in enumerate(_variants(m, arm)):
                rng = None if i % 2 == 0 else (41, 100)       # an odd start inside a 78-pixel group, the end inside another
                rows.append(dict(kernel=kern, entry="mt", mode=m, w=23, h=11, s=samples[i], range=rng, counter=v.get("reruns", False), **v))
            arm += 1
    return rows


def _rows():
    rows = _buffer_rows() + _frame_rows() + _mt_rows()
    for r in rows:
        eps = "nan" if r["eps"] != r["eps"] else f"{r['eps']:g}"
        r["id"] = f"{r['kernel']}|{'KO'[r['mode']]}|{r['var']}|s{r['s']}|d{r['depth']}|eps{eps}|f{r['flags']}"
        if r["entry"] == "paths":
            r["id"] += f"|b{r['path_begin']}c{r['path_count']}"
        elif r["range"]:
            r["id"] += f"|px{r['range'][0]}+{r['range'][1]}"
        if r.get("accel"):
            r["id"] += "|" + r["accel"]
        if r.get("knob"):
            r["id"] += "|" + r["knob"][0]
    return rows


ROWS = _rows()


# ---- CPU: the rows cover the code object ---------------------------------------------------------------------------------------------
def test_rows_are_well_formed():
    ids = [r["id"] for r in ROWS]
    assert len(ids) == len(set(ids))
    for r in ROWS:
        if r["kernel"].startswith("render_paths2_kernel"):
            n = r["w"] * r["h"] * 4 * r["s"]
            assert (r["path_count"] or n - r["path_begin"]) >= TWO_PATH_MIN, r["id"]
    # every edge value and depth class appears on every kernel family in both modes
    for fam in ("render_paths2_kernel", "render_paths_queue_kernel", "render_paths_kernel", "render_frame_queue8_kernel", "render_frame_kernel",
                "render_frame_mt_kernel", "render_frame_mt_any_kernel"):
        for m in (K, O):
            fr = [r for r in ROWS if r["kernel"].split("<")[0] == fam and r["mode"] == m]
            assert any(r["flags"] & EMISSION for r in fr) and any(r["var"] in ("neg", "nonfinite") for r in fr), (fam, m)
            assert any(r["depth"] == 1 for r in fr) and any(r["depth"] >= 3 and r["depth"] % 2 for r in fr), (fam, m)
            if fam != "render_frame_queue8_kernel":
                assert any(not (0 < r["eps"] < 1e20) for r in fr) and any(r["depth"] == 0 for r in fr), (fam, m)
    assert {("nan" if e != e else e) for e in (r["eps"] for r in ROWS) if not (0 < e < 1e20)} == {0.0, -1.0, 1e21, "nan"}


@needs_hipcc
def test_every_render_kernel_of_the_code_object_has_a_row():
    names = code_object_kernels("render_kernels")
    render = {n for n in names if n.startswith(("render_paths", "render_frame"))}
    assert names - render == NOT_RENDER_KERNELS, "a kernel that is neither a render kernel nor in the exclusion list"
    rowset = {r["kernel"] for r in ROWS}
    assert render == rowset, {"without a row": sorted(render - rowset), "rows naming no kernel": sorted(rowset - render)}
    assert len(render) == 54


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def apt():
    import __graft_entry__ as g
    g.build()                   # a no-op when the in-tree library is current
    import ascendpathtracing_amd as pkg
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    pkg.render, pkg.gen_data = render, gen_data
    return pkg


def _degenerate_rays(k=64, seed=3):
    """tests/test_gpu_parity.py test_degenerate_rays_nan_inf_and_all_miss's set: origin at a sphere centre, zero direction, huge / inf /
    NaN components, rays far outside the room (mostly all-miss)."""
    rng = np.random.RandomState(seed)
    r = np.zeros((6, k), dtype=np.float32)
    r[:3] = rng.uniform(-200, 300, size=(3, k))
    d = rng.normal(size=(3, k))
    r[3:] = d / np.linalg.norm(d, axis=0)
    r[:, 0] = [27, 16.5, 47, 0, 0, 1]
    r[:, 1] = [50, 52, 295.6, 0, 0, 0]
    r[:, 2] = [1e30, 0, 0, 1, 0, 0]
    r[:, 3] = [50, 52, 100, np.inf, 0, 0]
    r[:, 4] = [np.nan, 52, 100, 0, 0, -1]
    r[:, 5] = [50, 52, 100, 1e20, 1e20, 1e20]
    r[:, 6] = [3e38, 3e38, 3e38, -1, 0, 0]
    r[:3, 7:k // 2] *= 1e4
    return r


def _unusual_albedos(alb, kind, idx):
    """alb: [3][Ns] view.  `idx`: five sphere indices -> negative / -0 (neg) or +inf / NaN (nonfinite) components next to zero albedos."""
    a, b, c, z0, z1 = idx
    alb[:, z0] = 0.0
    alb[:, z1] = (0.0, 0.0, 0.0)
    if kind == "neg":
        alb[:, a] = (-0.5, -0.25, -0.75); alb[:, b] = (-0.0, 0.7, -0.0); alb[:, c] = (0.6, -0.9, 0.3)
    else:
        alb[:, a] = (np.inf, 0.5, 0.5); alb[:, b] = (np.nan, 0.75, 0.25); alb[:, c] = (0.5, 0.5, np.inf)


_SCENES = {}


def _scene(apt, key):
    """key -> (numpy table, num_spheres)"""
    if key in _SCENES:
        return _SCENES[key]
    from oracle import oracle
    if key in ("ref", "emit", "neg", "nonfinite"):
        ns, t = 8, oracle.gen_spheres().copy()
        tab = t[:80].reshape(10, 8)
        if key == "emit":
            tab[4:7, 7] = (20.0, 7.5, 0.25)
        elif key != "ref":
            # the back wall becomes a sphere of radius 2^31 (r2 = 2^62): |hit - centre| lies beyond the fast sequences' 2^29
            tab[0, 2] = np.float32(2.0 ** 62)
            tab[3, 2] = np.float32(2.0 ** 31)
            _unusual_albedos(tab[7:10], key, (1, 2, 6, 3, 0))
    else:
        kind, rest = key.split("_", 1) if "_" in key else (key, "ref")
        ns = GRID_NS if kind == "grid" else TILE_NS
        t = oracle.gen_scene(ns, seed=7).copy()
        tab = t[:10 * ns].reshape(10, ns)
        if rest == "emit":
            tab[4:7, ns - 1] = (20.0, 7.5, 0.25)
        elif rest in ("neg", "nonfinite"):
            _unusual_albedos(tab[7:10], rest, (0, 1, 12, 2, 20))
            tab[7:10, 25:35] = -0.5 if rest == "neg" else np.nan
    _SCENES[key] = (t, ns)
    return _SCENES[key]


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    ok = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    return bool(ok.all()), np.argwhere(~ok)[:5]


def _oracle_params(oracle, r, ns, **kw):
    return oracle.make_params(r["w"], r["h"], r["s"], depth=r["depth"], num_spheres=ns, eps=r["eps"], mode=r["mode"],
                              flags=r["flags"] & (RETIRE | RR | EMISSION), seed=9, rr_start=2, **kw)


def _apt_params(apt, r, ns, **kw):
    return apt.make_params(r["w"], r["h"], r["s"], depth=r["depth"], num_spheres=ns, eps=r["eps"], mode=r["mode"], flags=r["flags"],
                           seed=9, rr_start=2, **kw)


_GRIDS = {}


def _accel(apt, r, scene, ns):
    import torch
    if not r.get("accel"):
        return 0, None
    key = (r["scene"], r["accel"])
    if key not in _GRIDS:
        g = torch.from_numpy(apt.gen_data.build_grid(scene, ns).view(np.int32)).cuda()
        assert int(g[26]) != 0                  # off_cellslot: the grid carries the pair-slot tables
        if r["accel"] == "bare":
            g[26] = 0
        _GRIDS[key] = g
    return _GRIDS[key].data_ptr(), _GRIDS[key]


def _run_paths(apt, oracle, r, scene, ns, d_scene):
    import torch
    n = r["w"] * r["h"] * 4 * r["s"]
    b, c = r["path_begin"], r["path_count"] or n - r["path_begin"]
    rays = oracle.gen_rays_counter(oracle.make_params(r["w"], r["h"], r["s"], seed=5)).copy()
    deg = _degenerate_rays()
    k = deg.shape[1]
    if c >= TWO_PATH_MIN:
        # lane pairs of render_paths2_kernel: both halves of a run, in every run of a thread, and the partial last run (no B half)
        offs = [0, BLOCK]
        offs += [it * 2 * BLOCK + 100 + h * BLOCK for it in range(1, PAIRS) for h in (0, 1)]
        offs += [(c // (2 * BLOCK)) * 2 * BLOCK]                      # the start of the last (partial) run
        offs += [c - k]
    else:
        offs = [0, c // 2 - k // 2, c - k]
    for o in offs:
        kk = max(0, min(k, c - o))
        rays[:, b + o:b + o + kk] = deg[:, :kk]
    accel, _keep = _accel(apt, r, scene, ns)
    p = _apt_params(apt, r, ns, path_begin=b, path_count=r["path_count"], accel=accel)
    want, _ = oracle.render_paths(_oracle_params(oracle, r, ns, path_begin=b, path_count=r["path_count"]), rays, scene,
                                  threads=oracle.max_threads())
    with apt.render.TraceCounter() as tc:
        if r["band"]:
            d_rays = torch.from_numpy(np.ascontiguousarray(rays[:, b:b + c])).cuda().reshape(-1)
            col = torch.full((3 * c,), -7.0, device="cuda")
            apt.render.render_do_ex(p, None, d_rays, d_scene, col)
            got = col.view(3, c).cpu().numpy()
        else:
            col = torch.full((3 * n,), -7.0, device="cuda")
            apt.render.render_do_ex(p, None, torch.from_numpy(rays).cuda().reshape(-1), d_scene, col)
            full = col.view(3, n).cpu().numpy()
            assert (full[:, :b] == -7.0).all() and (full[:, b + c:] == -7.0).all(), "written outside the range"
            got = full[:, b:b + c]
    return got, want[:, b:b + c], tc


def _run_frame(apt, oracle, r, scene, ns, d_scene):
    pb, pc = r["range"] or (0, r["w"] * r["h"])
    accel, _keep = _accel(apt, r, scene, ns)
    fb_w, u8_w, _, _ = oracle.render_frame(_oracle_params(oracle, r, ns), scene, pixel_begin=pb, pixel_count=pc, threads=oracle.max_threads())
    p = _apt_params(apt, r, ns, accel=accel)

    def go():
        if r["counter"]:
            with apt.render.TraceCounter() as tc:
                fb, u8 = apt.render.render_frame(p, d_scene, pixel_begin=pb, pixel_count=pc)
            return fb, u8, tc
        fb, u8 = apt.render.render_frame(p, d_scene, pixel_begin=pb, pixel_count=pc)
        return fb, u8, None

    if r["knob"]:
        with apt.render.debug_knob(*r["knob"]):
            fb, u8, tc = go()
    else:
        fb, u8, tc = go()
    import torch
    torch.cuda.synchronize()
    return (fb.cpu().numpy(), u8.cpu().numpy()), (fb_w, u8_w), tc


def _run_mt(apt, oracle, r, scene, d_scene):
    import torch
    from ascendpathtracing_amd import _lib
    w, h, s = r["w"], r["h"], r["s"]
    pb, pc = r["range"] or (0, w * h)
    rays = oracle.gen_rays(w, h, s, seed=0)
    col, _ = oracle.render_paths(oracle.make_params(w, h, s, depth=r["depth"], eps=r["eps"], mode=r["mode"], flags=r["flags"] & EMISSION),
                                 rays, scene, threads=oracle.max_threads())
    _, fb_w, u8_w = oracle.decode_color(col, w, h, s)
    # apt_render_frame_mt through ctypes: render_reference_frame_fused() does not take eps
    ck, g_lo = apt.render.mt_group_checkpoints(w, h, s, 0, pb, pc)
    ck_d = torch.from_numpy(ck.view(np.int32)).cuda()
    p = apt.make_params(w, h, s, depth=r["depth"], eps=r["eps"], mode=r["mode"], flags=r["flags"])
    fb = torch.empty((3, pc), dtype=torch.float32, device="cuda")
    u8 = torch.empty((pc, 3), dtype=torch.uint8, device="cuda")

    def go():
        _lib.check(_lib.lib().apt_render_frame_mt(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream),
                                                  ctypes.c_void_p(ck_d.data_ptr()), ctypes.c_uint64(ck_d.shape[0]), ctypes.c_uint64(g_lo),
                                                  ctypes.c_void_p(d_scene.data_ptr()), ctypes.c_uint64(pb), ctypes.c_uint64(pc),
                                                  ctypes.c_void_p(fb.data_ptr()), ctypes.c_void_p(u8.data_ptr())), "apt_render_frame_mt")

    tc = None
    if r["counter"]:
        with apt.render.TraceCounter() as tc:
            go()
    else:
        go()
    torch.cuda.synchronize()
    return (fb.cpu().numpy(), u8.cpu().numpy()), (fb_w[:, pb:pb + pc], u8_w[pb:pb + pc]), tc


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r["id"] for r in ROWS])
def test_launch_arm_equals_the_oracle(apt, oracle, row):
    import torch
    scene, ns = _scene(apt, row["scene"])
    d_scene = torch.from_numpy(np.ascontiguousarray(scene, dtype=np.float32)).cuda()
    if row["entry"] == "paths":
        got, want, tc = _run_paths(apt, oracle, row, scene, ns, d_scene)
        ok, where = _same(got, want)
        assert ok, (row["id"], where)
    else:
        (fb, u8), (fb_w, u8_w), tc = (_run_frame(apt, oracle, row, scene, ns, d_scene) if row["entry"] == "frame"
                                      else _run_mt(apt, oracle, row, scene, d_scene))
        ok, where = _same(fb, fb_w)
        assert ok, (row["id"], where)
        assert np.array_equal(u8, u8_w), row["id"]
    if row.get("reruns") and 0 < row["eps"] < 1e20 and row["depth"] > 0:
        assert tc is not None and tc.exact_reruns > 0, row["id"]      # the radius-2^41 sphere sends the fast sequences out of range


# ---- the retirement contract ----------------------------------------------------------------------------------------------------------
def _neg_inf_scene(oracle):
    t = oracle.gen_spheres().copy()
    alb = t[56:80].reshape(3, 8)
    alb[:, 2] = (-0.5, -0.25, -0.75)
    alb[:, 1] = (np.inf, 0.5, 0.5)
    return t


def test_retirement_is_not_result_preserving_for_negative_or_infinite_albedos(oracle):
    """include/render_mi355x.h APT_FLAG_RETIRE: results equal the full trace only while every albedo component is finite with a clear sign
    bit.  With a negative albedo 0 * albedo = -0 and with an infinite one NaN, so a path with zero throughput is not finished: the oracle
    with and without FLAG_RETIRE differs here (and agrees on the reference scene)."""
    sph = oracle.gen_spheres()
    t = _neg_inf_scene(oracle)
    for mode in (K, O):
        fa, _, _, _ = oracle.render_frame(oracle.make_params(24, 16, 16, depth=8, mode=mode), t, threads=oracle.max_threads())
        fr, _, _, _ = oracle.render_frame(oracle.make_params(24, 16, 16, depth=8, mode=mode, flags=RETIRE), t, threads=oracle.max_threads())
        assert not _same(fa, fr)[0], mode
        ga, _, _, _ = oracle.render_frame(oracle.make_params(24, 16, 16, depth=8, mode=mode), sph, threads=oracle.max_threads())
        gr, _, _, _ = oracle.render_frame(oracle.make_params(24, 16, 16, depth=8, mode=mode, flags=RETIRE), sph, threads=oracle.max_threads())
        assert _same(ga, gr)[0], mode


@pytest.mark.gpu
def test_retire_and_full_trace_frames_each_equal_their_own_oracle(apt, oracle):
    """On the scene of the test above, a RETIRE frame equals the oracle's RETIRE frame and a full-trace frame the oracle's full trace."""
    import torch
    t = _neg_inf_scene(oracle)
    d = torch.from_numpy(t).cuda()
    for mode in (K, O):
        for s in (8, 16):
            for flags in (0, RETIRE):
                fb, u8 = apt.render.render_frame(apt.make_params(24, 16, s, depth=8, mode=mode, flags=flags), d)
                fb_w, u8_w, _, _ = oracle.render_frame(oracle.make_params(24, 16, s, depth=8, mode=mode, flags=flags), t,
                                                       threads=oracle.max_threads())
                torch.cuda.synchronize()
                assert _same(fb.cpu().numpy(), fb_w)[0] and np.array_equal(u8.cpu().numpy(), u8_w), (mode, s, flags)
