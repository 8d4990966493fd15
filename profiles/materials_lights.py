#!/usr/bin/env python3
"""A light table in the material renderer (the *_lights entries): what it costs and what it buys.  Needs an MI355X (no fallback).

    python profiles/materials_lights.py [--reps 5] [--parent-lib PATH] [--out profiles/materials_lights.jsonl]
    rocprofv3 --kernel-trace --stats -d <dir> -o ml -- python profiles/materials_lights.py --trace     (a run of its own: one frame per shape)
    python profiles/materials_lights.py --kernel-stats <dir>/ml_results.db   (no GPU: that trace -> profiles/materials_lights_kernel_stats.csv)

In the manner of profiles/materials_nee.py, whose six scenes it takes: 1920x1080, depth 8, HIP events around each frame, one warm-up per
shape, all shapes alternated in one process; every line carries all repetitions, their median, minimum and maximum.  Three questions:
  (1) do the plain and the APT_FLAG_NEE frames cost what they cost in the parent commit?  --parent-lib: a librender_mi355x.so built
      from the parent, loaded next to this tree's and timed in the same alternation (the kernels are instruction-identical);
  (2) a one-light table against APT_FLAG_NEE on the same scenes: the price of the per-lane record, the selection and the extra state;
  (3) several lights -- the 8-sphere scene with two lamps, the 10 000-sphere scene through the grid with 16 and with 256 lamps --,
      table launch against plain launch: ms, segments per path, and the per-channel variance ratio of the path radiance at equal
      sample count (2^20 camera rays, buffer mode), from which the equal-time efficiency (variance ratio / time ratio) follows."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402
from materials_nee import kernel_stats  # noqa: E402

W, H, DEPTH = 1920, 1080, 8
NS_BIG, SEED_BIG = 10000, 1
VAR_W, VAR_H, VAR_S = 512, 256, 2            # 2^20 camera rays for the variance ratio


def two_lamps(gen_data):
    """tests/lights_ref.py two_lamps: spheres 6 and 7 of the 8-sphere DIFF scene as lamps of different colour and radius."""
    sph = gen_data.with_lamps(gen_data.gen_spheres(), 8, [6, 7], radius=[4.0, 1.5], centres=[(27.0, 16.5, 47.0), (50.0, 81.6 - 16.5, 81.6)],
                              emission=[(60.0, 30.0, 15.0), 400.0])
    return sph, np.array([1, 1, 1, 1, 1, 1, 1, 1], dtype=np.int32)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(here, "materials_lights.jsonl"))
    ap.add_argument("--parent-lib", help="librender_mi355x.so of the parent commit: its plain and APT_FLAG_NEE frames are timed in the same run")
    ap.add_argument("--trace", action="store_true", help="one warm frame per shape and nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-stats", metavar="DB", help="summarise a rocprofv3 kernel trace (its sqlite output) per kernel and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, os.path.join(os.path.dirname(args.out), "materials_lights_kernel_stats.csv"))
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def scene(sph, mat, light, samples, use_grid, lights):
        ns = int(mat.size)
        table = dev(sph)
        grid = gen_data.build_grid_device(table, ns) if use_grid else None      # from the table it serves
        return dict(sph=table, mat=dev(mat), ns=ns, light=light, samples=samples, grid=grid,
                    gflags=gen_data.grid_flags(grid, ns) if use_grid else 0,
                    lights=dev(gen_data.build_lights(sph, ns, lights).view(np.int32)), nlights=len(lights))

    s8, m8 = gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    s9, m9 = gen_data.gen_spheres_materials()
    sb, mb = gen_data.gen_scene_materials(NS_BIG, seed=SEED_BIG)
    one, many = {}, {}                             # the NEE table's six scenes, their light listed alone; the several-light scenes
    for name, (sph, mat, light, samples, use_grid) in {"diff8": (s8, m8, 7, 64, False), "demo9": (s9, m9, 7, 64, False),
                                                       "grid10k": (sb, mb, NS_BIG - 1, 8, True)}.items():
        for lamp in (False, True):
            one[name + ("_lamp" if lamp else "")] = scene(gen_data.with_lamp(sph, mat.size, light) if lamp else sph, mat, light, samples,
                                                          use_grid, [light])
    many["two8"] = scene(*two_lamps(gen_data), 7, 64, False, [6, 7])
    for n in (16, 256):
        idx = [6 + ((NS_BIG - 7) // n) * i for i in range(n)]
        sph = gen_data.with_lamps(sb, NS_BIG, idx, radius=1.0, emission=[(40.0 + (i % 5) * 20.0, 60.0, 100.0 - (i % 3) * 30.0) for i in range(n)])
        many["grid10k_%dlamps" % n] = scene(sph, mb, NS_BIG - 1, 8, True, idx)

    def params(sc, nee=False, w=W, h=H, samples=None, seed=0):
        return apt.make_params(w, h, samples or sc["samples"], depth=DEPTH, num_spheres=sc["ns"], light_index=sc["light"], seed=seed,
                               accel=sc["grid"].data_ptr() if sc["grid"] is not None else 0,
                               flags=sc["gflags"] | (apt.APT_FLAG_NEE if nee else 0))

    fb_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    u8_buf = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")

    def frame(sc, p, how):
        """how: "plain" / "table" through this build, or a ctypes library (the parent's build, through its C-ABI: the struct is unchanged)."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if isinstance(how, str):
            render.render_frame(p, sc["sph"], fb=fb_buf, fb_u8=u8_buf, materials=sc["mat"], lights=sc["lights"] if how == "table" else None)
        else:
            rc = how.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(sc["sph"].data_ptr()), ctypes.c_void_p(sc["mat"].data_ptr()),
                                                ctypes.c_uint64(0), ctypes.c_uint64(W * H), ctypes.c_void_p(fb_buf.data_ptr()),
                                                ctypes.c_void_p(u8_buf.data_ptr()))
            assert rc == 0, rc
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    shapes = {}
    for name, sc in one.items():
        shapes[name + "_off"] = (sc, params(sc), "plain")
        shapes[name + "_nee"] = (sc, params(sc, True), "plain")
        shapes[name + "_table1"] = (sc, params(sc), "table")
        if parent is not None:
            shapes[name + "_off_parent"] = (sc, params(sc), parent)
            shapes[name + "_nee_parent"] = (sc, params(sc, True), parent)
    for name, sc in many.items():
        shapes[name + "_off"] = (sc, params(sc), "plain")
        shapes[name + "_table"] = (sc, params(sc), "table")
    if args.trace:
        for sc, p, how in shapes.values():
            frame(sc, p, how)
        render.check_device_status()
        return
    times = {k: [] for k in shapes}
    for sc, p, how in shapes.values():               # warm-up: code objects
        frame(sc, p, how)
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, (sc, p, how) in shapes.items():
            times[name].append(round(frame(sc, p, how), 3))
    render.check_device_status()

    def row(name):
        t = times[name]
        return {"shape": name, "frame": f"{W}x{H}", "depth": DEPTH, "samples": shapes[name][1].samples, "ms": t,
                "median_ms": round(statistics.median(t), 3), "min_ms": min(t), "max_ms": max(t)}

    rows = [row(name) for name in shapes]
    med = {r["shape"]: r["median_ms"] for r in rows}

    def segments(name):
        with render.TraceCounter() as tc:
            frame(*shapes[name])
        return tc.value

    for name in one:
        s = {"shape": "summary_" + name, "table1_over_nee": round(med[name + "_table1"] / med[name + "_nee"], 3),
             "nee_over_off": round(med[name + "_nee"] / med[name + "_off"], 3),
             "segments_nee": segments(name + "_nee"), "segments_table1": segments(name + "_table1")}
        if parent is not None:
            for kind in ("off", "nee"):
                a, b = times[name + "_" + kind], times[name + "_" + kind + "_parent"]
                s.update({kind + "_minus_parent_ms": round(med[name + "_" + kind] - med[name + "_" + kind + "_parent"], 3),
                          kind + "_parent_spread_ms": round(max(b) - min(b), 3), kind + "_spread_ms": round(max(a) - min(a), 3)})
        rows.append(s)
    for name, sc in many.items():
        npaths = W * H * 4 * sc["samples"]
        pv = params(sc, w=VAR_W, h=VAR_H, samples=VAR_S, seed=5)
        rays = render.gen_rays_device(pv).reshape(-1)
        on = render.render_paths(pv, rays, sc["sph"], materials=sc["mat"], lights=sc["lights"]).double()
        off = render.render_paths(pv, rays, sc["sph"], materials=sc["mat"]).double()
        torch.cuda.synchronize()
        ratio = (off.var(dim=1) / on.var(dim=1)).tolist()
        t = med[name + "_table"] / med[name + "_off"]
        rows.append({"shape": "summary_" + name, "lights": sc["nlights"], "table_over_off": round(t, 3),
                     "segments_per_path_off": round(segments(name + "_off") / npaths, 3),
                     "segments_per_path_table": round(segments(name + "_table") / npaths, 3),
                     "variance_paths": pv.num_paths, "variance_off_over_table": [round(v, 2) for v in ratio],
                     "mean_off": [round(v, 5) for v in off.mean(dim=1).tolist()], "mean_table": [round(v, 5) for v in on.mean(dim=1).tolist()],
                     "equal_time_efficiency": [round(v / t, 2) for v in ratio]})
    render.check_device_status()
    meta = {"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
            "parent_lib": bool(parent), "scene_grid10k": f"gen_scene_materials({NS_BIG}, seed={SEED_BIG})"}
    with open(args.out, "w") as f:
        for r in rows + [meta]:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
