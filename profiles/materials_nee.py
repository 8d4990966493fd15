#!/usr/bin/env python3
"""Direct light sampling (APT_FLAG_NEE) in the material renderer: what it costs and what it buys.  Needs an MI355X (no fallback).

    python profiles/materials_nee.py [--reps 5] [--parent-lib PATH] [--out profiles/materials_nee.jsonl]
    rocprofv3 --kernel-trace --stats -d <dir> -o mn -- python profiles/materials_nee.py --trace      (a run of its own: one frame per shape)
    python profiles/materials_nee.py --kernel-stats <dir>/mn_results.db       (no GPU: that trace -> profiles/materials_nee_kernel_stats.csv)

HIP events around each frame, one warm-up per shape, all shapes alternated in the same process; every line of the output carries all
repetitions, their median, minimum and maximum.  Shapes: BASELINE C2 (1920x1080, samples 64, depth 8) on the 8-sphere scene (DIFF walls
and light, SPEC mirror) and on the 9-sphere demo scene, each with the stock light and with smallpt's lamp (gen_data.with_lamp); C4's
10 000-sphere scene with codes at samples 8 through the grid, stock light and lamp.  Three questions:
  (1) does the flag-off path cost what it cost before the flag existed?  --parent-lib: a librender_mi355x.so built from the parent
      commit, loaded next to this tree's and timed in the same alternation (the kernels are instruction-identical, so the difference
      must lie inside the parent's own run-to-run spread);
  (2) flag-on over flag-off time, per scene;
  (3) on the lamp scenes, at equal time: RMSE against a converged frame (flag on, 64x the samples, another seed) of a flag-on frame and
      of a flag-off frame whose sample count is scaled so that it takes the flag-on frame's measured time."""
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

W, H, DEPTH = 1920, 1080, 8
NS_BIG, SEED_BIG = 10000, 1
RMSE_SAMPLES, RMSE_FACTOR = 8, 64


def kernel_stats(db_path, out):
    import csv
    import sqlite3
    rows = sqlite3.connect(db_path).execute("select name, count(*), sum(duration), avg(duration), min(duration), max(duration) from kernels "
                                            "group by name order by sum(duration) desc").fetchall()
    total = sum(r[2] for r in rows)
    with open(out, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs", "Percentage"])
        for r in rows:
            w.writerow([r[0], r[1], r[2], round(r[3]), r[4], r[5], round(100.0 * r[2] / total, 2)])


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(here, "materials_nee.jsonl"))
    ap.add_argument("--parent-lib", help="librender_mi355x.so of the parent commit: its material frames are timed in the same run")
    ap.add_argument("--trace", action="store_true", help="one warm frame per shape and nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-stats", metavar="DB", help="summarise a rocprofv3 kernel trace (its sqlite output) per kernel and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, os.path.join(os.path.dirname(args.out), "materials_nee_kernel_stats.csv"))
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    # scene -> (table, codes, light index, samples, builds a grid)
    s8, m8 = gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    s9, m9 = gen_data.gen_spheres_materials()
    sb, mb = gen_data.gen_scene_materials(NS_BIG, seed=SEED_BIG)
    host = {"diff8": (s8, m8, 7, 64, False), "demo9": (s9, m9, 7, 64, False), "grid10k": (sb, mb, NS_BIG - 1, 8, True)}
    scenes = {}
    for name, (sph, mat, light, samples, use_grid) in host.items():
        for lamp in (False, True):
            table = dev(gen_data.with_lamp(sph, mat.size, light) if lamp else sph)
            grid = gen_data.build_grid_device(table, mat.size) if use_grid else None      # from the table it serves
            gflags = gen_data.grid_flags(grid, mat.size) if use_grid else 0
            scenes[name + ("_lamp" if lamp else "")] = dict(sph=table, mat=dev(mat), ns=int(mat.size), light=light, samples=samples,
                                                            grid=grid, gflags=gflags)

    def params(sc, nee, samples=None, seed=0):
        return apt.make_params(W, H, samples or sc["samples"], depth=DEPTH, num_spheres=sc["ns"], light_index=sc["light"], seed=seed,
                               accel=sc["grid"].data_ptr() if sc["grid"] is not None else 0,
                               flags=sc["gflags"] | (apt.APT_FLAG_NEE if nee else 0))

    fb_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    u8_buf = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")

    def frame(sc, p, lib=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if lib is None:
            render.render_frame(p, sc["sph"], fb=fb_buf, fb_u8=u8_buf, materials=sc["mat"])
        else:                                        # the parent's build, through its C-ABI (the struct is unchanged)
            rc = lib.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(sc["sph"].data_ptr()), ctypes.c_void_p(sc["mat"].data_ptr()),
                                                ctypes.c_uint64(0), ctypes.c_uint64(W * H), ctypes.c_void_p(fb_buf.data_ptr()),
                                                ctypes.c_void_p(u8_buf.data_ptr()))
            assert rc == 0, rc
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    shapes = {}
    for name, sc in scenes.items():
        shapes[name + "_off"] = (sc, params(sc, False), None)
        shapes[name + "_nee"] = (sc, params(sc, True), None)
        if parent is not None:
            shapes[name + "_off_parent"] = (sc, params(sc, False), parent)
    for name in ("diff8_lamp", "demo9_lamp"):         # the equal-time comparison's flag-on frame
        shapes[name + "_nee_s%d" % RMSE_SAMPLES] = (scenes[name], params(scenes[name], True, RMSE_SAMPLES), None)
        shapes[name + "_off_s%d" % RMSE_SAMPLES] = (scenes[name], params(scenes[name], False, RMSE_SAMPLES), None)
    if args.trace:
        for sc, p, lib in shapes.values():
            frame(sc, p, lib)
        render.check_device_status()
        return
    times = {k: [] for k in shapes}
    for sc, p, lib in shapes.values():               # warm-up: code objects
        frame(sc, p, lib)
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, (sc, p, lib) in shapes.items():
            times[name].append(round(frame(sc, p, lib), 3))
    render.check_device_status()

    def row(name):
        t = times[name]
        return {"shape": name, "frame": f"{W}x{H}", "depth": DEPTH, "samples": shapes[name][1].samples, "ms": t,
                "median_ms": round(statistics.median(t), 3), "min_ms": min(t), "max_ms": max(t)}

    rows = [row(name) for name in shapes]
    med = {r["shape"]: r["median_ms"] for r in rows}
    for name, sc in scenes.items():
        with render.TraceCounter() as t_off:
            frame(sc, shapes[name + "_off"][1])
        with render.TraceCounter() as t_on:
            frame(sc, shapes[name + "_nee"][1])
        s = {"shape": "summary_" + name, "nee_over_off": round(med[name + "_nee"] / med[name + "_off"], 3),
             "segments_off": t_off.value, "segments_nee": t_on.value, "segments_ratio": round(t_on.value / t_off.value, 3)}
        if parent is not None:
            a, b = times[name + "_off"], times[name + "_off_parent"]
            s.update(off_over_parent=round(med[name + "_off"] / med[name + "_off_parent"], 4),
                     off_minus_parent_ms=round(med[name + "_off"] - med[name + "_off_parent"], 3),
                     parent_spread_ms=round(max(b) - min(b), 3), off_spread_ms=round(max(a) - min(a), 3))
        rows.append(s)

    # (3) equal time on the lamp scenes
    def image(sc, p):
        t = frame(sc, p)
        return t, fb_buf.clone()

    for name in ("diff8_lamp", "demo9_lamp"):
        sc = scenes[name]
        t_on, t_off = med[name + "_nee_s%d" % RMSE_SAMPLES], med[name + "_off_s%d" % RMSE_SAMPLES]
        s_off = max(1, round(RMSE_SAMPLES * t_on / t_off))                   # the plain renderer's samples in the flag-on frame's time
        _, ref = image(sc, params(sc, True, RMSE_SAMPLES * RMSE_FACTOR, seed=12345))
        _, on = image(sc, params(sc, True, RMSE_SAMPLES, seed=1))
        image(sc, params(sc, False, s_off, seed=1))                          # warm-up of this sample count
        ts = [image(sc, params(sc, False, s_off, seed=1)) for _ in range(3)]
        off = ts[-1][1]
        _, off_same_s = image(sc, params(sc, False, RMSE_SAMPLES, seed=1))
        rmse = lambda x: float(((x - ref).double() ** 2).mean().sqrt())
        rows.append({"shape": "equal_time_" + name, "reference": f"flag on, samples {RMSE_SAMPLES * RMSE_FACTOR}, seed 12345",
                     "nee_samples": RMSE_SAMPLES, "nee_ms": t_on, "off_samples": s_off, "off_ms": round(statistics.median(t for t, _ in ts), 3),
                     "rmse_nee": round(rmse(on), 6), "rmse_off_equal_time": round(rmse(off), 6),
                     "rmse_off_equal_samples": round(rmse(off_same_s), 6),
                     "rmse_ratio_off_over_nee_equal_time": round(rmse(off) / rmse(on), 3),
                     "mean_ref": round(float(ref.mean()), 6), "mean_nee": round(float(on.mean()), 6), "mean_off": round(float(off.mean()), 6)})
    render.check_device_status()
    meta = {"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
            "parent_lib": bool(parent), "scene_grid10k": f"gen_scene_materials({NS_BIG}, seed={SEED_BIG})"}
    with open(args.out, "w") as f:
        for r in rows + [meta]:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
