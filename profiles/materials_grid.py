#!/usr/bin/env python3
"""The material renderer through the uniform grid against its tile form (brute force) on BASELINE configuration C4's scene with material
codes: gen_data.gen_scene_materials(10000, seed=1), 1920x1080, depth 8.  Needs an MI355X (no fallback).

    python profiles/materials_grid.py [--reps 5] [--out profiles/materials_grid.jsonl]
    rocprofv3 --kernel-trace --stats -d <dir> -o mg -- python profiles/materials_grid.py --trace     (a run of its own: one frame per shape)
    python profiles/materials_grid.py --kernel-stats <dir>/mg_results.db      (no GPU: that trace -> profiles/materials_grid_kernel_stats.csv)

HIP events around each frame, one warm-up per shape, the two forms alternated in the same process; every line of the output carries all
repetitions, their median, minimum and maximum.  samples 8 (32 spp): grid form and tile form (the tile form is the code the renderer had before the
grid form existed).  samples 64 (256 spp): the grid form, next to the mirror renderer's grid frame of the same scene.  The images of the two forms
are compared on the way (sha256 of the float frame): a speed-up between different images would not be one."""
import argparse
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

NS, SEED, W, H, DEPTH = 10000, 1, 1920, 1080, 8


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "materials_grid.jsonl"))
    ap.add_argument("--trace", action="store_true", help="one warm frame per kernel and nothing else (for rocprofv3 --kernel-trace)")
    ap.add_argument("--kernel-stats", metavar="DB", help="summarise a rocprofv3 kernel trace (its sqlite output) per kernel and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, os.path.join(os.path.dirname(args.out), "materials_grid_kernel_stats.csv"))
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    sph_h, mat_h = gen_data.gen_scene_materials(NS, seed=SEED)
    sph, mat = torch.from_numpy(sph_h).cuda(), torch.from_numpy(mat_h).cuda()
    grid = gen_data.build_grid_device(sph, NS)
    gflags = gen_data.grid_flags(grid, NS)
    assert gflags == apt.APT_FLAG_GRID_SLOTS

    def params(samples, with_grid):
        return apt.make_params(W, H, samples, depth=DEPTH, num_spheres=NS, accel=grid.data_ptr() if with_grid else 0,
                               flags=gflags if with_grid else 0)

    def frame(p, materials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fb, _ = render.render_frame(p, sph, materials=materials)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), fb

    shapes = {"materials_grid_s8": (params(8, True), mat), "materials_tiles_s8": (params(8, False), mat),
              "materials_grid_s64": (params(64, True), mat), "mirror_grid_s64": (params(64, True), None)}
    if args.trace:
        for name, (p, m) in shapes.items():
            frame(p, m)
        render.check_device_status()
        return
    times = {k: [] for k in shapes}
    sha = {}
    for name, (p, m) in shapes.items():              # warm-up: code objects, and the images
        sha[name] = hashlib.sha256(frame(p, m)[1].cpu().numpy().tobytes()).hexdigest()[:16]
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, (p, m) in shapes.items():
            times[name].append(round(frame(p, m)[0], 3))
    render.check_device_status()
    with render.TraceCounter() as tc:
        frame(*shapes["materials_grid_s8"])
    traced, cells, tests = tc.stats
    rows = [{"shape": name, "scene": f"gen_scene_materials({NS}, seed={SEED})", "frame": f"{W}x{H}", "depth": DEPTH,
             "ms": times[name], "median_ms": round(statistics.median(times[name]), 3), "min_ms": min(times[name]), "max_ms": max(times[name]),
             "fb_sha256": sha[name], "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id()} for name in shapes]
    g8, t8 = rows[0], rows[1]
    rows.append({"shape": "summary", "images_equal_s8": sha["materials_grid_s8"] == sha["materials_tiles_s8"],
                 "tiles_over_grid_s8": round(t8["median_ms"] / g8["median_ms"], 2),
                 "tiles_over_grid_s8_worst_case": round(t8["min_ms"] / g8["max_ms"], 2),
                 "materials_over_mirror_grid_s64": round(rows[2]["median_ms"] / rows[3]["median_ms"], 2),
                 "segments_s8": traced, "cells_per_segment": round(cells / traced, 2), "candidates_per_segment": round(tests / traced, 2),
                 "tile_pair_tests_per_s": round(traced * NS / (t8["median_ms"] * 1e-3), -9)})
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
