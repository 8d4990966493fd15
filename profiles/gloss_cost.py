#!/usr/bin/env python3
"""What the rough-metal material (APT_MAT_GLOSS, APT_FLAG_GLOSS) costs the material renderer.  Needs an MI355X (no fallback).

    python profiles/gloss_cost.py [--reps 5] [--parent-lib OTHER/librender_mi355x.so] [--out profiles/gloss_cost.jsonl]

HIP events around each frame, one warm-up per shape, the shapes alternated in the same process (profiles/materials_grid.py's method);
every line carries all repetitions, their median, minimum and maximum.  1920x1080, samples 64 (256 spp), depth 8 -- BASELINE's C2 shape:
  a   the demo scene (9 spheres: the tile form) without the flag: the kernel the renderer had before the flag existed
  b   the same table with the flag and no gloss word: the price of the gloss instantiation alone
  c   the mirror ball as a gloss ball, alpha 0.25
  a8 / b8 / c8   the same three on gen_spheres' 8 spheres (walls and light DIFF, ball SPEC): the 8-sphere form
  a_parent / a8_parent   (--parent-lib) shapes a and a8 through another build of the library, loaded next to this one
samples 8, gen_scene_materials(10000, seed=1) through its grid:
  d0  the codes as generated (flagless)      d   every SPEC word a gloss word, alpha 0.05 .. 1"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, DEPTH, NS, SEED = 1920, 1080, 8, 10000, 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", help="another build of librender_mi355x.so: shapes a and a8 are also timed through it")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "gloss_cost.jsonl"))
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    GL = apt.APT_FLAG_GLOSS
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    sph9, mat9 = gen_data.gen_spheres_materials()
    _, mat9g = gen_data.gen_spheres_materials(gloss=0.25)
    sph8, mat8 = gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    mat8g = mat8.copy()
    mat8g[6] = gen_data.gloss(0.25)
    sphN, matN = gen_data.gen_scene_materials(NS, seed=SEED)
    matNg = np.array(matN, dtype=np.int32)
    spec = np.nonzero(matNg == apt.MAT_SPEC)[0]
    for i in spec:
        matNg[i] = gen_data.gloss(0.05 + 0.95 * ((int(i) * 977) % 1000) / 999.0)
    assert gen_data.materials_flags(mat9) == 0 and gen_data.materials_flags(mat9g) == GL and gen_data.materials_flags(matNg) == GL
    d_sph9, d_sph8, d_sphN = dev(sph9), dev(sph8), dev(sphN)
    grid = gen_data.build_grid_device(d_sphN, NS)
    gflags = gen_data.grid_flags(grid, NS)
    assert gflags == apt.APT_FLAG_GRID_SLOTS

    def params(ns, samples, flags, accel=0):
        return apt.make_params(W, H, samples, depth=DEPTH, num_spheres=ns, flags=flags, accel=accel)

    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))           # a second copy of the library: its own contexts and kernels

    def frame(p, sph, mat, lib=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if lib is None:
            a.record()
            fb, _ = render.render_frame(p, sph, materials=mat)
            b.record()
        else:
            fb = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
            u8 = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")
            st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            a.record()
            rc = lib.apt_render_frame_materials(ctypes.byref(p), st, ctypes.c_void_p(sph.data_ptr()), ctypes.c_void_p(mat.data_ptr()),
                                                ctypes.c_uint64(0), ctypes.c_uint64(W * H), ctypes.c_void_p(fb.data_ptr()),
                                                ctypes.c_void_p(u8.data_ptr()))
            b.record()
            assert rc == 0, rc
        torch.cuda.synchronize()
        return a.elapsed_time(b), fb

    shapes = {"a": (params(9, 64, 0), d_sph9, dev(mat9), None), "b": (params(9, 64, GL), d_sph9, dev(mat9), None),
              "c": (params(9, 64, GL), d_sph9, dev(mat9g), None),
              "a8": (params(8, 64, 0), d_sph8, dev(mat8), None), "b8": (params(8, 64, GL), d_sph8, dev(mat8), None),
              "c8": (params(8, 64, GL), d_sph8, dev(mat8g), None),
              "d0": (params(NS, 8, gflags, grid.data_ptr()), d_sphN, dev(matN), None),
              "d": (params(NS, 8, gflags | GL, grid.data_ptr()), d_sphN, dev(matNg), None)}
    if parent is not None:
        shapes["a_parent"] = shapes["a"][:3] + (parent,)
        shapes["a8_parent"] = shapes["a8"][:3] + (parent,)
    times = {k: [] for k in shapes}
    sha = {}
    for name, s in shapes.items():                   # warm-up: code objects, and the images
        sha[name] = hashlib.sha256(frame(*s)[1].cpu().numpy().tobytes()).hexdigest()[:16]
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, s in shapes.items():
            times[name].append(round(frame(*s)[0], 3))
    render.check_device_status()
    rows = [{"shape": name, "samples": shapes[name][0].samples, "num_spheres": shapes[name][0].num_spheres, "flags": shapes[name][0].flags,
             "frame": f"{W}x{H}", "depth": DEPTH, "ms": times[name], "median_ms": round(statistics.median(times[name]), 3),
             "min_ms": min(times[name]), "max_ms": max(times[name]), "fb_sha256": sha[name], "device": torch.cuda.get_device_name(0),
             "build_id": _lib.build_id()} for name in shapes]
    med = {r["shape"]: r["median_ms"] for r in rows}
    summary = {"shape": "summary", "b_over_a": round(med["b"] / med["a"], 4), "c_over_a": round(med["c"] / med["a"], 4),
               "b8_over_a8": round(med["b8"] / med["a8"], 4), "c8_over_a8": round(med["c8"] / med["a8"], 4),
               "d_over_d0": round(med["d"] / med["d0"], 4), "gloss_words_d": int(spec.size),
               "a_spread": round((max(times["a"]) - min(times["a"])) / med["a"], 4),
               "a8_spread": round((max(times["a8"]) - min(times["a8"])) / med["a8"], 4),
               "flag_without_gloss_words_same_image": sha["a"] == sha["b"] and sha["a8"] == sha["b8"]}
    if parent is not None:
        summary.update(a_over_parent=round(med["a"] / med["a_parent"], 4), a8_over_parent=round(med["a8"] / med["a8_parent"], 4),
                       parent_same_image=sha["a"] == sha["a_parent"] and sha["a8"] == sha["a8_parent"])
    rows.append(summary)
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
