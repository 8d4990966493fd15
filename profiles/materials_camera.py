#!/usr/bin/env python3
"""The movable camera of the material renderer (apt_context_set_camera): what ray generation in its general form, and the thin lens,
cost per frame.  Needs an MI355X (no fallback).

    python profiles/materials_camera.py [--reps 5] [--parent-lib PATH] [--out profiles/materials_camera.jsonl]

HIP events around each frame, one warm-up per shape, all shapes alternated in the same process; every line of the output carries all
repetitions, their median, minimum and maximum.  Shapes: 1920x1080, depth 8, on the 8-sphere DIFF scene and the 9-sphere demo scene at
samples 64 and on the 10 000-sphere scene through the grid at samples 8; each with
  (a) no camera set -- on this build and, with --parent-lib (a librender_mi355x.so built from the parent commit, loaded next to this
      tree's), on the parent's: the kernels are instruction-identical, so this build's median must lie inside the parent's own spread;
  (b) apt_camera_default_host's record set: the same rays through the camera kernels (what the general form costs);
  (c) a look-at camera inside the room;
  (d) the same camera with a lens."""
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


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(here, "materials_camera.jsonl"))
    ap.add_argument("--parent-lib", help="librender_mi355x.so of the parent commit: its material frames are timed in the same run")
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    s8, m8 = gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    s9, m9 = gen_data.gen_spheres_materials()
    sb, mb = gen_data.gen_scene_materials(NS_BIG, seed=SEED_BIG)
    scenes = {}
    for name, (sph, mat, samples, use_grid) in {"diff8": (s8, m8, 64, False), "demo9": (s9, m9, 64, False), "grid10k": (sb, mb, 8, True)}.items():
        table = dev(sph)
        grid = gen_data.build_grid_device(table, mat.size) if use_grid else None
        scenes[name] = dict(sph=table, mat=dev(mat), ns=int(mat.size), samples=samples, grid=grid,
                            gflags=gen_data.grid_flags(grid, mat.size) if use_grid else 0)
    look = dict(eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), vfov_deg=55.0, offset=0.0, width=W, height=H)
    cameras = {"none": None, "default": gen_data.default_camera(W, H), "lookat": gen_data.camera(**look),
               "lens": gen_data.camera(aperture=2.5, **look)}

    def params(sc):
        return apt.make_params(W, H, sc["samples"], depth=DEPTH, num_spheres=sc["ns"], seed=0,
                               accel=sc["grid"].data_ptr() if sc["grid"] is not None else 0, flags=sc["gflags"])

    fb_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    u8_buf = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")

    def frame(sc, p, cam, lib=None):
        if lib is None:
            render.set_camera(cam)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if lib is None:
            render.render_frame(p, sc["sph"], fb=fb_buf, fb_u8=u8_buf, materials=sc["mat"])
        else:                                        # the parent's build, through its C-ABI (apt_render_params is unchanged)
            rc = lib.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(sc["sph"].data_ptr()), ctypes.c_void_p(sc["mat"].data_ptr()),
                                                ctypes.c_uint64(0), ctypes.c_uint64(W * H), ctypes.c_void_p(fb_buf.data_ptr()),
                                                ctypes.c_void_p(u8_buf.data_ptr()))
            assert rc == 0, rc
        b.record()
        torch.cuda.synchronize()
        if lib is None:
            render.set_camera(None)
        return a.elapsed_time(b)

    shapes = {}
    for name, sc in scenes.items():
        for cname, cam in cameras.items():
            shapes[f"{name}_{cname}"] = (sc, params(sc), cam, None)
        if parent is not None:
            shapes[f"{name}_none_parent"] = (sc, params(sc), None, parent)
    times = {k: [] for k in shapes}
    for sc, p, cam, lib in shapes.values():          # warm-up: code objects
        frame(sc, p, cam, lib)
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, (sc, p, cam, lib) in shapes.items():
            times[name].append(round(frame(sc, p, cam, lib), 3))
    render.check_device_status()

    def row(name):
        t = times[name]
        return {"shape": name, "frame": f"{W}x{H}", "depth": DEPTH, "samples": shapes[name][1].samples, "ms": t,
                "median_ms": round(statistics.median(t), 3), "min_ms": min(t), "max_ms": max(t)}

    rows = [row(name) for name in shapes]
    med = {r["shape"]: r["median_ms"] for r in rows}
    for name in scenes:
        s = {"shape": "summary_" + name, "default_over_none": round(med[name + "_default"] / med[name + "_none"], 4),
             "lookat_ms": med[name + "_lookat"], "lens_over_lookat": round(med[name + "_lens"] / med[name + "_lookat"], 4)}
        if parent is not None:
            b = times[name + "_none_parent"]
            s.update(none_over_parent=round(med[name + "_none"] / med[name + "_none_parent"], 4), parent_min_ms=min(b), parent_max_ms=max(b),
                     none_inside_parent_spread=bool(min(b) <= med[name + "_none"] <= max(b)))
        rows.append(s)
    meta = {"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
            "parent_lib": bool(parent), "scene_grid10k": f"gen_scene_materials({NS_BIG}, seed={SEED_BIG})", "lookat": {k: v for k, v in look.items()}}
    with open(args.out, "w") as f:
        for r in rows + [meta]:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
