#!/usr/bin/env python3
"""The environment of the material renderer (include/render_mi355x.h "environment"): what carrying it costs.  Needs an MI355X (no fallback).

    python profiles/environment_cost.py [--reps 5] [--parent-lib PATH] [--out profiles/environment_cost.jsonl]

In the manner of profiles/materials_lights.py: 1920x1080, depth 8, HIP events around each frame, one warm-up per shape, all shapes
alternated in one process; every line carries all repetitions, their median, minimum and maximum.  Three questions:
  (1) do the closed 8-sphere and 9-sphere material scenes without an environment cost what they cost in the parent commit?
      --parent-lib: a librender_mi355x.so built from the parent, loaded next to this tree's and timed in the same alternation (the
      kernels differ in the offset of their hidden arguments only);
  (2) the same scenes with a black environment set: the price of carrying the feature -- the kMatEnv kernels, which are always the
      general-camera, gloss instantiations, on frames that never leave the room;
  (3) the open 8-sphere scene (64 samples) and the open 10 000-sphere scene through the grid (8 samples) under a sky and a sun, the sun
      sampled (APT_ENV_SAMPLE_SUN) and not: ms and segments per path.
Nothing here says what bounds these kernels: that takes a counter run of its own."""
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
    ap.add_argument("--out", default=os.path.join(here, "environment_cost.jsonl"))
    ap.add_argument("--parent-lib", help="librender_mi355x.so of the parent commit: its frames without an environment are timed in the same run")
    ap.add_argument("--parent-first", action="store_true", help="time the parent's frame before this build's in every round, not after it (the slot's own effect)")
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def scene(sph, mat, samples, use_grid=False):
        ns = int(mat.size)
        table = dev(sph)
        grid = gen_data.build_grid_device(table, ns) if use_grid else None
        return dict(sph=table, mat=dev(mat), ns=ns, samples=samples, grid=grid, gflags=gen_data.grid_flags(grid, ns) if use_grid else 0,
                    mflags=gen_data.materials_flags(mat))

    closed = {"diff8": scene(gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 64),
              "demo9": scene(*gen_data.gen_spheres_materials(), 64)}
    opened = {"open8": scene(*gen_data.gen_spheres_open(), 64), "open_grid10k": scene(*gen_data.gen_scene_open(NS_BIG, seed=SEED_BIG), 8, True)}
    black = gen_data.environment()
    sky = dict(horizon=(0.6, 0.7, 0.8), zenith=(0.15, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(3.0e4, 2.8e4, 2.4e4), sun_angle_deg=0.2666)
    envs = {"black": black, "sun_sampled": gen_data.environment(sample_sun=True, **sky), "sun_plain": gen_data.environment(sample_sun=False, **sky)}

    def params(sc):
        return apt.make_params(W, H, sc["samples"], depth=DEPTH, num_spheres=sc["ns"], light_index=sc["ns"] - 1, seed=0,
                               accel=sc["grid"].data_ptr() if sc["grid"] is not None else 0, flags=sc["gflags"] | sc["mflags"])

    fb_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    u8_buf = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")

    def frame(sc, p, how):
        """how: None / the name of an environment through this build, or a ctypes library (the parent's build, through its C-ABI)."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if how is None or isinstance(how, str):
            render.set_environment(envs[how] if how else None)
            a.record()
            render.render_frame(p, sc["sph"], fb=fb_buf, fb_u8=u8_buf, materials=sc["mat"])
        else:
            a.record()
            rc = how.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(sc["sph"].data_ptr()), ctypes.c_void_p(sc["mat"].data_ptr()),
                                                ctypes.c_uint64(0), ctypes.c_uint64(W * H), ctypes.c_void_p(fb_buf.data_ptr()),
                                                ctypes.c_void_p(u8_buf.data_ptr()))
            assert rc == 0, rc
        b.record()
        torch.cuda.synchronize()
        render.set_environment(None)
        return a.elapsed_time(b)

    shapes = {}
    for name, sc in closed.items():
        if parent is not None and args.parent_first:
            shapes[name + "_noenv_parent"] = (sc, params(sc), parent)
        shapes[name + "_noenv"] = (sc, params(sc), None)
        shapes[name + "_black"] = (sc, params(sc), "black")
        if parent is not None and not args.parent_first:
            shapes[name + "_noenv_parent"] = (sc, params(sc), parent)
    for name, sc in opened.items():
        shapes[name + "_sun_sampled"] = (sc, params(sc), "sun_sampled")
        shapes[name + "_sun_plain"] = (sc, params(sc), "sun_plain")
    times = {k: [] for k in shapes}
    for sc, p, how in shapes.values():               # warm-up: code objects
        frame(sc, p, how)
    render.check_device_status()
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, (sc, p, how) in shapes.items():
            times[name].append(round(frame(sc, p, how), 3))
    render.check_device_status()

    def segments(name):
        with render.TraceCounter() as tc:
            frame(*shapes[name])
        return tc.value

    rows = []
    for name in shapes:
        t, p = times[name], shapes[name][1]
        r = {"shape": name, "frame": f"{W}x{H}", "depth": DEPTH, "samples": p.samples, "ms": t, "median_ms": round(statistics.median(t), 3),
             "min_ms": min(t), "max_ms": max(t)}
        if not name.endswith("_parent"):
            r["segments_per_path"] = round(segments(name) / p.num_paths, 3)
        rows.append(r)
    med = {r["shape"]: r["median_ms"] for r in rows}
    for name in closed:
        s = {"shape": "summary_" + name, "black_over_noenv": round(med[name + "_black"] / med[name + "_noenv"], 4)}
        if parent is not None:
            a, b = times[name + "_noenv"], times[name + "_noenv_parent"]
            s.update({"noenv_minus_parent_ms": round(med[name + "_noenv"] - med[name + "_noenv_parent"], 3),
                      "noenv_spread_ms": round(max(a) - min(a), 3), "parent_spread_ms": round(max(b) - min(b), 3)})
        rows.append(s)
    for name in opened:
        rows.append({"shape": "summary_" + name, "sampled_over_plain": round(med[name + "_sun_sampled"] / med[name + "_sun_plain"], 4)})
    render.check_device_status()
    meta = {"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps, "parent_lib": bool(parent), "parent_first": args.parent_first,
            "scene_open_grid10k": f"gen_scene_open({NS_BIG}, seed={SEED_BIG})", "sun": "0.2666 degrees half angle, radiance 3e4"}
    with open(args.out, "w") as f:
        for r in rows + [meta]:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
