#!/usr/bin/env python3
"""The film of the material renderer (include/render_mi355x.h "film"): what a film pass and the resolve cost.  Needs an MI355X (no fallback).

    python profiles/film_cost.py [--reps 5] [--parent-lib PATH] [--out profiles/film_cost.jsonl]

In the manner of profiles/environment_cost.py: 1920x1080, depth 8, 64 samples, HIP events around each launch, one warm-up per shape,
all shapes alternated in one process; every line carries all repetitions, their median, minimum and maximum.
  (a) the closed 8-sphere DIFF room with a black environment through apt_render_frame_materials, on this build and -- with
      --parent-lib, a librender_mi355x.so built from the parent commit and loaded next to this tree's -- on the parent's;
  (b) the same frame as one film pass: the kernels differ from (a)'s in the tail only, so (a) on the parent build is its yardstick;
  (c) gen_spheres_open under a sky and a sampled sun, as a frame and as a film pass;
  (d) four film passes of 16 samples against one frame of 64: what launching in passes costs;
  (e) the resolve at 1080p, both curves (clip and Reinhard), in microseconds and GB/s of the 12 B read and 3 B (8-bit image only) or
      15 B (with the float image) written per pixel.
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

W, H, DEPTH, SAMPLES = 1920, 1080, 8, 64


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(here, "film_cost.jsonl"))
    ap.add_argument("--parent-lib", help="librender_mi355x.so of the parent commit: its frame (a) is timed in the same run")
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    L = _lib.lib()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def scene(sph, mat):
        return dict(sph=dev(sph), mat=dev(mat), ns=int(mat.size), mflags=gen_data.materials_flags(mat))

    room = scene(gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32))
    open8 = scene(*gen_data.gen_spheres_open())
    black = gen_data.environment()
    sun = gen_data.environment(horizon=(0.6, 0.7, 0.8), zenith=(0.15, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(3.0e4, 2.8e4, 2.4e4),
                               sun_angle_deg=0.2666, sample_sun=True)

    def params(sc, samples=SAMPLES):
        return apt.make_params(W, H, samples, depth=DEPTH, num_spheres=sc["ns"], light_index=sc["ns"] - 1, seed=0, flags=sc["mflags"])

    fb_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    u8_buf = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")
    film = torch.zeros((3, W * H), dtype=torch.float32, device="cuda")
    out_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    tables = {c: dev(gen_data.film_curve(c)) for c in ("linear", "srgb")}

    def timed(env, fn):
        """One launch sequence between two events, with the default context's environment set -> ms."""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        render.set_environment(env)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        render.set_environment(None)
        return a.elapsed_time(b)

    def frame(sc, p, lib=None):
        if lib is None:
            return lambda: render.render_frame(p, sc["sph"], fb=fb_buf, fb_u8=u8_buf, materials=sc["mat"])

        def call():                                  # the parent's build through its C-ABI; its default context gets the environment too
            rc = lib.apt_render_frame_materials(ctypes.byref(p), None, ctypes.c_void_p(sc["sph"].data_ptr()), ctypes.c_void_p(sc["mat"].data_ptr()),
                                                ctypes.c_uint64(0), ctypes.c_uint64(W * H), ctypes.c_void_p(fb_buf.data_ptr()),
                                                ctypes.c_void_p(u8_buf.data_ptr()))
            assert rc == 0, rc
        return call

    def passes(sc, p, n):
        def call():
            for k in range(n):
                render.render_frame_film(p, sc["sph"], sc["mat"], film=film, pass_index=k)
        return call

    def resolve(curve, tonemap, want_out):
        rec = _lib.film_resolve_record(4, 1.0, tonemap, 1.0 / 64.0 if tonemap else 0.0)

        def call():
            rc = L.apt_film_resolve_device(ctypes.byref(rec), None, ctypes.c_void_p(film.data_ptr()), ctypes.c_uint64(W * H),
                                           ctypes.c_void_p(tables[curve].data_ptr()), ctypes.c_void_p(out_buf.data_ptr()) if want_out else None,
                                           ctypes.c_void_p(u8_buf.data_ptr()))
            assert rc == 0, rc
        return call

    # name -> (the context's environment, the launches, the parent's environment setter or None)
    shapes = {}
    if parent is not None:
        shapes["a_room_black_frame_parent"] = (None, frame(room, params(room), parent))
    shapes["a_room_black_frame"] = (black, frame(room, params(room)))
    shapes["b_room_black_film_pass"] = (black, passes(room, params(room), 1))
    shapes["b_room_noenv_film_pass"] = (None, passes(room, params(room), 1))
    shapes["c_open8_sun_frame"] = (sun, frame(open8, params(open8)))
    shapes["c_open8_sun_film_pass"] = (sun, passes(open8, params(open8), 1))
    shapes["d_open8_sun_film_4x16"] = (sun, passes(open8, params(open8, 16), 4))
    for curve in ("linear", "srgb"):
        shapes[f"e_resolve_{curve}_clip_u8"] = (None, resolve(curve, 0, False))
        shapes[f"e_resolve_{curve}_reinhard_u8_float"] = (None, resolve(curve, 1, True))

    def run(name):
        env, fn = shapes[name]
        if name.endswith("_parent"):                 # the parent library has a default context of its own
            assert parent.apt_set_environment(ctypes.byref(black)) == 0
            try:
                return timed(None, fn)
            finally:
                assert parent.apt_set_environment(None) == 0
        return timed(env, fn)

    times = {k: [] for k in shapes}
    for name in shapes:                              # warm-up: code objects
        run(name)
    render.check_device_status()
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name in shapes:
            times[name].append(round(run(name), 4))
    render.check_device_status()

    rows = []
    for name in shapes:
        t = times[name]
        r = {"shape": name, "frame": f"{W}x{H}", "ms": t, "median_ms": round(statistics.median(t), 4), "min_ms": min(t), "max_ms": max(t)}
        if name.startswith("e_"):
            nbytes = W * H * (12 + 3 + (12 if name.endswith("_float") else 0))
            r.update({"median_us": round(statistics.median(t) * 1e3, 2), "bytes": nbytes, "gb_per_s": round(nbytes / (statistics.median(t) * 1e-3) / 1e9, 1)})
        else:
            r.update({"depth": DEPTH, "samples": 16 if name.endswith("4x16") else SAMPLES})
        rows.append(r)
    med = {r["shape"]: r["median_ms"] for r in rows}
    s = {"shape": "summary", "film_pass_over_frame_room_black": round(med["b_room_black_film_pass"] / med["a_room_black_frame"], 4),
         "film_pass_over_frame_open8_sun": round(med["c_open8_sun_film_pass"] / med["c_open8_sun_frame"], 4),
         "four_passes_of_16_over_frame_of_64": round(med["d_open8_sun_film_4x16"] / med["c_open8_sun_frame"], 4),
         "four_passes_of_16_over_film_pass_of_64": round(med["d_open8_sun_film_4x16"] / med["c_open8_sun_film_pass"], 4)}
    if parent is not None:
        b = times["a_room_black_frame_parent"]
        s.update({"film_pass_minus_parent_frame_ms": round(med["b_room_black_film_pass"] - med["a_room_black_frame_parent"], 4),
                  "frame_minus_parent_frame_ms": round(med["a_room_black_frame"] - med["a_room_black_frame_parent"], 4),
                  "parent_spread_ms": round(max(b) - min(b), 4)})
    rows.append(s)
    meta = {"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps, "parent_lib": bool(parent),
            "sun": "0.2666 degrees half angle, radiance 3e4, sampled", "resolve_passes": 4}
    with open(args.out, "w") as f:
        for r in rows + [meta]:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
