#!/usr/bin/env python3
"""The first-hit feature planes (include/render_mi355x.h "features"): what a features launch costs next to one film pass of the same
parameters.  Needs an MI355X (no fallback).

    python profiles/features_cost.py [--reps 5] [--parent-lib PATH] [--out profiles/features_cost.jsonl]

In the manner of profiles/film_cost.py: 1920x1080, 8 samples, HIP events around each launch, one warm-up per shape, all shapes
alternated in one process; every line carries all repetitions, their median, minimum and maximum.
  (a) the closed 8-sphere room: a features launch, and one film pass at depth 8 (all DIFF but the mirror ball);
  (b) gen_scene_materials(10000, seed=1) through its grid: the same pair;
  (c) the same scene by LDS tiles (no grid): the same pair;
  (d) the headline mirror frame (render_frame, 64 samples, depth 8) on this build and -- with --parent-lib, a librender_mi355x.so built
      from the parent commit and loaded next to this tree's -- on the parent's: that nothing moved.  A phase of its own before the
      others, ten repetitions in the order this, parent, parent, this.
  (e) the room at 48x32 and 256x256: one lane per pixel leaves most of the chip idle at small frames.
(c) is alternated on its own, last: a launch that follows its 1.5 s film pass runs slower than it otherwise does -- in turn with (c),
(a)'s features launch took 1.07 instead of 0.87 ms and the headline frame 20.4 instead of 17.9 ms.
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

W, H, DEPTH, SAMPLES, HEADLINE_SAMPLES = 1920, 1080, 8, 8, 64
NS_BIG, SEED_BIG = 10000, 1


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(here, "features_cost.jsonl"))
    ap.add_argument("--parent-lib", help="librender_mi355x.so of the parent commit: its headline frame (d) is timed in the same run")
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def scene(sph, mat):
        return dict(sph=dev(sph), mat=dev(mat), ns=int(mat.size), mflags=gen_data.materials_flags(mat), accel=0, gflags=0)

    room = scene(gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32))
    big_sph, big_mat = gen_data.gen_scene_materials(NS_BIG, seed=SEED_BIG)
    tiles = scene(big_sph, big_mat)
    hgrid = gen_data.build_grid(big_sph, NS_BIG)
    d_grid = torch.from_numpy(hgrid.view(np.int32)).cuda()
    grid = dict(tiles, accel=d_grid.data_ptr(), gflags=gen_data.grid_flags(hgrid, NS_BIG))
    assert grid["gflags"] == apt.APT_FLAG_GRID_SLOTS

    def params(sc, w=W, h=H):
        return apt.make_params(w, h, SAMPLES, depth=DEPTH, num_spheres=sc["ns"], light_index=sc["ns"] - 1, seed=0, flags=sc["mflags"] | sc["gflags"],
                               accel=sc["accel"])

    film = torch.zeros((3, W * H), dtype=torch.float32, device="cuda")
    feat = torch.zeros((apt.APT_FEATURE_PLANES, W * H), dtype=torch.float32, device="cuda")
    fb_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    u8_buf = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")
    mirror = dev(gen_data.gen_spheres())
    headline = apt.make_params(W, H, HEADLINE_SAMPLES, depth=DEPTH, seed=0)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def features(sc, w=W, h=H):
        p = params(sc, w, h)                         # the film pass's record, as it is
        out = feat.view(-1)[:apt.APT_FEATURE_PLANES * w * h].view(apt.APT_FEATURE_PLANES, w * h)
        return lambda: render.render_frame_features(p, sc["sph"], features=out)

    def film_pass(sc, w=W, h=H):
        p = params(sc, w, h)
        out = film.view(-1)[:3 * w * h].view(3, w * h)
        return lambda: render.render_frame_film(p, sc["sph"], sc["mat"], film=out, pass_index=0)

    def mirror_frame(lib=None):
        if lib is None:
            return lambda: render.render_frame(headline, mirror, fb=fb_buf, fb_u8=u8_buf)

        def call():                                  # the parent's build through its C-ABI
            rc = lib.render_frame(ctypes.byref(headline), None, ctypes.c_void_p(mirror.data_ptr()), ctypes.c_uint64(0), ctypes.c_uint64(W * H),
                                  ctypes.c_void_p(fb_buf.data_ptr()), ctypes.c_void_p(u8_buf.data_ptr()))
            assert rc == 0, rc
        return call

    shapes = {"a_room_features": features(room), "a_room_film_pass": film_pass(room),
              "b_grid10000_features": features(grid), "b_grid10000_film_pass": film_pass(grid),
              "c_tiles10000_features": features(tiles), "c_tiles10000_film_pass": film_pass(tiles),
              "d_headline_mirror_frame": mirror_frame()}
    for w, h in ((48, 32), (256, 256)):
        shapes[f"e_room_{w}x{h}_features"] = features(room, w, h)
        shapes[f"e_room_{w}x{h}_film_pass"] = film_pass(room, w, h)
    if parent is not None:
        shapes["d_headline_mirror_frame_parent"] = mirror_frame(parent)

    times = {k: [] for k in shapes}
    for name in shapes:                              # warm-up: code objects
        timed(shapes[name])
    render.check_device_status()
    pair = [n for n in shapes if n.startswith("d_")]
    for r in range(2 * args.reps):                   # (d) first, the order swapped every repetition
        for name in (pair if r % 2 == 0 else pair[::-1]):
            times[name].append(round(timed(shapes[name]), 4))
    heavy = [n for n in shapes if n.startswith("c_")]
    for group in ([n for n in shapes if n not in pair + heavy], heavy):
        for _ in range(args.reps):                   # alternated: neighbours in time see the same machine
            for name in group:
                times[name].append(round(timed(shapes[name]), 4))
    render.check_device_status()

    rows = []
    for name in shapes:
        t = times[name]
        rows.append({"shape": name, "frame": name.split("_")[2] if name.startswith("e_") else f"{W}x{H}", "samples": HEADLINE_SAMPLES if name.startswith("d_") else SAMPLES, "depth": DEPTH, "ms": t,
                     "median_ms": round(statistics.median(t), 4), "min_ms": min(t), "max_ms": max(t)})
    med = {r["shape"]: r["median_ms"] for r in rows}
    s = {"shape": "summary"}
    for k in ("a_room", "b_grid10000", "c_tiles10000"):
        s[f"features_over_film_pass_{k[2:]}"] = round(med[f"{k}_features"] / med[f"{k}_film_pass"], 4)
    if parent is not None:
        b = times["d_headline_mirror_frame_parent"]
        s.update({"headline_minus_parent_ms": round(med["d_headline_mirror_frame"] - med["d_headline_mirror_frame_parent"], 4),
                  "parent_spread_ms": round(max(b) - min(b), 4)})
    rows.append(s)
    meta = {"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps, "parent_lib": bool(parent)}
    with open(args.out, "w") as f:
        for r in rows + [meta]:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
