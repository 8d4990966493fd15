#!/usr/bin/env python3
"""What APT_FLAG_MIS costs and what it buys.  Needs an MI355X (no fallback).

    python profiles/mis_cost.py [--reps 5] [--parent-lib OTHER/librender_mi355x.so] [--out profiles/mis_ab.json]

Timing: HIP events around each frame, one warm-up per shape, the shapes alternated in the same process (profiles/gloss_cost.py's
method); every shape carries all repetitions, their median, minimum and maximum.  1920x1080, samples 8 (32 spp), depth 8, APT_FLAG_NEE,
the glossy lamp room: gen_spheres with the ball a rough metal of alpha 0.3 and smallpt's small lamp as the light,
  room8 / room8_mis     the 8-sphere form without and with the flag
  grid9 / grid9_mis     the demo scene's 9 spheres (its mirror ball the rough metal) behind their grid
  room8_parent / grid9_parent   (--parent-lib) the flagless shapes through another build of the library, loaded next to this one
Quality: a 256x192 frame of the 8-sphere room through the film entries (unclipped), MSE over all pixels and channels against a flagless
reference of 4096 spp (64 passes of samples 16), for 8 passes of samples 2 (64 spp) without and with the flag: equal samples (the same
passes) and equal time (the passes scaled by the measured cost ratio of the 256x192 pass).  The same three figures over the pixels whose
first surface is the rough ball alone (the feature planes' albedo), and against a 4096-spp reference rendered WITH the flag: the
flagless reference's highlight is itself not converged."""
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

W, H, SAMPLES, DEPTH = 1920, 1080, 8, 8
QW, QH = 256, 192


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "mis_ab.json"))
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    sph8, mat8 = gen_data.with_lamp(gen_data.gen_spheres(), 8, 7), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    mat8[6] = gen_data.gloss(0.3)
    sph9, mat9 = gen_data.gen_spheres_materials(gloss=0.3)
    sph9 = gen_data.with_lamp(sph9, 9, 7)
    d8, d9, m8, m9 = dev(sph8), dev(sph9), dev(mat8), dev(np.asarray(mat9))
    grid = gen_data.build_grid_device(d9, 9)
    gflags = gen_data.grid_flags(grid, 9)
    assert gflags == apt.APT_FLAG_GRID_SLOTS
    base = apt.APT_FLAG_NEE | gen_data.materials_flags(mat8)
    with_mis = apt.APT_FLAG_NEE | gen_data.materials_flags(mat8, mis=True)
    assert with_mis == base | apt.APT_FLAG_MIS

    def params(ns, flags, accel=0, w=W, h=H, samples=SAMPLES, seed=1):
        return apt.make_params(w, h, samples, depth=DEPTH, num_spheres=ns, light_index=7, flags=flags, accel=accel, seed=seed)

    parent = ctypes.CDLL(os.path.abspath(args.parent_lib)) if args.parent_lib else None

    def frame(p, sph, mat, lib=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if lib is None:
            a.record()
            render.render_frame(p, sph, materials=mat)
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
        return a.elapsed_time(b)

    shapes = {"room8": (params(8, base), d8, m8, None), "room8_mis": (params(8, with_mis), d8, m8, None),
              "grid9": (params(9, base | gflags, grid.data_ptr()), d9, m9, None),
              "grid9_mis": (params(9, with_mis | gflags, grid.data_ptr()), d9, m9, None)}
    if parent is not None:
        shapes["room8_parent"] = shapes["room8"][:3] + (parent,)
        shapes["grid9_parent"] = shapes["grid9"][:3] + (parent,)
    times = {k: [] for k in shapes}
    for s in shapes.values():
        frame(*s)
    for _ in range(args.reps):
        for name, s in shapes.items():
            times[name].append(round(frame(*s), 3))
    render.check_device_status()
    med = {k: round(statistics.median(v), 3) for k, v in times.items()}
    out = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "frame": f"{W}x{H}", "samples": SAMPLES, "depth": DEPTH,
           "timing": {k: {"ms": v, "median_ms": med[k], "min_ms": min(v), "max_ms": max(v)} for k, v in times.items()},
           "mis_over_flagless": {"room8": round(med["room8_mis"] / med["room8"], 4), "grid9": round(med["grid9_mis"] / med["grid9"], 4)},
           "flagless_spread": {k: round((max(times[k]) - min(times[k])) / med[k], 4) for k in ("room8", "grid9")}}
    if parent is not None:
        out["flagless_over_parent"] = {"room8": round(med["room8"] / med["room8_parent"], 4), "grid9": round(med["grid9"] / med["grid9_parent"], 4)}

    # ---- quality: MSE against a 4096-spp flagless film -------------------------------------------------------------------------------
    def film(flags, samples, passes, seed):
        p = params(8, flags, w=QW, h=QH, samples=samples, seed=seed)
        buf = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(passes):
            buf = render.render_frame_film(p, d8, m8, film=buf, pass_index=k)
        b.record()
        torch.cuda.synchronize()
        return (buf / float(passes)).double().cpu().numpy(), a.elapsed_time(b)

    ref, _ = film(base, 16, 64, seed=1000)                       # 64 passes x 64 spp = 4096 spp
    ref_mis, _ = film(with_mis, 16, 64, seed=2000)
    feat = render.render_frame_features(params(8, base, w=QW, h=QH, samples=2, seed=7), d8).cpu().numpy()
    ball_albedo = sph8[:80].reshape(10, 8)[7:10, 6]
    ball = (feat[apt.APT_FEATURE_COVERAGE] == 1.0) & (np.abs(feat[apt.APT_FEATURE_ALBEDO:apt.APT_FEATURE_ALBEDO + 3] - ball_albedo[:, None]) < 1e-4).all(axis=0)
    film(base, 2, 2, 5), film(with_mis, 2, 2, 5)                 # warm-up
    n = 8                                                        # 8 passes x 8 spp = 64 spp
    plain, t_plain = film(base, 2, n, seed=7)
    mis, t_mis = film(with_mis, 2, n, seed=7)
    n_eq = max(1, int(round(n * t_plain / t_mis)))               # what the flag affords in the flagless frame's time
    mis_eq, t_mis_eq = film(with_mis, 2, n_eq, seed=7)
    mse = lambda x, r=None, m=None: float((((x - (ref if r is None else r)) ** 2)[:, slice(None) if m is None else m]).mean())
    out["quality"] = {"frame": f"{QW}x{QH}", "reference_spp": 4096, "spp": 8 * n, "mse_flagless": mse(plain), "mse_mis_equal_samples": mse(mis),
                      "ms_flagless": round(t_plain, 3), "ms_mis_equal_samples": round(t_mis, 3), "equal_time_passes": n_eq,
                      "mse_mis_equal_time": mse(mis_eq), "ms_mis_equal_time": round(t_mis_eq, 3),
                      "ball_pixels": int(ball.sum()),
                      "ball_vs_flagless_reference": {"mse_flagless": mse(plain, None, ball), "mse_mis_equal_samples": mse(mis, None, ball),
                                                     "mse_mis_equal_time": mse(mis_eq, None, ball)},
                      "ball_vs_mis_reference": {"mse_flagless": mse(plain, ref_mis, ball), "mse_mis_equal_samples": mse(mis, ref_mis, ball),
                                                "mse_mis_equal_time": mse(mis_eq, ref_mis, ball),
                                                "mse_of_the_flagless_reference": mse(ref, ref_mis, ball)},
                      "frame_vs_mis_reference": {"mse_flagless": mse(plain, ref_mis), "mse_mis_equal_samples": mse(mis, ref_mis),
                                                 "mse_mis_equal_time": mse(mis_eq, ref_mis)}}
    render.check_device_status()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
