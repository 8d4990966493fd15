#!/usr/bin/env python3
"""The film's moments and its filter (libdenoise_mi355x.so, include/render_mi355x_denoise.h): what they cost.  Needs an MI355X (no fallback).

    python profiles/denoise_cost.py [--reps 5] [--out profiles/denoise_cost.jsonl]

In the manner of profiles/film_cost.py: 1920x1080, HIP events around each launch sequence, one warm-up per shape, all shapes alternated
in one process; every line carries all repetitions, their median, minimum and maximum.
  (a) one film pass of 8 samples, depth 8, of the closed 8-sphere DIFF room with its lamp under APT_FLAG_NEE, directly into the film, and
      as a film with moments takes it: the scratch film zeroed, the pass into it, apt_film_accumulate_device.  The difference is the
      price of the moments; the accumulate alone is timed beside it.
  (b) apt_film_denoise_device with iterations = 1 .. 5.  The launches of one call run back to back on one stream, so
      T(j) - T(j - 1) is iteration j - 1 alone (step 1 << (j - 1)), and T(1) is prepare + iteration 0 + finish together: the entry gives
      no way to time those three apart, a kernel trace does.
  (c) the feature launch and the resolve beside them.
For the iteration kernel the achieved bytes/s are from the LOGICAL bytes of its text: 25 taps x 48 B of records, 9 x 4 B of variance
for gv, 16 B stored = 1252 B per pixel (taps that fall outside the image are not subtracted: under 2 % at step 16).  The operations
are counted from the contract: per tap 47 fp32 operations and two selects, per pixel about 1200.  Nothing here reads a counter."""
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

W, H, DEPTH, SAMPLES, PASSES = 1920, 1080, 8, 8, 4
ITER_BYTES = 25 * 48 + 9 * 4 + 16
ITER_FLOPS = 25 * 47 + 40


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(here, "denoise_cost.jsonl"))
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    L, DL = _lib.lib(), _lib.denoise_lib()
    N = W * H

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    sph = dev(gen_data.with_lamp(gen_data.gen_spheres(), 8, 7))
    mat = dev(np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32))
    p = apt.make_params(W, H, SAMPLES, depth=DEPTH, num_spheres=8, light_index=7, seed=0, flags=apt.APT_FLAG_NEE)

    # a real film of PASSES passes with its moments and features: what the filter is timed on
    film = render.Film(W, H, moments=True)
    for _ in range(PASSES):
        film.add_pass(p, sph, mat)
    feat = film.features(p, sph)
    plain = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    scratch = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    acc_film = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    acc_mom = torch.zeros((2, N), dtype=torch.float32, device="cuda")
    work = torch.empty(DL.apt_film_denoise_work_floats(W, H), dtype=torch.float32, device="cuda")
    out = torch.empty((3, N), dtype=torch.float32, device="cuda")
    u8 = torch.empty((N, 3), dtype=torch.uint8, device="cuda")
    table = dev(gen_data.film_curve("srgb"))
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def direct():
        render.render_frame_film(p, sph, mat, film=plain, pass_index=1)

    def through_scratch():
        scratch.zero_()
        render.render_frame_film(p, sph, mat, film=scratch, pass_index=1)
        render.film_accumulate(scratch, acc_film, acc_mom, 1)

    def denoise(it):
        rec = _lib.film_denoise_record(PASSES, it)
        return lambda: render.film_denoise(rec, film.buffer, film.moments, feat, W, H, work=work, out=out)

    def resolve():
        rec = _lib.film_resolve_record(1, 1.0, _lib.APT_TONEMAP_CLIP, 0.0)
        rc = L.apt_film_resolve_device(ctypes.byref(rec), None, out.data_ptr(), N, table.data_ptr(), None, u8.data_ptr())
        assert rc == 0, rc

    shapes = {"a_film_pass_direct": direct, "a_film_pass_scratch_accumulate": through_scratch,
              "a_accumulate_alone": lambda: render.film_accumulate(scratch, acc_film, acc_mom, 1)}
    for it in range(1, 6):
        shapes[f"b_denoise_{it}_iterations"] = denoise(it)
    shapes["c_features"] = lambda: render.render_frame_features(p, sph, features=feat)
    shapes["c_resolve_srgb_clip_u8"] = resolve

    times = {k: [] for k in shapes}
    for name, fn in shapes.items():                  # warm-up: code objects
        timed(fn)
    render.check_device_status()
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, fn in shapes.items():
            times[name].append(round(timed(fn), 4))
    render.check_device_status()

    rows = []
    for name, t in times.items():
        rows.append({"shape": name, "frame": f"{W}x{H}", "ms": t, "median_ms": round(statistics.median(t), 4), "min_ms": min(t), "max_ms": max(t)})
    med = {r["shape"]: r["median_ms"] for r in rows}
    for j in range(1, 5):                            # iteration j alone, repetition by repetition
        d = [round(b - a, 4) for a, b in zip(times[f"b_denoise_{j}_iterations"], times[f"b_denoise_{j + 1}_iterations"])]
        m = statistics.median(d)
        rows.append({"shape": f"b_iteration_{j}_step_{1 << j}_by_difference", "ms": d, "median_ms": round(m, 4), "min_ms": min(d), "max_ms": max(d),
                     "logical_bytes": N * ITER_BYTES, "logical_gb_per_s": round(N * ITER_BYTES / (m * 1e-3) / 1e9, 1),
                     "counted_gflop_per_s": round(N * ITER_FLOPS / (m * 1e-3) / 1e9, 1)})
    full = med["b_denoise_5_iterations"]
    rows.append({"shape": "summary", "samples_per_pass": SAMPLES, "depth": DEPTH,
                 "moments_price_ms": round(med["a_film_pass_scratch_accumulate"] - med["a_film_pass_direct"], 4),
                 "moments_price_over_film_pass": round(med["a_film_pass_scratch_accumulate"] / med["a_film_pass_direct"] - 1, 4),
                 "prepare_iteration0_finish_ms": med["b_denoise_1_iterations"],
                 "denoise_5_iterations_ms": full, "denoise_over_one_film_pass": round(full / med["a_film_pass_direct"], 4),
                 "denoise_features_resolve_ms": round(full + med["c_features"] + med["c_resolve_srgb_clip_u8"], 4)})
    rows.append({"shape": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
                 "film_passes": PASSES, "iteration_logical_bytes_per_pixel": ITER_BYTES, "iteration_counted_flops_per_pixel": ITER_FLOPS})
    with open(args.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
