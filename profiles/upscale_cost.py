#!/usr/bin/env python3
"""Guided film upscaling (include/render_mi355x_upscale.h): what apt_film_upscale_device costs at 1920x1080 from 960x540, beside the
meter and film_compare (the yardsticks of profiles/metrics_cost.py), one 8-sample film pass at each of the two resolutions and one
feature launch at full size.  Needs an MI355X (no fallback).  The method is profiles/metrics_cost.py's.

    python profiles/upscale_cost.py [--reps 5] [--out profiles/upscale_cost.jsonl]

The scene is open8 under the sky and the sun (tests/gpu_harness.py's), seen by the same look-at camera at both sizes (two contexts, one
per size).  Each shape is warmed up, then timed with device events around enough back-to-back launches to fill about a quarter of a
second, `reps` times, all shapes alternated in one process, no profiler attached; every line carries all repetitions (ms per call),
their median, minimum and maximum.

The algorithmic bytes of one upscale call are counted from the shapes: prepare reads 11 floats a low pixel and writes its three
16-byte records (12 floats); the upsample reads 8 plane floats a full pixel and every record once (12 floats a low pixel: taps shared
between lanes are not counted twice), and writes 3 floats and one word a full pixel: 140 bytes a low pixel + 48 bytes a full pixel,
172 MB here, set against a peak of 8 TB/s.  That fits the 256 MiB last-level cache, and back-to-back launches over the same buffers
find much of it there; the "_rotating" shapes take another of 4 sets of full-size planes and outputs and of low inputs (4 x 125 MB of
full-size buffers) at every launch, and are the ones to read for planes that were just rendered by something else.  Nothing here says
what bounds the kernels: that takes a counter run of its own."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, LW, LH, DEPTH, SAMPLES = 1920, 1080, 960, 540, 4, 8
N, NL = W * H, LW * LH
PEAK_BYTES_PER_S = 8e12
SETS = 4


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fill-ms", type=float, default=250.0, help="device time one measurement fills with back-to-back launches")
    ap.add_argument("--out", default=os.path.join(here, "upscale_cost.jsonl"))
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    sph, mat = gen_data.gen_spheres_open()
    sph = gen_data.with_lamps(sph, 8, [5, 4], radius=8.0, emission=[(30.0, 20.0, 10.0), 12.0])
    flags = gen_data.materials_flags(mat)
    d_sph, d_mat = dev(sph), dev(mat)
    env = gen_data.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(30.0, 28.0, 24.0),
                               sun_angle_deg=8.0, sample_sun=True)
    camera = lambda w, h: gen_data.camera(width=w, height=h, eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05),
                                          vfov_deg=55.0, offset=0.0)
    params = lambda w, h, seed: apt.make_params(w, h, SAMPLES, depth=DEPTH, num_spheres=8, light_index=5, seed=seed, flags=flags)
    p_hi, p_lo = params(W, H, 3), params(LW, LH, 3)
    ctx_hi, ctx_lo = render.Context(), render.Context()
    for ctx, (w, h) in ((ctx_hi, (W, H)), (ctx_lo, (LW, LH))):
        ctx.set_environment(env)
        ctx.set_camera(camera(w, h))
    film, ref, low = render.Film(W, H), render.Film(W, H), render.Film(LW, LH)
    for _ in range(2):
        film.add_pass(p_hi, d_sph, d_mat, context=ctx_hi)
        ref.add_pass(params(W, H, 4), d_sph, d_mat, context=ctx_hi)
        low.add_pass(p_lo, d_sph, d_mat, context=ctx_lo)
    lo_mean = low.mean()
    lo_feat = low.features(p_lo, d_sph, context=ctx_lo)
    hi_feat = film.features(p_hi, d_sph, context=ctx_hi)
    scratch_hi = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    scratch_lo = torch.zeros((3, NL), dtype=torch.float32, device="cuda")
    feat_out = torch.empty((_lib.APT_FEATURE_PLANES, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx_hi.check()
    ctx_lo.check()

    U = _lib.upscale_lib()
    urec = _lib.film_upscale_record()
    work = torch.empty(U.apt_film_upscale_work_floats(LW, LH), dtype=torch.float32, device="cuda")
    out = torch.empty((3, N), dtype=torch.float32, device="cuda")
    resolved = torch.empty(N, dtype=torch.int32, device="cuda")
    sets = [(lo_mean.clone(), lo_feat.clone(), hi_feat.clone(), torch.empty_like(work), torch.empty_like(out), torch.empty_like(resolved))
            for _ in range(SETS)]
    M = _lib.metrics_lib()
    crec = _lib.film_compare_record(film.passes, ref.passes)
    cwork = torch.empty(M.apt_film_compare_work_doubles(N), dtype=torch.float64, device="cuda")
    cres = torch.empty(_lib.APT_COMPARE_WORDS, dtype=torch.int64, device="cuda")
    mrec = _lib.film_meter_record(film.passes)
    mwork = torch.empty(_lib.post_lib().apt_film_meter_work_words(N), dtype=torch.int32, device="cuda")
    hist = torch.empty(_lib.APT_METER_WORDS, dtype=torch.int32, device="cuda")
    turn = [0]

    def rotating():
        turn[0] = (turn[0] + 1) % SETS
        a, b, c, wk, o, r = sets[turn[0]]
        return render.film_upscale(urec, a, b, LW, LH, c, W, H, wk, o, r)

    shapes = {
        "film_pass_8spp_full": lambda: ctx_hi.render_frame_film(p_hi, d_sph, d_mat, scratch_hi, 1),
        "film_pass_8spp_low": lambda: ctx_lo.render_frame_film(p_lo, d_sph, d_mat, scratch_lo, 1),
        "features_full": lambda: ctx_hi.render_frame_features(p_hi, d_sph, feat_out),
        "meter": lambda: render.film_meter(mrec, film.buffer, mwork, hist),
        "compare": lambda: render.film_compare(crec, film.buffer, ref.buffer, cwork, cres),
        "upscale": lambda: render.film_upscale(urec, lo_mean, lo_feat, LW, LH, hi_feat, W, H, work, out, resolved),
        "upscale_rotating": rotating,
    }
    upscale_bytes = 140 * NL + 48 * N
    algorithmic_bytes = {"meter": 12 * N, "compare": 24 * N, "upscale": upscale_bytes, "upscale_rotating": upscale_bytes}

    def timed(fn, calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / calls

    calls = {}
    for name, fn in shapes.items():                  # warm-up (code objects), and how many launches fill the time
        timed(fn, 1)
        one = timed(fn, 3)
        calls[name] = max(1, min(2000, int(args.fill_ms / max(one, 1e-3))))
    times = {k: [] for k in shapes}
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, fn in shapes.items():
            times[name].append(round(timed(fn, calls[name]), 5))
    render.film_upscale(urec, lo_mean, lo_feat, LW, LH, hi_feat, W, H, work, out, resolved)
    unresolved = float((resolved == 0).float().mean().cpu())
    ctx_hi.check()
    ctx_lo.check()

    rows, med = [], {}
    for name in shapes:
        t = times[name]
        r = {"shape": name, "frame": f"{LW}x{LH}" if name.endswith("_low") else f"{W}x{H}", "calls_per_measurement": calls[name], "ms_per_call": t,
             "median_ms": round(statistics.median(t), 5), "min_ms": min(t), "max_ms": max(t)}
        med[name] = r["median_ms"]
        if name in algorithmic_bytes:
            r["algorithmic_bytes"] = algorithmic_bytes[name]
            r["algorithmic_TBps"] = round(algorithmic_bytes[name] / (r["median_ms"] * 1e-3) / 1e12, 3)
            r["share_of_8TBps_peak"] = round(algorithmic_bytes[name] / (r["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
        if name.startswith("film_pass") or name == "features_full":
            r.update({"depth": DEPTH, "samples": SAMPLES})
        rows.append(r)
    reduced = med["film_pass_8spp_low"] + med["features_full"] + med["upscale_rotating"]
    rows.append({"shape": "summary", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
                 "sets_rotated": SETS, "low": f"{LW}x{LH}", "full": f"{W}x{H}", "unresolved_share": round(unresolved, 4),
                 "upscale_over_compare": round(med["upscale"] / med["compare"], 3),
                 "upscale_rotating_over_compare": round(med["upscale_rotating"] / med["compare"], 3),
                 "upscale_over_meter": round(med["upscale"] / med["meter"], 3),
                 "low_pass_over_full_pass": round(med["film_pass_8spp_low"] / med["film_pass_8spp_full"], 4),
                 "features_over_full_pass": round(med["features_full"] / med["film_pass_8spp_full"], 4),
                 "reduced_frame_ms": round(reduced, 5),
                 "reduced_frame_over_full_pass": round(reduced / med["film_pass_8spp_full"], 4)})
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))
    ctx_hi.close()
    ctx_lo.close()


if __name__ == "__main__":
    main()
