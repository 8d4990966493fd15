#!/usr/bin/env python3
"""Film comparison metrics (include/render_mi355x_metrics.h): what compare and SSIM cost at 1920x1080, beside the meter (the yardstick:
one pass over ONE film, where compare reads two) and one 8-sample film pass.  Needs an MI355X (no fallback).

    python profiles/metrics_cost.py [--reps 5] [--out profiles/metrics_cost.jsonl]

The scene is open8 under the sky and the sun (tests/gpu_harness.py's); the compared films are two films of two 8-sample passes each,
of different seeds.  Each shape is warmed up, then timed with device events around enough back-to-back launches to fill about a
quarter of a second, `reps` times, all shapes alternated in one process, no profiler attached; every line carries all repetitions (ms
per call), their median, minimum and maximum.  The algorithmic bytes are counted from the shapes -- the meter reads 3 floats a pixel,
compare 6 (its rows are below 100 KB) and with err_map writes 1, SSIM reads 6 a pixel once (a pixel is read by up to 4 tiles; the
overlap is not counted), writes a float a window and reads it again for the sum -- and set against a peak of 8 TB/s.

Both films (50 MB) fit the 256 MiB last-level cache, and back-to-back launches over the same buffers find them there: those shares say
how the time compares with the bytes, not that HBM delivered them.  The "_rotating" shapes take another of 8 film pairs (400 MB, more
than the cache) at every launch, so that a launch finds little of its input there; they are the ones to read for a film that was just
rendered by something else.  Nothing here says what bounds the kernels: that takes a counter run of its own."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, DEPTH, SAMPLES = 1920, 1080, 4, 8
N = W * H
WINDOWS = (W - 10) * (H - 10)
PEAK_BYTES_PER_S = 8e12
PAIRS = 8


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fill-ms", type=float, default=250.0, help="device time one measurement fills with back-to-back launches")
    ap.add_argument("--out", default=os.path.join(here, "metrics_cost.jsonl"))
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
    cam = gen_data.camera(width=W, height=H, eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05), vfov_deg=55.0, offset=0.0)
    p = apt.make_params(W, H, SAMPLES, depth=DEPTH, num_spheres=8, light_index=5, seed=3, flags=flags)
    p_ref = p.copy(seed=4)
    render.set_environment(env)
    render.set_camera(cam)
    film, ref = render.Film(W, H), render.Film(W, H)
    for _ in range(2):
        film.add_pass(p, d_sph, d_mat)
        ref.add_pass(p_ref, d_sph, d_mat)
    scratch = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    many_a = [film.buffer.clone() for _ in range(PAIRS)]
    many_b = [ref.buffer.clone() for _ in range(PAIRS)]
    torch.cuda.synchronize()
    render.check_device_status()

    M = _lib.metrics_lib()
    rec = _lib.film_compare_record(film.passes, ref.passes)
    cwork = torch.empty(M.apt_film_compare_work_doubles(N), dtype=torch.float64, device="cuda")
    cres = torch.empty(_lib.APT_COMPARE_WORDS, dtype=torch.int64, device="cuda")
    emap = torch.empty(N, dtype=torch.float32, device="cuda")
    swork = torch.empty((M.apt_film_ssim_work_bytes(W, H) + 7) // 8, dtype=torch.float64, device="cuda")
    sres = torch.empty(_lib.APT_SSIM_WORDS, dtype=torch.int64, device="cuda")
    smap = torch.empty(WINDOWS, dtype=torch.float32, device="cuda")
    mrec = _lib.film_meter_record(film.passes)
    mwork = torch.empty(_lib.post_lib().apt_film_meter_work_words(N), dtype=torch.int32, device="cuda")
    hist = torch.empty(_lib.APT_METER_WORDS, dtype=torch.int32, device="cuda")
    turn = {"meter": 0, "compare": 0, "ssim": 0}
    every_film = many_a + many_b

    def rotating(kind):
        if kind == "meter":                          # one film a launch: all 16 films in turn, the same 400 MB
            k = turn[kind] = (turn[kind] + 1) % (2 * PAIRS)
            return render.film_meter(mrec, every_film[k], mwork, hist)
        k = turn[kind] = (turn[kind] + 1) % PAIRS
        if kind == "compare":
            return render.film_compare(rec, many_a[k], many_b[k], cwork, cres)
        return render.film_ssim(rec, many_a[k], many_b[k], W, H, swork, sres)

    shapes = {
        "film_pass_8spp": lambda: render.render_frame_film(p, d_sph, d_mat, film=scratch, pass_index=1),
        "meter": lambda: render.film_meter(mrec, film.buffer, mwork, hist),
        "compare": lambda: render.film_compare(rec, film.buffer, ref.buffer, cwork, cres),
        "compare_err_map": lambda: render.film_compare(rec, film.buffer, ref.buffer, cwork, cres, emap),
        "ssim": lambda: render.film_ssim(rec, film.buffer, ref.buffer, W, H, swork, sres),
        "ssim_map": lambda: render.film_ssim(rec, film.buffer, ref.buffer, W, H, swork, sres, smap),
        "meter_rotating": lambda: rotating("meter"),
        "compare_rotating": lambda: rotating("compare"),
        "ssim_rotating": lambda: rotating("ssim"),
    }
    algorithmic_bytes = {"meter": 12 * N, "meter_rotating": 12 * N, "compare": 24 * N, "compare_rotating": 24 * N, "compare_err_map": 28 * N,
                         "ssim": 24 * N + 8 * WINDOWS, "ssim_map": 24 * N + 8 * WINDOWS, "ssim_rotating": 24 * N + 8 * WINDOWS}

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
    summary = render.compare_summary(render.film_compare(rec, film.buffer, ref.buffer, cwork, cres),
                                     render.film_ssim(rec, film.buffer, ref.buffer, W, H, swork, sres))
    times = {k: [] for k in shapes}
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, fn in shapes.items():
            times[name].append(round(timed(fn, calls[name]), 5))
    render.check_device_status()
    render.set_camera(None)
    render.set_environment(None)

    rows, med = [], {}
    for name in shapes:
        t = times[name]
        r = {"shape": name, "frame": f"{W}x{H}", "calls_per_measurement": calls[name], "ms_per_call": t, "median_ms": round(statistics.median(t), 5),
             "min_ms": min(t), "max_ms": max(t)}
        med[name] = r["median_ms"]
        if name in algorithmic_bytes:
            r["algorithmic_bytes"] = algorithmic_bytes[name]
            r["algorithmic_TBps"] = round(algorithmic_bytes[name] / (r["median_ms"] * 1e-3) / 1e12, 3)
            r["share_of_8TBps_peak"] = round(algorithmic_bytes[name] / (r["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
        if name == "film_pass_8spp":
            r.update({"depth": DEPTH, "samples": SAMPLES})
        rows.append(r)
    rows.append({"shape": "summary", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
                 "film_pairs_rotated": PAIRS, "compared": {k: v for k, v in summary.items()},
                 "compare_over_meter": round(med["compare"] / med["meter"], 3),
                 "compare_rotating_over_meter_rotating": round(med["compare_rotating"] / med["meter_rotating"], 3),
                 "ssim_over_meter": round(med["ssim"] / med["meter"], 3),
                 "ssim_rotating_over_meter_rotating": round(med["ssim_rotating"] / med["meter_rotating"], 3),
                 "compare_plus_ssim_over_film_pass": round((med["compare"] + med["ssim"]) / med["film_pass_8spp"], 4)})
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
