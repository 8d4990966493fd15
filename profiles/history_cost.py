#!/usr/bin/env python3
"""Temporal accumulation (include/render_mi355x_history.h): what the reprojection and the export cost at 1920x1080, beside one 8-sample
film pass and the denoiser.  Needs an MI355X (no fallback).

    python profiles/history_cost.py [--reps 5] [--out profiles/history_cost.jsonl]

The scene is open8 under the sky and the sun (tests/gpu_harness.py's), rendered from two cameras a unit apart; the history handed to
the reprojection is the previous frame's own first history.  Each shape is warmed up, then timed with device events around enough
back-to-back launches to fill about a quarter of a second, `reps` times, all shapes alternated in one process, no profiler attached;
every line carries all repetitions (ms per call), their median, minimum and maximum.  The algorithmic bytes are counted from the
shapes -- the reprojection reads 3 + 5 floats of the current frame and writes 6 per pixel, and its four taps of 5 feature and 6
history planes overlap between neighbours, so their unique traffic is 11 floats per pixel: 25 floats = 100 B per pixel; the export
reads 6 and writes 5: 44 B per pixel -- and set against a peak of 8 TB/s.  Nothing here says what bounds the kernels: that takes a
counter run of its own (rocprofv3 --kernel-trace --stats of this script with --reps 1 gives the kernel time alone)."""
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
PEAK_BYTES_PER_S = 8e12


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fill-ms", type=float, default=250.0, help="device time one measurement fills with back-to-back launches")
    ap.add_argument("--out", default=os.path.join(here, "history_cost.jsonl"))
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
    cams = [gen_data.camera(width=W, height=H, eye=(20.0 + k, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05), vfov_deg=55.0,
                            offset=0.0) for k in (0, 1)]
    p = apt.make_params(W, H, SAMPLES, depth=DEPTH, num_spheres=8, light_index=5, seed=3, flags=flags)
    render.set_environment(env)
    frames = []
    for cam in cams:
        render.set_camera(cam)
        film = render.Film(W, H)
        film.add_pass(p, d_sph, d_mat)
        frames.append((film.mean(), film.features(p, d_sph), cam))
    scratch = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    render.check_device_status()

    rec = _lib.film_history_record()
    hist0 = torch.empty((6, W, H), dtype=torch.float32, device="cuda")
    hist1 = torch.empty((6, W, H), dtype=torch.float32, device="cuda")
    render.film_history(rec, frames[0][0], frames[0][1], cams[0], hist0)
    e_film, e_mom = render.film_history_export(hist0)
    drec = _lib.film_denoise_record(2)
    work = torch.empty(_lib.denoise_lib().apt_film_denoise_work_floats(W, H), dtype=torch.float32, device="cuda")
    den = torch.empty((3, N), dtype=torch.float32, device="cuda")
    prev = (hist0, frames[0][1], cams[0])

    shapes = {
        "film_pass_8spp": lambda: render.render_frame_film(p, d_sph, d_mat, film=scratch, pass_index=1),
        "history_first_frame": lambda: render.film_history(rec, frames[1][0], frames[1][1], cams[1], hist1),
        "history_reproject": lambda: render.film_history(rec, frames[1][0], frames[1][1], cams[1], hist1, prev),
        "history_export": lambda: render.film_history_export(hist1, e_film, e_mom),
        "denoise_5_iterations": lambda: render.film_denoise(drec, e_film, e_mom, frames[1][1], W, H, work=work, out=den),
    }
    algorithmic_bytes = {"history_first_frame": (3 + 6) * 4 * N, "history_reproject": 25 * 4 * N, "history_export": 11 * 4 * N}

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
    valid = float((hist1[5] > 1).float().mean().cpu())
    times = {k: [] for k in shapes}
    for _ in range(args.reps):                       # alternated: neighbours in time see the same machine
        for name, fn in shapes.items():
            times[name].append(round(timed(fn, calls[name]), 5))
    render.check_device_status()
    render.set_camera(None)
    render.set_environment(None)

    rows = []
    for name in shapes:
        t = times[name]
        r = {"shape": name, "frame": f"{W}x{H}", "calls_per_measurement": calls[name], "ms_per_call": t, "median_ms": round(statistics.median(t), 5),
             "min_ms": min(t), "max_ms": max(t)}
        if name in algorithmic_bytes:
            r["algorithmic_bytes"] = algorithmic_bytes[name]
            r["share_of_8TBps_peak"] = round(algorithmic_bytes[name] / (r["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
        if name == "film_pass_8spp":
            r.update({"depth": DEPTH, "samples": SAMPLES})
        if name == "history_reproject":
            r["valid_pixel_fraction"] = round(valid, 4)
        rows.append(r)
    rows.append({"shape": "summary", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(),
                 "history_reproject_plus_export_over_film_pass": round((rows[2]["median_ms"] + rows[3]["median_ms"]) / rows[0]["median_ms"], 4),
                 "history_reproject_plus_export_over_denoise": round((rows[2]["median_ms"] + rows[3]["median_ms"]) / rows[4]["median_ms"], 4)})
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
