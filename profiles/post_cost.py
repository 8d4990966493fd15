#!/usr/bin/env python3
"""Metering and bloom (include/render_mi355x_post.h): what the histogram and the bloom pyramid cost at 1920x1080, beside one 8-sample
film pass and the 5-iteration denoiser.  Needs an MI355X (no fallback).

    python profiles/post_cost.py [--reps 5] [--out profiles/post_cost.jsonl] [--atomics-lib profiles/microbench/libpost_atomics.so]

--atomics-lib: a build of libpost_mi355x.so with -DAPT_POST_METER_ATOMICS (post.hip: hist cleared on the stream, every workgroup adds
its 257 sums with 32-bit integer global atomics, no work rows and no second launch), timed beside the product's meter as
"meter_global_atomics" after its histogram was compared with the product's.  Made by compiling post.hip with the Makefile's HIPFLAGS
and that macro into an object of its own and linking it with post_host.o as the Makefile links the product.

The scene is open8 under the sky and the sun (tests/gpu_harness.py's); the metered and bloomed film is a film of two 8-sample passes
of it.  "meter_constant" is the same launch over an image of ONE value: every lane of every wave adds to the same LDS word, the worst
case of the sub-histograms.  Each shape is warmed up, then timed with device events around enough back-to-back launches to fill about a
quarter of a second, `reps` times, all shapes alternated in one process, no profiler attached; every line carries all repetitions (ms
per call), their median, minimum and maximum.  The algorithmic bytes are counted from the shapes -- the meter reads 3 floats a pixel
(its work rows and the 257 words are below 1 MB); the bloom's first down step reads the film once (its 16 taps overlap between
neighbours) and writes a 16-byte record per level-0 pixel, a later down step reads the level before and writes its own, a combine
reads and writes its own level and reads the coarser one, the composite reads the film and level 0 and writes 3 floats a pixel -- and
set against a peak of 8 TB/s.  The whole film (25 MB) and every pyramid level fit the 256 MiB last-level cache, and back-to-back
launches over the same buffers find them there: the shares say how the time compares with the bytes, not that HBM delivered them.
Nothing here says what bounds the kernels: that takes a counter run of its own."""
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
BLOOM_LEVELS = (1, 3, 5)


def bloom_bytes(levels):
    sizes, w, h = [], W, H
    for _ in range(levels):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        sizes.append(w * h)
    total = 12 * N + 16 * sizes[0]                                   # down from the film
    total += sum(16 * sizes[j - 1] + 16 * sizes[j] for j in range(1, levels))
    total += sum(2 * 16 * sizes[j] + 16 * sizes[j + 1] for j in range(levels - 1))
    return total + 12 * N + 16 * sizes[0] + 12 * N                   # the composite


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fill-ms", type=float, default=250.0, help="device time one measurement fills with back-to-back launches")
    ap.add_argument("--out", default=os.path.join(here, "post_cost.jsonl"))
    ap.add_argument("--atomics-lib", default=None, help="a libpost_mi355x.so built with -DAPT_POST_METER_ATOMICS")
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
    render.set_environment(env)
    render.set_camera(cam)
    film = render.Film(W, H, moments=True)
    film.add_pass(p, d_sph, d_mat)
    film.add_pass(p, d_sph, d_mat)
    feat = film.features(p, d_sph)
    scratch = torch.zeros((3, N), dtype=torch.float32, device="cuda")
    constant = torch.full((3, N), 0.37, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    render.check_device_status()

    mrec = _lib.film_meter_record(film.passes)
    mwork = torch.empty(_lib.post_lib().apt_film_meter_work_words(N), dtype=torch.int32, device="cuda")
    hist = torch.empty(_lib.APT_METER_WORDS, dtype=torch.int32, device="cuda")
    brecs = {L: _lib.film_bloom_record(film.passes, levels=L) for L in BLOOM_LEVELS}
    bwork = torch.empty(_lib.post_lib().apt_film_bloom_work_floats(W, H, max(BLOOM_LEVELS)), dtype=torch.float32, device="cuda")
    bout = torch.empty((3, N), dtype=torch.float32, device="cuda")
    drec = _lib.film_denoise_record(film.passes)
    dwork = torch.empty(_lib.denoise_lib().apt_film_denoise_work_floats(W, H), dtype=torch.float32, device="cuda")
    den = torch.empty((3, N), dtype=torch.float32, device="cuda")

    shapes = {
        "film_pass_8spp": lambda: render.render_frame_film(p, d_sph, d_mat, film=scratch, pass_index=1),
        "meter": lambda: render.film_meter(mrec, film.buffer, mwork, hist),
        "meter_constant": lambda: render.film_meter(mrec, constant, mwork, hist),
        "denoise_5_iterations": lambda: render.film_denoise(drec, film.buffer, film.moments, feat, W, H, work=dwork, out=den),
    }
    for L in BLOOM_LEVELS:
        shapes["bloom_%d_levels" % L] = (lambda L=L: render.film_bloom(brecs[L], film.buffer, W, H, bwork, bout))
    algorithmic_bytes = {"meter": 12 * N, "meter_constant": 12 * N}
    if args.atomics_lib:
        import ctypes
        entry = ctypes.CDLL(os.path.abspath(args.atomics_lib)).apt_film_meter_device
        entry.restype, entry.argtypes = _lib.POST_PROTOTYPES["apt_film_meter_device"]
        hist2 = torch.empty(_lib.APT_METER_WORDS, dtype=torch.int32, device="cuda")

        def meter_atomics(planes):
            rc = entry(ctypes.byref(mrec), torch.cuda.current_stream().cuda_stream, planes.data_ptr(), N, mwork.data_ptr(), hist2.data_ptr())
            assert rc == 0, rc

        for planes in (film.buffer, constant):       # the same histogram as the product's, before anything is timed
            meter_atomics(planes)
            assert torch.equal(hist2, render.film_meter(mrec, planes, mwork, hist)), "the atomics build counts differently"
        shapes["meter_global_atomics"] = lambda: meter_atomics(film.buffer)
        shapes["meter_global_atomics_constant"] = lambda: meter_atomics(constant)
        algorithmic_bytes.update({"meter_global_atomics": 12 * N, "meter_global_atomics_constant": 12 * N})
    algorithmic_bytes.update({"bloom_%d_levels" % L: bloom_bytes(L) for L in BLOOM_LEVELS})

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
    exposure = render.film_exposure(mrec, render.film_meter(mrec, film.buffer, mwork, hist))
    above = float((film.mean().mul(torch.tensor([[0.2126], [0.7152], [0.0722]], device="cuda")).sum(0) > 1.0).float().mean().cpu())
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
            r["share_of_8TBps_peak"] = round(algorithmic_bytes[name] / (r["median_ms"] * 1e-3) / PEAK_BYTES_PER_S, 4)
        if name == "film_pass_8spp":
            r.update({"depth": DEPTH, "samples": SAMPLES})
        rows.append(r)
    rows.append({"shape": "summary", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
                 "metered_exposure": exposure, "pixels_above_the_bloom_threshold": round(above, 4),
                 "meter_plus_bloom_5_levels_over_film_pass": round((med["meter"] + med["bloom_5_levels"]) / med["film_pass_8spp"], 4),
                 "meter_plus_bloom_5_levels_over_denoise": round((med["meter"] + med["bloom_5_levels"]) / med["denoise_5_iterations"], 4)})
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
