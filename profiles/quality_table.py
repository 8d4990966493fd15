#!/usr/bin/env python3
"""A quality table made on the device by Film.compare (include/render_mi355x_metrics.h), at a size the host-side MSE copies never
reached: 256 x 192 on the lamp room (the diffuse closed room under smallpt's small lamp, APT_FLAG_NEE) and on open8 under the sky and
the sun.  Needs an MI355X (no fallback).  It changes and tunes nothing: every record is its library's default.

    python profiles/quality_table.py [--out profiles/quality_table.jsonl]

Both scenes are seen by the look-at camera of tests/gpu_harness.py's inside_pinhole, eye (20, 60, 160), target (70, 20, 60); passes are 1
sample (4 paths a pixel) of depth 4.  The reference of a camera is a 1024-pass film of seed 977; the films under test are of seed 11.
Rows, each with clipped_mse, rel_mse, ssim (and psnr, mse, mae, bad) against the reference:
  film_4_passes            a 4-pass film
  film_4_passes_denoised   the same film through Film.denoise (5 iterations, default sigmas)
  adaptive                 4 uniform passes, then Film.add_adaptive_pass rounds (default record) until at least 16 pixel-passes a
                           pixel are spent (or nothing is selected, or 96 rounds)
  uniform_equal_paths      the uniform film of ceil(spent / N) passes of the same seed: never fewer paths than the adaptive one
  moved_frame_alone        after the eye moved a unit along x per frame for 3 frames: the 4th frame's 4-pass film alone ...
  moved_history            ... and the History (default record) that was pushed the four frames' means, against the 4th camera's reference
ONE run, ONE seed: the table says what the metrics read on these films, not which setting wins."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, DEPTH, REF_PASSES, REF_SEED, SEED, BUDGET_PASSES, MAX_ROUNDS, FRAMES = 256, 192, 4, 1024, 977, 11, 16, 96, 4
N = W * H


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "quality_table.jsonl"))
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    lamp_sph = gen_data.with_lamp(gen_data.gen_spheres(), 8, 7)
    lamp_mat = np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    open_sph, open_mat = gen_data.gen_spheres_open()
    open_sph = gen_data.with_lamps(open_sph, 8, [5, 4], radius=8.0, emission=[(30.0, 20.0, 10.0), 12.0])
    sky = gen_data.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(30.0, 28.0, 24.0),
                               sun_angle_deg=8.0, sample_sun=True)
    scenes = [("lamp_room", lamp_sph, lamp_mat, 7, _lib.APT_FLAG_NEE, None),
              ("open8_sky", open_sph, open_mat, 5, gen_data.materials_flags(open_mat), sky)]
    camera = lambda k: gen_data.camera(width=W, height=H, eye=(20.0 + k, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05),
                                       vfov_deg=55.0, offset=0.0)
    rows = []
    for name, sph, mat, light, flags, env in scenes:
        d_sph, d_mat = dev(sph), dev(np.asarray(mat, dtype=np.int32))
        params = lambda seed: apt.make_params(W, H, 1, depth=DEPTH, num_spheres=8, light_index=light, seed=seed, flags=flags)
        render.set_environment(env)

        def reference(k):
            render.set_camera(camera(k))
            ref = render.Film(W, H)
            for _ in range(REF_PASSES):
                ref.add_pass(params(REF_SEED), d_sph, d_mat)
            return ref

        def row(label, film, ref, source=None, **more):
            d = film.compare(ref, source=source)
            rows.append(dict({"scene": name, "row": label, "frame": f"{W}x{H}"}, **more, **d))

        ref0 = reference(0)
        render.set_camera(camera(0))
        p = params(SEED)
        film = render.Film(W, H, moments=True)
        for _ in range(4):
            film.add_pass(p, d_sph, d_mat)
        row("film_4_passes", film, ref0, passes=4)
        row("film_4_passes_denoised", film, ref0, source=film.denoise(p, d_sph), passes=4)

        adaptive = render.Film(W, H, moments=True, adaptive=True)
        for _ in range(4):
            adaptive.add_pass(p, d_sph, d_mat)
        spent, rounds = 4 * N, 0
        while spent < BUDGET_PASSES * N and rounds < MAX_ROUNDS:
            count = adaptive.add_adaptive_pass(p, d_sph, d_mat)
            if count == 0:
                break
            spent += count
            rounds += 1
        row("adaptive", adaptive, ref0, passes=4, rounds=rounds, pixel_passes_per_pixel=round(spent / N, 3))
        u = max(4, math.ceil(spent / N))
        uniform = render.Film(W, H)
        for _ in range(u):
            uniform.add_pass(p, d_sph, d_mat)
        row("uniform_equal_paths", uniform, ref0, passes=u)

        history = render.History(W, H)
        frame = render.Film(W, H)
        for k in range(FRAMES):
            cam = camera(k)
            render.set_camera(cam)
            q = params(SEED + 100 + k)
            frame.reset()
            for _ in range(4):
                frame.add_pass(q, d_sph, d_mat)
            history.push(frame.mean(), frame.features(q, d_sph), cam)
        ref_moved = reference(FRAMES - 1)
        row("moved_frame_alone", frame, ref_moved, passes=4, frames=FRAMES)
        reset = float((history.length() == 1).float().mean().cpu())
        row("moved_history", frame, ref_moved, source=history.radiance().contiguous(), passes=4, frames=FRAMES, reset_share=round(reset, 4))
        render.check_device_status()
        render.set_camera(None)
        render.set_environment(None)
    rows.append({"row": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reference_passes": REF_PASSES,
                 "reference_seed": REF_SEED, "seed": SEED, "depth": DEPTH, "budget_passes": BUDGET_PASSES})
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
