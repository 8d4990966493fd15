#!/usr/bin/env python3
"""What guided film upscaling (include/render_mi355x_upscale.h) does to the error of a frame, read by Film.compare on the device at
256 x 192 from 128 x 96, on the two scenes of profiles/quality_table.py (the lamp room under APT_FLAG_NEE, open8 under the sky and the
sun) against 1024-pass full-size references of another seed.  Needs an MI355X (no fallback).  It changes and tunes nothing: every
record is its library's default.

    python profiles/upscale_quality.py [--out profiles/upscale_quality.jsonl]

The camera is tests/gpu_harness.py's inside_pinhole at both sizes; passes are 1 sample (4 paths a pixel) of depth 4; the films under
test are of seed 11, the feature planes of 1 sample.  Rows, each with clipped_mse, rel_mse, ssim (and psnr, mse, mae, bad) against the
reference, and the unresolved share where an upscale ran:
  full_4_passes                  a 4-pass full-size film
  low_16_upscaled                a 16-pass low film (the same number of paths) through Upscaler.upscale
  low_16_refined                 the same, then Upscaler.refine(passes=4): the unresolved pixels from 4 full-size list passes
  low_16_bilinear_demodulated    the same low film with every sigma 0 (g = 1: bilinear interpolation of the demodulated illumination)
  low_4_upscaled                 a 4-pass low film (a quarter of the paths)
  low_4_refined                  the same, refined
  low_16_denoised_upscaled,
  low_4_denoised_upscaled        each low film through Film.denoise (5 iterations, default sigmas) before the upscale
ONE run, ONE seed: the table says what the metrics read on these frames, not which setting wins."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, LW, LH, DEPTH, REF_PASSES, REF_SEED, SEED, REFINE_PASSES = 256, 192, 128, 96, 4, 1024, 977, 11, 4


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "upscale_quality.jsonl"))
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
    camera = lambda w, h: gen_data.camera(width=w, height=h, eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05),
                                          vfov_deg=55.0, offset=0.0)
    rows = []
    for name, sph, mat, light, flags, env in scenes:
        d_sph, d_mat = dev(sph), dev(np.asarray(mat, dtype=np.int32))
        params = lambda w, h, seed: apt.make_params(w, h, 1, depth=DEPTH, num_spheres=8, light_index=light, seed=seed, flags=flags)
        ctx_hi, ctx_lo = render.Context(), render.Context()
        for ctx, (w, h) in ((ctx_hi, (W, H)), (ctx_lo, (LW, LH))):
            ctx.set_environment(env)
            ctx.set_camera(camera(w, h))
        p_hi, p_lo = params(W, H, SEED), params(LW, LH, SEED)

        ref = render.Film(W, H)
        for _ in range(REF_PASSES):
            ref.add_pass(params(W, H, REF_SEED), d_sph, d_mat, context=ctx_hi)
        full = render.Film(W, H)
        for _ in range(4):
            full.add_pass(p_hi, d_sph, d_mat, context=ctx_hi)
        hi_feat = full.features(p_hi, d_sph, context=ctx_hi)

        def row(label, source=None, **more):
            d = full.compare(ref, source=source)
            rows.append(dict({"scene": name, "row": label, "frame": f"{W}x{H}", "low": f"{LW}x{LH}"}, **more, **d))

        row("full_4_passes", passes=4)
        for low_passes in (16, 4):
            low = render.Film(LW, LH, moments=True)
            for _ in range(low_passes):
                low.add_pass(p_lo, d_sph, d_mat, context=ctx_lo)
            lo_feat = low.features(p_lo, d_sph, context=ctx_lo)
            up = render.Upscaler(W, H, LW, LH)
            out = up.upscale(low.mean(), lo_feat, hi_feat)
            share = round(float((up.resolved == 0).float().mean().cpu()), 4)
            row(f"low_{low_passes}_upscaled", source=out, passes=low_passes, unresolved_share=share)
            count = up.refine(p_hi, d_sph, d_mat, passes=REFINE_PASSES, context=ctx_hi)
            row(f"low_{low_passes}_refined", source=up.out, passes=low_passes, refine_passes=REFINE_PASSES, unresolved_share=share,
                refined_pixels=count)
            if low_passes == 16:
                flat = render.Upscaler(W, H, LW, LH, sigma_n=0.0, sigma_z=0.0, sigma_c=0.0, sigma_a=0.0)
                out = flat.upscale(low.mean(), lo_feat, hi_feat)
                row("low_16_bilinear_demodulated", source=out, passes=low_passes,
                    unresolved_share=round(float((flat.resolved == 0).float().mean().cpu()), 4))
            den = low.denoise(p_lo, d_sph, features=lo_feat, context=ctx_lo)
            out = up.upscale(den, lo_feat, hi_feat)
            row(f"low_{low_passes}_denoised_upscaled", source=out, passes=low_passes,
                unresolved_share=round(float((up.resolved == 0).float().mean().cpu()), 4))
        ctx_hi.check()
        ctx_lo.check()
        ctx_hi.close()
        ctx_lo.close()
    rows.append({"row": "meta", "device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reference_passes": REF_PASSES,
                 "reference_seed": REF_SEED, "seed": SEED, "depth": DEPTH, "refine_passes": REFINE_PASSES})
    with open(args.out, "w") as fh:
        for r in rows:
            fh.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()
