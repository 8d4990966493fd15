#!/usr/bin/env python3
"""Temporal accumulation (include/render_mi355x_history.h): what the history is worth on the run tests/test_gpu_history.py asserts its
benefit condition on.  Needs an MI355X (no fallback).

    python profiles/history_benefit.py [--out profiles/history_benefit.txt]

open8 under the sky and the sun at 48 x 32, 1-sample frames (seeds 40, 41, ...) from an eye that starts at (20, 60, 160) and moves a
unit along x per frame, the target (70, 20, 60) fixed, pushed through render.History with the default record.  After each frame: the
clipped MSE (radiance clipped to [0, 1], as the resolve's clip) of the history's radiance, and of the history denoised through
denoise_inputs() and film_denoise(passes = 2), each over the clipped MSE of that frame alone -- over all pixels and over those whose
first surface is DIFF --, and the share of reset pixels.  The reference of a frame is a 64-pass film from that frame's camera."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, DEPTH, FRAMES, REF_PASSES = 48, 32, 4, 12, 64


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "history_benefit.txt"))
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    sph, mat = gen_data.gen_spheres_open()
    sph = gen_data.with_lamps(sph, 8, [5, 4], radius=8.0, emission=[(30.0, 20.0, 10.0), 12.0])
    d_sph, d_mat = dev(sph), dev(mat)
    render.set_environment(gen_data.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45),
                                                sun_radiance=(30.0, 28.0, 24.0), sun_angle_deg=8.0, sample_sun=True))
    table = np.asarray(sph, dtype=np.float32)[:80].reshape(10, 8)
    diff_spheres = [s for s in range(8) if int(mat[s]) == _lib.MAT_DIFF]

    def mse(a, ref, mask):
        d = np.clip(a.astype(np.float64), 0, 1) - np.clip(ref.astype(np.float64), 0, 1)
        return float((d[:, mask] ** 2).mean())

    history, film, ref_film = render.History(W, H), render.Film(W, H), render.Film(W, H)
    drec = _lib.film_denoise_record(2)
    lines = ["# frame  reset_share  diff_pixels  history/frame: all  diff   denoised history/frame: all  diff"]
    for k in range(FRAMES):
        cam = gen_data.camera(width=W, height=H, eye=(20.0 + k, 60.0, 160.0), target=(70.0, 20.0, 60.0), up=(0.1, 1.0, 0.05), vfov_deg=55.0,
                              offset=0.0)
        render.set_camera(cam)
        p = apt.make_params(W, H, 1, depth=DEPTH, num_spheres=8, light_index=5, seed=40 + k, flags=gen_data.materials_flags(mat))
        film.reset()
        film.add_pass(p, d_sph, d_mat)
        mean, feat = film.mean(), film.features(p, d_sph)
        history.push(mean, feat, cam)
        ref_film.reset()
        q = p.copy(seed=1000)
        for _ in range(REF_PASSES):
            ref_film.add_pass(q, d_sph, d_mat)
        e_film, e_mom = history.denoise_inputs()
        den = render.film_denoise(drec, e_film, e_mom, feat, W, H)
        torch.cuda.synchronize()
        render.check_device_status()
        ref, frame, hist, den, f = (t.cpu().numpy() for t in (ref_film.mean(), mean, history.radiance(), den, feat))
        diff = np.zeros(W * H, dtype=bool)
        for s in diff_spheres:
            diff |= (f[0] == 1) & np.all(f[5:8] == table[7:10, s][:, None], axis=0)
        every = np.ones(W * H, dtype=bool)
        reset = float((history.length() == 1).float().mean().cpu())
        lines.append("%5d  %.4f  %5d  %.4f  %.4f  %.4f  %.4f" % (k, reset, diff.sum(), mse(hist, ref, every) / mse(frame, ref, every),
                                                                  mse(hist, ref, diff) / mse(frame, ref, diff), mse(den, ref, every) / mse(frame, ref, every),
                                                                  mse(den, ref, diff) / mse(frame, ref, diff)))
    render.set_camera(None)
    render.set_environment(None)
    lines.append("# device: %s, build %s" % (torch.cuda.get_device_name(0), _lib.build_id()))
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
