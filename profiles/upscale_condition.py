#!/usr/bin/env python3
"""The one quality condition of guided upscaling (DESIGN.md "Upscale"), checked on the CPU with the restatements alone
(tests/materials_ref.py, tests/upscale_ref.py): after the unresolved pixels were refined, is the clipped MSE of the upscaled frame
against a many-pass full-size reference of another seed below that of the SAME low film upsampled by plain bilinear interpolation
(the restatement with g dropped and no demodulation)?  No GPU; the device gives the restatement's bits (tests/test_gpu_upscale.py).

    python profiles/upscale_condition.py > profiles/upscale_condition.txt

gen_spheres_open() under the sky and the sun from tests/gpu_harness.py's inside_pinhole; a low film of 4 passes (seed 40), features of
1 sample (seed 3), 4 full-size refine passes (seed 50), depth 4, a reference of seed 1000; at 1 and at 16 samples a pass.  One seed
each: figures, not a ranking.  Nothing is asserted and no default follows from it."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import camera_ref as cr  # noqa: E402
import features_ref as ft  # noqa: E402
import film_ref as fr  # noqa: E402
import materials_ref as mr  # noqa: E402
import upscale_ref as ur  # noqa: E402
from gpu_harness import Scene, inside_pinhole, load_host, oracle_params, sky_and_sun  # noqa: E402

F = np.float32
PASSES, DEPTH = 4, 4


def run(apt, sc, menv, LW, LH, W, H, samples, ref_passes):
    rec_lo, rec_hi = cr.from_ctypes(inside_pinhole(apt, LW, LH)), cr.from_ctypes(inside_pinhole(apt, W, H))
    p_lo, p_hi, p_ref = sc.params(LW, LH, samples, DEPTH, seed=40), sc.params(W, H, samples, DEPTH, seed=50), sc.params(W, H, 1, DEPTH, seed=1000)
    rays = lambda rec, w, h, s: (lambda seed: cr.rays(rec, w, h, s, seed=seed))
    render = lambda p, rec, w, h, s, k: fr.render_pass(oracle_params(p), sc.sph, sc.mat, env=menv, pass_index=k, rays=rays(rec, w, h, s))[0]
    mean = (fr.accumulate([render(p_lo, rec_lo, LW, LH, samples, k) for k in range(PASSES)]) / F(PASSES)).astype(F)
    lf, hf = ft.planes(rec_lo, LW, LH, 1, 3, sc.sph, sc.ns, 1e-4), ft.planes(rec_hi, W, H, 1, 3, sc.sph, sc.ns, 1e-4)
    up, res, _ = ur.upscale(ur.DEFAULTS, mean, lf, LW, LH, hf, W, H)
    lst = np.flatnonzero(res == 0)
    sums = fr.accumulate([render(p_hi, rec_hi, W, H, samples, k)[:, lst] for k in range(PASSES)])
    refined = ur.patch(sums, lst.astype(np.uint32), PASSES, up)
    plain = ur.upscale(ur.DEFAULTS, mean, lf, LW, LH, hf, W, H, plain=True)[0]
    ref = fr.accumulate([render(p_ref, rec_hi, W, H, 1, k) for k in range(ref_passes)]).astype(np.float64) / ref_passes
    cm = lambda a: float(((np.clip(a.astype(np.float64), 0, 1) - np.clip(ref, 0, 1)) ** 2).mean())
    print("%2d x %2d from %2d x %2d, %2d samples a pass, reference %3d passes: unresolved %.4f; clipped_mse guided %.4e, refined %.4e, "
          "plain bilinear %.4e; refined / plain %.3f" % (W, H, LW, LH, samples, ref_passes, lst.size / (W * H), cm(up), cm(refined), cm(plain),
                                                         cm(refined) / cm(plain)))


def main():
    apt = load_host()
    sph, mat = apt.gen_data.gen_spheres_open()
    sc = Scene(apt, sph, mat, 8)
    menv = mr.Env.from_ctypes(sky_and_sun(apt))
    for samples in (1, 16):
        run(apt, sc, menv, 16, 12, 32, 24, samples, 256)
        run(apt, sc, menv, 32, 24, 64, 48, samples, 256 if samples == 1 else 128)


if __name__ == "__main__":
    main()
