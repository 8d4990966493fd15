#!/usr/bin/env python3
"""What adaptive sampling gains, on the CPU restatement (tests/adaptive_ref.py, tests/film_ref.py): no GPU.
   python profiles/adaptive_benefit.py > profiles/adaptive_benefit.txt
The scene and the error are DESIGN "Denoise"'s: the diffuse closed room with its lamp under APT_FLAG_NEE, 32 x 24, depth 4, 1 sample
(4 paths) per pixel and pass; the reference is one pass of 256 samples (1024 paths per pixel, seed 977); the error is the mean squared
error of the means clipped to [0, 1].  For each base seed an adaptive film -- min_passes uniform passes, then rounds of select / list
pass / accumulate, the list pass of round r being the whole pass min_passes + r gathered at the list, exactly as Film.add_adaptive_pass
does it -- runs until it has spent at least BUDGET pixel-passes, and is compared with the uniform film of ceil(spent / N) passes of the
same seed: the uniform film never has fewer paths.  One line per (min_passes, max_passes, threshold, floor): the ratio adaptive /
uniform clipped MSE per seed, their geometric mean, and how many seeds it is below 1 on."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import adaptive_ref as ar  # noqa: E402
import film_ref as fr  # noqa: E402

W, H, DEPTH, SEEDS, BUDGET_PASSES, MAX_ROUNDS = 32, 24, 4, (11, 12, 13, 14, 15, 16, 17, 18), 16, 96
D = np.float64


def main():
    from oracle import oracle
    from ascendpathtracing_amd import gen_data
    n = W * H
    sph = gen_data.with_lamp(gen_data.gen_spheres(), 8, 7)
    mat = np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32)
    mk = lambda s, seed: oracle.make_params(width=W, height=H, samples=s, depth=DEPTH, num_spheres=8, light_index=7, seed=seed, flags=32)
    ref = fr.render_pass(mk(256, 977), sph, mat)[0].astype(D)
    clip = lambda a: np.clip(a, 0, 1)
    mse = lambda a: float(np.mean((clip(a.astype(D)) - clip(ref)) ** 2))
    passes = {s: [fr.render_pass(mk(1, s), sph, mat, pass_index=k)[0] for k in range(MAX_ROUNDS + 8)] for s in SEEDS}
    uniform = {s: [None] + [mse(ar.mean(fr.accumulate(passes[s][:k]), k)) for k in range(1, MAX_ROUNDS + 8)] for s in SEEDS}
    print("uniform clipped MSE by passes (mean over seeds): " + "  ".join("%d: %.6f" % (k, np.mean([uniform[s][k] for s in SEEDS])) for k in (2, 4, 8, 16, 32)))
    print("min max threshold floor | adaptive / uniform clipped MSE per seed | geometric mean | seeds below 1 | pixel-passes spent / N (mean) | rounds (mean)")
    for lo in (2, 4, 8):
        for hi_mul in (4, 16):
            for thr in (0.025, 0.05, 0.1, 0.2):
                for floor in (1 / 64, 1 / 16, 1 / 4):
                    hi = lo * hi_mul
                    ratios, spent_all, rounds_all = [], [], []
                    for s in SEEDS:
                        ps = passes[s]
                        film, mom, extra = fr.accumulate(ps[:lo]), ar.moments_of(ps[:lo]), np.zeros(n, dtype=np.uint32)
                        spent, r = lo * n, 0
                        while spent < BUDGET_PASSES * n and r < MAX_ROUNDS:
                            lst = ar.select(mom, extra, base=lo, min_passes=lo, max_passes=hi, threshold=thr, floor=floor)
                            if lst.size == 0:
                                break
                            film, mom, extra = ar.accumulate_list(ar.list_pass(ps[lo + r], lst), lst, film, mom, extra)
                            spent += lst.size
                            r += 1
                        u = max(lo, math.ceil(spent / n))
                        ratios.append(mse(ar.mean(film, lo, extra)) / uniform[s][u])
                        spent_all.append(spent / n)
                        rounds_all.append(r)
                    gm = math.exp(np.mean(np.log(ratios)))
                    print("%d %3d %.3f %.4f | %s | %.3f | %d of %d | %.2f | %.1f" % (lo, hi, thr, floor, " ".join("%.3f" % x for x in ratios), gm,
                                                                                   sum(x < 1 for x in ratios), len(SEEDS), np.mean(spent_all), np.mean(rounds_all)))


if __name__ == "__main__":
    main()
