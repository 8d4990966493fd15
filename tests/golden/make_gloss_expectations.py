#!/usr/bin/env python3
"""Writes tests/golden/gloss_expectations.json: the float64 expectations of tests/gloss_physics.py for its eight rays in gloss8 and
gloss9, at the midpoint rule's resolution N_QUAD, and next to each its own error -- the difference to resolution 2 N_QUAD.  No GPU.

    python tests/golden/make_gloss_expectations.py

tests/test_gloss_cpu.py recomputes `expect` (equal to 1e-12) and holds `quad_err` below a fifth of the estimator's standard error for
every component; the GPU test reads the file."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import gloss_physics as gp  # noqa: E402


def main():
    rays8 = gp.rays()
    doc = {"made_by": "tests/golden/make_gloss_expectations.py", "n_quad": gp.N_QUAD, "fractions": list(gp.FRACTIONS), "depth": gp.DEPTH,
           "layout": "[channel][ray]", "scenes": {}}
    for name in ("gloss8", "gloss9"):
        scene = getattr(gp, name)()
        coarse, fine = gp.expectation(rays8, scene, gp.N_QUAD), gp.expectation(rays8, scene, 2 * gp.N_QUAD)
        err = abs(coarse - fine)
        doc["scenes"][name] = {"alpha": gp.alpha_of(scene), "expect": coarse.tolist(), "quad_err": err.tolist()}
        print(name, "largest |E_n - E_2n| = %.3g" % err.max())
    with open(gp.FIXTURE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
