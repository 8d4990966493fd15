#!/usr/bin/env python3
"""Writes tests/golden/restatement_hashes.json: per case of tests/test_restatement_frozen.py the SHA-256 of the colours and of the
bad-material mask that THE RESTATEMENT (tests/materials_ref.py) gives, and its segment count.

    python tests/golden/make_restatement_hashes.py [OUT.json]

The committed file was first written from the six modules the restatement once was, each case through the module that owned it, and
this script's output was byte-identical to it.  A record of APT_FLAG_MIS that the flag does not reach would hold nothing: the script
fails unless every room case's colours differ from those of the same case traced with mis=False.  Run it again only when the header's arithmetic changes on purpose: the file is what
holds the restatement, which every GPU test of the material kernels compares against, to what it computed before.  The case list, the
scenes, the rays and the digest are the test's own, so there is one list.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_restatement_frozen as fz  # noqa: E402


def main():
    from gpu_harness import load_host
    from oracle import oracle
    pkg = load_host()
    gen_data = pkg.gen_data
    world = {**fz.scenes(gen_data), **fz.mis_scenes(pkg)}
    results = {}
    for case in fz.cases():
        for depth, rr in fz.variants(case):
            results[fz.key(case[0], depth, rr)] = d = fz.restated(gen_data, oracle, world, case, depth, rr)
            if case[2].startswith("harness/"):
                assert d["L"] != fz.restated(gen_data, oracle, world, case, depth, rr, mis=False)["L"], (case[0], depth, rr)
    out = sys.argv[1] if len(sys.argv) > 1 else fz.HASHES
    with open(out, "w") as f:
        f.write(fz.dump(results))
    print("wrote %d cases to %s" % (len(results), out))


if __name__ == "__main__":
    main()
