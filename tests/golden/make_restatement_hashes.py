#!/usr/bin/env python3
"""Writes tests/golden/restatement_hashes.json: per case of tests/test_restatement_frozen.py the SHA-256 of the colours and of the
bad-material mask that THE RESTATEMENT (tests/materials_ref.py) gives, and its segment count.

    python tests/golden/make_restatement_hashes.py [OUT.json]

The committed file was first written from the five modules the restatement once was, each case through the module that owned it, and
this script's output was byte-identical to it.  Run it again only when the header's arithmetic changes on purpose: the file is what
holds the restatement, which every GPU test of the material kernels compares against, to what it computed before.  The case list, the
scenes, the rays and the digest are the test's own, so there is one list.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_restatement_frozen as fz  # noqa: E402


def main():
    import __graft_entry__ as g
    g.build()
    from ascendpathtracing_amd import gen_data
    from oracle import oracle
    world = fz.scenes(gen_data)
    results = {fz.key(case[0], depth, rr): fz.restated(gen_data, oracle, world, case, depth, rr) for case in fz.cases() for depth, rr in fz.VARIANTS}
    out = sys.argv[1] if len(sys.argv) > 1 else fz.HASHES
    with open(out, "w") as f:
        f.write(fz.dump(results))
    print("wrote %d cases to %s" % (len(results), out))


if __name__ == "__main__":
    main()
