#!/usr/bin/env python3
"""Which material kernels did a run launch?  The tests compare images, and images cannot tell which instantiation made them: a kernel
trace can.

    rocprofv3 --kernel-trace -f csv -d DIR -o NAME -- python -m pytest tests/test_gpu_material_matrix.py -q -m gpu      (needs an MI355X)
    python profiles/kernel_coverage.py DIR/.../NAME_kernel_trace.csv [more traces] [--out LIST.txt] [--csrc CSRC] [--rows]   (no GPU; after `make asm`)

The second form reads the Kernel_Name column of the traces, keeps the material render kernels -- render_frame_mat_kernel<SCN, GROUP>,
render_paths_mat_kernel<SCN>, features_kernel<SC> -- written as the ISA names them, and compares the set with the .amdhsa_kernel
names of materials.s, environment.s, film.s and features.s.  It prints the kernels of the code objects that the traces never saw,
writes the sorted list of those they saw to LIST.txt, and exits with status 1 unless every kernel was seen.
--rows (one trace, of tests/test_gpu_material_matrix.py alone): also holds the trace's material dispatches, in dispatch order, to the
kernels that the file's rows claim to launch, one by one (claimed_dispatches())."""
import csv
import os
import re
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = re.compile(r"((?:render_frame_mat_kernel|render_paths_mat_kernel|features_kernel)<[^>]*>)")
CODE_OBJECTS = ("materials", "environment", "film", "features")


def _name(text):
    m = KERNEL.search(text)
    return None if m is None else re.sub(r"\s*,\s*", ", ", m.group(1).replace(" ", ""))


def ordered(path):
    """The material kernels of one trace in dispatch order."""
    rows = sorted(csv.DictReader(open(path, newline="")), key=lambda r: int(r["Dispatch_Id"]))
    return [n for n in (_name(r["Kernel_Name"]) for r in rows) if n]


def traced(paths):
    """-> {kernel: dispatches} over the traces."""
    seen = {}
    for path in paths:
        for n in ordered(path):
            seen[n] = seen.get(n, 0) + 1
    return seen


def rows_differ(path):
    """-> the number of places where the trace and the matrix's claimed dispatches differ (a length difference counts)."""
    sys.path[:0] = [root, os.path.join(root, "tests")]
    from test_gpu_material_matrix import claimed_dispatches
    got, want = ordered(path), claimed_dispatches()
    bad = [i for i in range(min(len(got), len(want))) if got[i] != want[i]]
    for i in bad[:10]:
        print(f"dispatch {i}: traced {got[i]}, the row claims {want[i]}")
    print(f"{len(got)} material dispatches traced, {len(want)} claimed by the rows: {'equal one by one' if not bad and len(got) == len(want) else 'DIFFERENT'}")
    return len(bad) + abs(len(got) - len(want))


def listed(csrc):
    """-> {kernel: code object} from the assembly listings."""
    out = {}
    for co in CODE_OBJECTS:
        syms = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(os.path.join(csrc, co + ".s")).read(), re.M)
        dem = subprocess.run(["c++filt"], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        for d in dem:
            n = _name(d)
            if n:
                assert out.setdefault(n, co) == co, n
    return out


def main(argv):
    out, csrc, traces, rows = None, os.path.join(root, "ascendpathtracing_amd", "csrc"), [], False
    it = iter(argv)
    for a in it:
        if a == "--out":
            out = next(it)
        elif a == "--csrc":
            csrc = next(it)
        elif a == "--rows":
            rows = True
        else:
            traces.append(a)
    if not traces:
        sys.exit(__doc__)
    seen, want = traced(traces), listed(csrc)
    if out:
        with open(out, "w") as f:
            f.write("".join(n + "\n" for n in sorted(seen)))
    missing = sorted(set(want) - set(seen), key=lambda n: (want[n], n))
    unknown = sorted(set(seen) - set(want))
    for co in CODE_OBJECTS:
        have = [n for n in want if want[n] == co]
        print(f"{co}.s: {sum(n in seen for n in have)} of {len(have)} kernels launched")
    for n in missing:
        print(f"never launched: {want[n]}.s {n}")
    for n in unknown:
        print(f"launched but in no listing: {n}")
    print(f"{len(set(seen) & set(want))} of {len(want)} material kernels launched, {sum(seen.values())} dispatches")
    differ = rows_differ(traces[0]) if rows else 0
    return 1 if missing or unknown or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
