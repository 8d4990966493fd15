#!/usr/bin/env python3
"""The kernels of mis.s next to their counterparts -- the same scene form, light mode and group -- in environment.s and film.s:
registers, spills, scratch, LDS and occupancy, from the code objects' own metadata (`make asm` output; nothing is run on a GPU).

    python profiles/mis_resources.py > profiles/mis_kernel_resources.txt

Exit status 1 when a kernel of mis.s has scratch or a VGPR spill."""
import os
import re
import subprocess
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ascendpathtracing_amd", "csrc")
K_MIS, K_FILM = 256, 128


def kernels(name):
    """-> {demangled kernel name without arguments: its metadata fields and occupancy}"""
    text = open(os.path.join(CSRC, name)).read()
    occ = [int(x) for x in re.findall(r"^; Occupancy: (\d+)", text, re.M)]
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)
    out = {}
    meta = text[text.index("amdhsa.kernels:"):]
    for block in meta.split("  - .agpr_count:")[1:]:
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", block, re.M))
        d = subprocess.run(["c++filt", f["name"]], capture_output=True, text=True).stdout.strip()
        d = re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "")).replace("void ", "")
        f["occupancy"] = occ[names.index(f["name"])]
        out[d] = f
    return out


def row(f):
    return (f"{f['sgpr_count']:>5}{f['vgpr_count']:>5}{f['sgpr_spill_count']:>7}{f['vgpr_spill_count']:>7}{f['private_segment_fixed_size']:>8}"
            f"{f['group_segment_fixed_size']:>7}{f['occupancy']:>6}")


def main():
    subprocess.run(["make", "-s", "-C", CSRC, "mis.s", "environment.s", "film.s"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    mis, env, film = kernels("mis.s"), kernels("environment.s"), kernels("film.s")
    head = f"{'SGPR':>5}{'VGPR':>5}{'sSpill':>7}{'vSpill':>7}{'scratch':>8}{'LDS':>7}{'waves':>6}"
    print(f"{'kernel of mis.s':<38}{head}   counterpart{head}")
    bad = 0
    for n in sorted(mis, key=lambda n: (n.split("<")[0], [int(x) for x in re.findall(r"\d+", n)])):
        if not n.startswith(("render_frame_mat_kernel", "render_paths_mat_kernel")):
            continue
        scn = int(re.search(r"<(\d+)", n).group(1))
        other = n.replace(f"<{scn}", f"<{scn & ~K_MIS}")
        src, name = (film, "film.s") if scn & K_FILM else (env, "environment.s")
        print(f"{n:<38}{row(mis[n])}   {name + ' ' + other:<11}{row(src[other])}")
        bad += mis[n]["private_segment_fixed_size"] != "0" or mis[n]["vgpr_spill_count"] != "0"
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
