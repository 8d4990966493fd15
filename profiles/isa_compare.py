#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two builds' `make asm` output:
   python profiles/isa_compare.py OLD_CSRC [NEW_CSRC]     (NEW_CSRC: this tree's ascendpathtracing_amd/csrc)
Runs `make -B asm` in both directories.  For every kernel of the eight code objects -- render_kernels.s, materials.s, environment.s, film.s,
features.s, mis.s, selftest_seeded.s and denoise.s -- it compares the instruction lines
between the symbol and its .Lfunc_end (labels, directives and comments dropped; block labels renumbered per function, since a
function's index in the file moves them; differences counted by a sequence diff) and the kernel-resource-usage remarks (registers,
spills, scratch, LDS, occupancy).  Kernels of render_kernels.s are matched by symbol; those of the other files by demangled name
without the argument list, so that a kernel whose signature changed is compared with its predecessor.  A file other than
render_kernels.s and materials.s is skipped when the old build has none.
Prints one line per kernel that differs -- with whether the two bodies still hold the same instructions, each mnemonic as often as
before, i.e. differ by operands and order only -- and a summary per file.  For the files matched by name it also prints whether every kernel keeps scratch 0,
no VGPR spills and at least the old occupancy (`conditions`).  Exit status 1 when a kernel of render_kernels.s differs at all, when a
kernel of materials.s exists on one side only, or when one breaks those conditions."""
import difflib, os, re, subprocess, sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(csrc):
    r = subprocess.run(["make", "-B", "-C", csrc, "asm"], capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"make asm failed in {csrc}:\n{r.stderr[-4000:]}")
    res, cur = {}, None
    for l in r.stderr.split("\n"):
        m = re.search(r"remark:\s+(.*?)\s*\[-Rpass", l)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = res.setdefault(t.split(": ", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    return res


def kernels(path):
    out, name, body = {}, None, None
    for l in open(path):
        if name is None:
            m = re.match(r"^(_Z\S+):", l)
            if m:
                name, body = m.group(1), []
            continue
        if l.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        s = l.split(";", 1)[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*", "", d.replace("(anonymous namespace)::", "")) for n, d in zip(names, r)}


def main():
    if len(sys.argv) not in (2, 3):
        sys.exit(__doc__)
    old, new = sys.argv[1], sys.argv[2] if len(sys.argv) == 3 else os.path.join(root, "ascendpathtracing_amd", "csrc")
    with ThreadPoolExecutor(2) as ex:
        ro, rn = ex.map(build, (old, new))
    differ = 0
    for s in ("render_kernels.s", "materials.s", "environment.s", "film.s", "features.s", "mis.s", "selftest_seeded.s", "denoise.s"):
        if s not in ("render_kernels.s", "materials.s") and not os.path.exists(os.path.join(old, s)):   # an old build from before there was one
            continue
        ko, kn = kernels(os.path.join(old, s)), kernels(os.path.join(new, s))
        dm = demangle(sorted(set(ko) | set(kn)))
        by_name, broken = s != "render_kernels.s", []
        if by_name:               # symbol -> demangled name: a changed argument list still finds its predecessor
            assert len(set(dm[n] for n in ko)) == len(ko) and len(set(dm[n] for n in kn)) == len(kn), "demangled names are not unique"
            ko, kn = {dm[n]: b for n, b in ko.items()}, {dm[n]: b for n, b in kn.items()}
            so, sn = {dm.get(n, n): r for n, r in ro.items()}, {dm.get(n, n): r for n, r in rn.items()}
            dm = {n: n for n in set(ko) | set(kn)}
        else:
            so, sn = ro, rn
        same = 0
        for n in sorted(set(ko) | set(kn), key=lambda n: dm[n]):
            if n not in ko or n not in kn:
                print(f"{s}: {dm[n]}: only in {'new' if n in kn else 'old'}")
                differ += 1
                continue
            a, b = so.get(n, {}), sn.get(n, {})
            changed = [f"{k} {a.get(k)} -> {b.get(k)}" for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
            res = "  resources " + ", ".join(changed) if changed else ""
            if by_name and (b.get("ScratchSize [bytes/lane]") != "0" or b.get("VGPRs Spill") != "0"
                            or int(b.get("Occupancy [waves/SIMD]", 0)) < int(a.get("Occupancy [waves/SIMD]", 0))):
                broken.append(n)
            if ko[n] == kn[n] and not res:
                same += 1
                continue
            differ += not by_name
            ops = [o for o in difflib.SequenceMatcher(None, ko[n], kn[n]).get_opcodes() if o[0] != "equal"]
            lines = sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops)
            mnemonics = "same" if Counter(l.split()[0] for l in ko[n]) == Counter(l.split()[0] for l in kn[n]) else "DIFFERENT"
            print(f"{s}: {dm[n]}: {len(ko[n])} -> {len(kn[n])} instructions, {lines} lines in {len(ops)} hunks differ "
                  f"(first at instruction {ops[0][1] if ops else '-'}), {mnemonics} mnemonic counts{res}")
        print(f"{s}: {same} of {len(set(ko) | set(kn))} kernels identical (instructions and resources)")
        if by_name:
            print(f"{s}: conditions (scratch 0, no VGPR spills, occupancy not below the old build's): "
                  + ("kept by every kernel" if not broken else "BROKEN by " + ", ".join(broken)))
            differ += len(broken)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
