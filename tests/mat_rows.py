"""What the row matrices of the material kernels share (tests/test_gpu_material_matrix.py, test_gpu_mis.py, test_gpu_film_list.py): the
routing restated once, the kernel names of a code object, and a row's camera rays.  A plain module beside gpu_harness.py, imported the
same way; each matrix keeps its own rows, classes and launches."""
import os
import re
import shutil
import subprocess

import pytest

import camera_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ascendpathtracing_amd", "csrc")

# The bits of a material kernel's SCN; the scene form (0: 8 spheres in SGPRs, 1: LDS tiles, 2: a grid) is the two lowest.
NEE, TABLE, CAMERA, GLOSS, ENV, FILM, MIS, LIST = 4, 8, 16, 32, 64, 128, 256, 512


def mat_kernel(entry, ns, grid, mode, samples, gloss=True, camera=False, env=False, mis=False, listed=False):
    """materials.hip's routing and pt_mat_launch.h's scene form -> (code object, the kernel as the ISA names it) of the launch through
    `entry` ("frame", "film", "paths" or "features") of `ns` spheres in light mode `mode`; gloss / camera / env / mis / listed: the
    launch carries APT_FLAG_GLOSS / has a camera / has an environment / is routed by APT_FLAG_MIS / carries a pixel list.  Only
    materials.hip instantiates by gloss and camera: every other code object pins them (a flagless launch of those is data)."""
    form = 0 if ns == 8 else (2 if grid else 1)
    if entry == "features":
        return "features", f"features_kernel<{form}>"
    assert not mis or mode != "plain"
    scn = form | {"plain": 0, "nee": NEE, "table": TABLE}[mode]
    if entry == "paths":
        if mis:
            return "mis", f"render_paths_mat_kernel<{scn | GLOSS | ENV | MIS}>"
        if env:
            return "environment", f"render_paths_mat_kernel<{scn | GLOSS | ENV}>"
        return "materials", f"render_paths_mat_kernel<{scn | (GLOSS if gloss else 0)}>"
    assert entry in ("frame", "film") and (entry == "film" or not listed)
    if listed:
        co, scn = "film_list", scn | CAMERA | GLOSS | ENV | FILM | LIST | (MIS if mis else 0)
    elif mis:
        co, scn = "mis", scn | CAMERA | GLOSS | ENV | MIS | (FILM if entry == "film" else 0)
    elif entry == "film":
        co, scn = "film", scn | CAMERA | GLOSS | ENV | FILM
    elif env:
        co, scn = "environment", scn | CAMERA | GLOSS | ENV
    else:
        co, scn = "materials", scn | (CAMERA if camera else 0) | (GLOSS if gloss else 0)
    return co, f"render_frame_mat_kernel<{scn}, {8 if samples >= 8 else 1}>"


needs_hipcc = pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or shutil.which("c++filt") is None,
                                 reason="needs hipcc and c++filt")


def _kernel_name(demangled):
    """'void (anonymous namespace)::render_frame_kernel<0, 0, 8, false, true>(float const*, ...)' -> 'render_frame_kernel<0, 0, 8, false, true>'"""
    s = demangled.strip()
    if s.startswith("void "):
        s = s[5:]
    s = s.replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(s):                # cut the parameter list: the first '(' outside the template argument list
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            return s[:i]
    return s


def code_object_kernels(co):
    """The kernels of csrc/<co>.hip as the ISA names them, demangled -> a set.  Kernel names only: no instruction is looked at."""
    subprocess.run(["make", "-s", "-C", CSRC, co + ".s"], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = open(os.path.join(CSRC, co + ".s")).read()
    mangled = sorted(set(re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M)))
    assert mangled, co
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return {_kernel_name(d) for d in demangled}


def rays_of(q, cam, seed):
    """The camera rays [6][n] of the launch `q` (an oracle.Params) at `seed` -- q.seed, or a film pass's: the reference camera's, or
    camera_ref.rays of the camera record `cam`."""
    from oracle import oracle
    if cam is None:
        q = oracle.Params.from_buffer_copy(bytes(q))
        q.seed = seed
        return oracle.gen_rays_counter(q)
    return cr.rays(cr.from_ctypes(cam), q.width, q.height, q.samples, seed=seed)
