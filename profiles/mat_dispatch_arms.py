#!/usr/bin/env python3
"""Which kernel does each arm of the material launch path run?  Images cannot tell: the tile and the grid form render the same image,
and so do the gloss and the plain kernels on a table without gloss words.  A kernel trace can.

    rocprofv3 --kernel-trace -f csv -d DIR -o NAME -- python profiles/mat_dispatch_arms.py         (needs an MI355X)
    python profiles/mat_dispatch_arms.py --pair OLD_kernel_trace.csv NEW_kernel_trace.csv [CSRC]   (no GPU; CSRC after `make asm`)

The first form makes exactly one call per arm at 16x16, where samples 1 and 8 select the two groups, and prints one label per call:
  72 frame + 18 buffer arms without an environment: 3 scene forms x {plain, APT_FLAG_NEE, a light table} x gloss flag or none,
                                                     frames also x 2 groups x camera or none;
  18 frame +  9 buffer arms with an environment:    3 scene forms x 3 light modes, frames x 2 groups (no camera, APT_FLAG_GLOSS set);
  18 film arms, each at pass 0 and pass 1:          the same 18, with neither a camera nor an environment set.
The scenes are built as tests/test_gpu_environment.py builds its own: 8 open spheres, 40 (one LDS tile), 220 behind a vouched grid.  It starts no
child and replaces no program.  Run it on two builds of the library (APT_LIB_PATH names another one) under the tracer; the second
form then keeps the render_frame_mat_kernel / render_paths_mat_kernel rows of both traces and prints the paired list
(profiles/mat_dispatch_trace.txt).  Exit status 1 unless the two ordered lists are equal line for line, there is one row per call,
and the distinct kernels are exactly those of materials.s, environment.s and film.s."""
import csv
import os
import re
import subprocess
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
FORMS = [("8", "open8", False), ("tiles", "open40", False), ("grid", "open220", True)]
MODES = ["plain", "nee", "table"]


def calls():
    """-> (label, kind, arguments) of every call, in the order they are made."""
    out = []
    for env in (False, True):
        for form in FORMS:
            for mode in MODES:
                for gloss in ((True,) if env else (False, True)):
                    for s_ in (1, 8):
                        for cam in ((False,) if env else (False, True)):
                            out.append((f"frame env={int(env)} form={form[0]} mode={mode} gloss={int(gloss)} samples={s_} camera={int(cam)}",
                                        "frame", (form, mode, gloss, s_, cam, env, None)))
                    out.append((f"paths env={int(env)} form={form[0]} mode={mode} gloss={int(gloss)}", "paths", (form, mode, gloss, 1, False, env, None)))
    for form in FORMS:
        for mode in MODES:
            for s_ in (1, 8):
                for k in (0, 1):
                    out.append((f"film pass={k} form={form[0]} mode={mode} samples={s_}", "film", (form, mode, True, s_, False, False, k)))
    return out


def scene(apt, gd, name, grid):
    """The scenes of tests/test_gpu_environment.py, built here: gen_spheres_open with two of its DIFF balls as lamps; gen_scene_open(40)
    and (220) with two small lamps and every second mirror as rough metal.  -> device tensors, the flags of the two tables, the grid."""
    import numpy as np
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if name == "open8":
        ns, lamps = 8, [5, 4]
        sph, mat = gd.gen_spheres_open()
        sph = gd.with_lamps(sph, ns, lamps, radius=8.0, emission=[(30.0, 20.0, 10.0), 12.0])
        mat = np.array(mat, dtype=np.int32)
    else:
        ns = 40 if name == "open40" else 220
        lamps = [7, 19] if ns == 40 else [11, 97]
        sph, mat = gd.gen_scene_open(ns, seed=2)
        sph = gd.with_lamps(sph, ns, lamps, radius=[1.5, 2.0], emission=[(40.0, 30.0, 20.0), 25.0])
        mat = np.array(mat, dtype=np.int32)
        for i in np.nonzero(mat == apt.MAT_SPEC)[0][::2]:
            mat[i] = gd.gloss((600 + (int(i) * 977) % 64000) / 65536.0)
    sph = np.asarray(sph, dtype=np.float32)
    plain = mat.copy()
    plain[(plain & 0xFF) == apt.MAT_GLOSS] = apt.MAT_SPEC                  # the gloss-free table: those spheres are mirrors
    sc = dict(ns=ns, light=lamps[0], sph=dev(sph), mat={True: dev(mat), False: dev(plain)},
              flags={True: gd.materials_flags(mat), False: gd.materials_flags(plain)},
              table=dev(gd.build_lights(sph, ns, lamps).view(np.int32)), accel=0, grid_flags=0)
    assert sc["flags"] == {True: apt.APT_FLAG_GLOSS, False: 0}
    if grid:
        hgrid = gd.build_grid(sph, ns)
        sc["grid"] = dev(hgrid.view(np.int32))
        sc["accel"], sc["grid_flags"] = sc["grid"].data_ptr(), gd.grid_flags(hgrid, ns)
        assert sc["grid_flags"] == apt.APT_FLAG_GRID_SLOTS                  # a vouched grid
    return sc


def run():
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import ascendpathtracing_amd as apt
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    env = gen_data.environment(horizon=(0.5, 0.6, 0.7), zenith=(0.1, 0.3, 0.9), sun_dir=(0.4, 0.8, 0.45), sun_radiance=(30.0, 28.0, 24.0),
                               sun_angle_deg=8.0, sample_sun=True)
    lens = gen_data.camera(width=W, height=H, aperture=1.5, eye=(50.0, 45.0, 210.0), target=(50.0, 10.0, 60.0), up=(0.05, 1.0, 0.0),
                           vfov_deg=42.0, offset=0.0)
    rays = torch.from_numpy(np.ascontiguousarray(gen_data.gen_rays(W, H, 1, seed=0).ravel())).cuda()
    film = torch.zeros((3, W * H), dtype=torch.float32, device="cuda")
    scenes = {name: scene(apt, gen_data, name, grid) for _, name, grid in FORMS}
    for label, kind, ((_, name, _), mode, gloss, s_, cam, with_env, k) in calls():
        sc = scenes[name]
        flags = (apt.APT_FLAG_NEE if mode == "nee" else 0) | sc["grid_flags"] | sc["flags"][gloss]
        p = apt.make_params(W, H, s_, depth=3, num_spheres=sc["ns"], light_index=sc["light"], seed=7, flags=flags, accel=sc["accel"])
        mat, lights = sc["mat"][gloss], sc["table"] if mode == "table" else None
        render.set_camera(lens if cam else None)
        render.set_environment(env if with_env else None)
        try:
            if kind == "frame":
                render.render_frame(p, sc["sph"], materials=mat, lights=lights)
            elif kind == "paths":
                render.render_paths(p, rays, sc["sph"], materials=mat, lights=lights)
            else:
                render.render_frame_film(p, sc["sph"], mat, film=film, pass_index=k, lights=lights)
        finally:
            render.set_camera(None)
            render.set_environment(None)
        print(label, flush=True)
    torch.cuda.synchronize()
    render.check_device_status()
    print(f"{len(calls())} calls made through {_lib.LIB_PATH}, the status word is clean")


KERNEL = re.compile(r"(render_(?:frame|paths)_mat_kernel<[^>]*>)")


def trace_names(path):
    """The material kernels of a rocprofv3 kernel trace, in dispatch order, as `kernel<arguments>` without blanks."""
    rows = list(csv.DictReader(open(path, newline="")))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    names = (KERNEL.search(r["Kernel_Name"]) for r in rows)
    return [m.group(1).replace(" ", "") for m in names if m]


def listed_names(csrc):
    syms = []
    for s in ("materials.s", "environment.s", "film.s"):
        syms += re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(os.path.join(csrc, s)).read(), re.M)
    dem = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    names = [KERNEL.search(d) for d in dem]
    return [m.group(1).replace(" ", "") for m in names if m]


def pair(old, new, csrc):
    labels = [c[0] for c in calls()]
    a, b, listed = trace_names(old), trace_names(new), listed_names(csrc)
    for i in range(max(len(labels), len(a), len(b))):
        x, y = (a[i] if i < len(a) else "-"), (b[i] if i < len(b) else "-")
        print(f"{labels[i] if i < len(labels) else '-':64s} {x:36s} {y:36s} {'same' if x == y else 'DIFFERENT'}")
    ok_rows = len(a) == len(b) == len(labels)
    ok_same = a == b
    ok_names = len(listed) == len(set(listed)) and set(b) == set(listed) and set(a) == set(listed)
    print(f"calls {len(labels)}, rows old {len(a)}, new {len(b)}: {'one row per call' if ok_rows else 'NOT one row per call'}")
    print(f"ordered lists: {'equal line for line' if ok_same else 'DIFFERENT'}")
    print(f"distinct kernels: old {len(set(a))}, new {len(set(b))}, in the three listings {len(listed)}: {'the same set' if ok_names else 'NOT the same set'}")
    return 0 if ok_rows and ok_same and ok_names else 1


if __name__ == "__main__":
    if len(sys.argv) == 1:
        run()
    elif sys.argv[1] == "--pair" and len(sys.argv) in (4, 5):
        sys.exit(pair(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) == 5 else os.path.join(root, "ascendpathtracing_amd", "csrc")))
    else:
        sys.exit(__doc__)
