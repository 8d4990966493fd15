#!/usr/bin/env python3
"""The material frame kernels of this tree against the parent commit's, frame by frame.  Needs an MI355X (no fallback).

    python profiles/materials_ab.py --parent-lib PARENT/librender_mi355x.so [--reps 6] [--out profiles/mat_record_ab.json]

For a change that claims "the material kernels cost what they cost": the parent's library is loaded next to this tree's and both are
driven through the same C-ABI calls (apt_render_frame_materials / apt_render_frame_lights / apt_set_camera: unchanged), in the manner of
profiles/materials_lights.py, whose scene builders this takes.  1920x1080, samples 16 (64 spp, GROUP 8), depth 8; HIP events around each
frame, one warm-up per case and library, then parent and new alternated `reps` times, synchronised after every frame.  Twelve cases:
the 8-sphere scene, the 9-sphere demo scene (tiles) and the 10 000-sphere scene through its grid (APT_FLAG_GRID_SLOTS), each with no light
sampling, with APT_FLAG_NEE and with a light table; the demo scene with a thin-lens camera; the demo scene with APT_FLAG_GLOSS; the
10 000-sphere scene with a light table and the thin-lens camera (the grid + table + camera kernel, whose SGPR spills moved most).
Per case: every time, both spreads (max - min), new median - parent median, and `within`: that difference does not exceed the parent's
own spread in this alternation -- the smallest difference this run can tell from noise.  Exit status 1 when a case is not within."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, SAMPLES, DEPTH = 1920, 1080, 16, 8
NS_BIG, SEED_BIG = 10000, 1


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="librender_mi355x.so built from the parent commit")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(here, "mat_record_ab.json"))
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data
    _lib.require_gpu()
    libs = {"parent": ctypes.CDLL(os.path.abspath(args.parent_lib)), "new": _lib.lib()}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def scene(sph, mat, light, use_grid):
        ns = int(mat.size)
        table = dev(sph)
        grid = gen_data.build_grid_device(table, ns) if use_grid else None      # from the table it serves
        return dict(sph=table, mat=dev(mat), ns=ns, light=light, grid=grid, gflags=gen_data.grid_flags(grid, ns) if use_grid else 0,
                    lights=dev(gen_data.build_lights(sph, ns, [light]).view(np.int32)))

    s9, m9 = gen_data.gen_spheres_materials()
    scenes = {"diff8": scene(gen_data.gen_spheres(), np.array([1, 1, 1, 1, 1, 1, 0, 1], dtype=np.int32), 7, False),
              "demo9": scene(s9, m9, 7, False),
              "grid10k": scene(*gen_data.gen_scene_materials(NS_BIG, seed=SEED_BIG), NS_BIG - 1, True)}
    gloss9 = dict(scenes["demo9"], mat=dev(gen_data.gen_spheres_materials(gloss=0.25)[1]))
    lens = gen_data.camera(eye=(20.0, 60.0, 160.0), target=(70.0, 20.0, 60.0), vfov_deg=55.0, offset=0.0, aperture=2.5, width=W, height=H)

    def params(sc, flags=0):
        return apt.make_params(W, H, SAMPLES, depth=DEPTH, num_spheres=sc["ns"], light_index=sc["light"], seed=0,
                               accel=sc["grid"].data_ptr() if sc["grid"] is not None else 0, flags=sc["gflags"] | flags)

    cases = {}                                       # name -> (scene, params, light table?, camera)
    for name, sc in scenes.items():
        cases[name + "_off"] = (sc, params(sc), False, None)
        cases[name + "_nee"] = (sc, params(sc, apt.APT_FLAG_NEE), False, None)
        cases[name + "_table"] = (sc, params(sc), True, None)
    cases["demo9_lens"] = (scenes["demo9"], params(scenes["demo9"]), False, lens)
    cases["demo9_gloss"] = (gloss9, params(gloss9, apt.APT_FLAG_GLOSS), False, None)
    cases["grid10k_table_lens"] = (scenes["grid10k"], params(scenes["grid10k"]), True, lens)

    fb_buf = torch.empty((3, W * H), dtype=torch.float32, device="cuda")
    u8_buf = torch.empty((W * H, 3), dtype=torch.uint8, device="cuda")
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64

    def frame(lib, sc, p, table, cam):
        st = vp(torch.cuda.current_stream().cuda_stream)
        if cam is not None:
            assert lib.apt_set_camera(ctypes.byref(cam)) == 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if table:
            rc = lib.apt_render_frame_lights(ctypes.byref(p), st, vp(sc["sph"].data_ptr()), vp(sc["mat"].data_ptr()), vp(sc["lights"].data_ptr()),
                                             u64(0), u64(W * H), vp(fb_buf.data_ptr()), vp(u8_buf.data_ptr()))
        else:
            rc = lib.apt_render_frame_materials(ctypes.byref(p), st, vp(sc["sph"].data_ptr()), vp(sc["mat"].data_ptr()), u64(0), u64(W * H),
                                                vp(fb_buf.data_ptr()), vp(u8_buf.data_ptr()))
        b.record()
        torch.cuda.synchronize()
        if cam is not None:
            assert lib.apt_set_camera(None) == 0
        assert rc == 0, rc
        return a.elapsed_time(b)

    rows, bad = [], 0
    for name, case in cases.items():
        for lib in libs.values():                    # warm-up: code objects
            frame(lib, *case)
        t = {k: [] for k in libs}
        for _ in range(args.reps):                   # alternated: neighbours in time see the same machine
            for k, lib in libs.items():
                t[k].append(round(frame(lib, *case), 3))
        for lib in libs.values():
            assert lib.apt_check(None) == 0, "device status"
        med = {k: round(statistics.median(v), 3) for k, v in t.items()}
        spread = {k: round(max(v) - min(v), 3) for k, v in t.items()}
        diff = round(med["new"] - med["parent"], 3)
        rows.append({"case": name, "frame": f"{W}x{H}", "samples": SAMPLES, "depth": DEPTH, "parent_ms": t["parent"], "new_ms": t["new"],
                     "parent_median_ms": med["parent"], "new_median_ms": med["new"], "parent_spread_ms": spread["parent"],
                     "new_spread_ms": spread["new"], "new_minus_parent_ms": diff, "within": bool(diff <= spread["parent"])})
        bad += not rows[-1]["within"]
        print(json.dumps(rows[-1]), flush=True)
    out = {"device": torch.cuda.get_device_name(0), "build_id": _lib.build_id(), "reps": args.reps,
           "scene_grid10k": f"gen_scene_materials({NS_BIG}, seed={SEED_BIG})", "cases": rows}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
