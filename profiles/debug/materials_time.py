"""Kernel time of the material renderer at the C2 shape (1920x1080, samples 64 = 256 spp, depth 8) next to the mirror kernel, in one run.

    python profiles/debug/materials_time.py [--reps 7] [--out profiles/r07_materials_c2.jsonl]

HIP-event time of one render_frame call after a warm-up call, `reps` repetitions per case; prints and appends one JSON line per case
(median, min, max, spread = (max - min) / median, ns per traced segment from the trace counter of one extra call).  Cases:
  demo9_materials   the 9-sphere demo scene (walls and light DIFF, mirror SPEC, glass REFR) -- the LDS-tile form
  diff8_materials   the reference's 8 spheres with DIFF walls and light, the mirror SPEC -- the 8-sphere form
  mirror_8          the same shape through today's mirror kernel (render_frame without materials)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    g.build()
    import ascendpathtracing_amd as apt
    from ascendpathtracing_amd import gen_data, render
    apt._lib.require_gpu()
    w, h, s, d = a.width, a.height, a.samples, a.depth
    npix = w * h
    fb = torch.empty((3, npix), dtype=torch.float32, device="cuda")
    u8 = torch.empty((npix, 3), dtype=torch.uint8, device="cuda")
    demo_s, demo_m = gen_data.gen_spheres_materials()
    sph8 = gen_data.gen_spheres()
    cases = [("demo9_materials", demo_s, demo_m, 9), ("diff8_materials", sph8, np.array([1, 1, 1, 1, 1, 1, 0, 1], np.int32), 8),
             ("mirror_8", sph8, None, 8)]
    rows = []
    for name, sph, mat, ns in cases:
        p = apt.make_params(w, h, s, depth=d, num_spheres=ns, light_index=7, seed=1)
        d_sph = torch.from_numpy(sph).cuda()
        d_mat = None if mat is None else torch.from_numpy(np.ascontiguousarray(mat)).cuda()
        render.render_frame(p, d_sph, fb=fb, fb_u8=u8, materials=d_mat)       # warm-up
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            render.render_frame(p, d_sph, fb=fb, fb_u8=u8, materials=d_mat)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        with render.TraceCounter() as tc:                                     # segments actually traced (paths end at a miss)
            render.render_frame(p, d_sph, fb=fb, fb_u8=u8, materials=d_mat)
        render.check_device_status()
        t = np.array(times)
        med = float(np.median(t))
        row = dict(case=name, width=w, height=h, samples=s, spp=4 * s, depth=d, reps=a.reps, ms_median=round(med, 3),
                   ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3), spread=round(float((t.max() - t.min()) / med), 4),
                   segments_traced=tc.value, segments_nominal=npix * 4 * s * d,
                   ns_per_segment=round(med * 1e6 / tc.value, 5) if tc.value else None,
                   image_mean=[round(float(x), 5) for x in fb.mean(dim=1).tolist()], device=torch.cuda.get_device_name(0))
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
