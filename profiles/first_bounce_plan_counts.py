#!/usr/bin/env python3
"""The gate of the first-bounce plan (csrc/pt_first_plan.h), on the CPU: over the whole C2 frame (1920 x 1080, pixel q = column q / h,
row q % h, a wave traces pixels 2k and 2k + 1), the share of the waves in which the plan leaves each sphere out -- what both pixels
allow -- from the plan's CPU twin (libfirstplan_mi355x.so), priced with the per-sphere instruction counts of the first-bounce block
in `make render_kernels.s` (ISA below; recount them when the block changes).  Writes profiles/first_bounce_plan_counts.json.
    python profiles/first_bounce_plan_counts.py"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, DEPTH = 1920, 1080, 8
# VALU instructions of sphere k's block behind its plan branch in the first pair-bounce (own-coordinate terms, b, c, disc, its
# v_minimum3_f32 pair, the stage with its two v_mov_b32; ball and light: terms, b, c, disc and the 4-instruction joint test -- their
# stage is behind the joint test already and runs in 3 % / 16 % of the first bounces)
ISA = {0: 24, 1: 28, 3: 26, 4: 28, 5: 28, 6: 20, 7: 14}
# what the plan form adds to EVERY first pair-bounce: the walls' |disc| enter `amin` singly (6 v_minimum3_f32 more than the paired form)
ADDED = 6


def main():
    from ascendpathtracing_amd import gen_data
    L = ctypes.CDLL(os.path.join(ROOT, "ascendpathtracing_amd", "libfirstplan_mi355x.so"))
    L.apt_first_plan_mask_host.restype = ctypes.c_uint32
    sph = np.ascontiguousarray(gen_data.gen_spheres(), dtype=np.float32)
    rec = np.zeros(16, dtype=np.int32)
    assert L.apt_first_plan_host(ctypes.c_uint32(W), ctypes.c_uint32(H), ctypes.c_void_p(sph.ctypes.data), ctypes.c_double(1e-4), None,
                                 ctypes.c_void_p(rec.ctypes.data)) == 0
    # first_plan_mask is separable: a column part and a row part (checked against the twin on a sample below)
    c, j = np.arange(W)[:, None], np.arange(H)[None, :]
    inside = (c >= rec[0]) & (c < rec[1]) & (j >= rec[2]) & (j < rec[3])
    m = np.zeros((W, H), dtype=np.uint32)
    m |= np.where(inside & (rec[8] != 0), 8, 0).astype(np.uint32)
    m |= np.where(inside & (c >= W - rec[4]), 1, 0).astype(np.uint32)
    m |= np.where(inside & (c < rec[5]), 2, 0).astype(np.uint32)
    m |= np.where(inside & (j >= H - rec[6]), 16, 0).astype(np.uint32)
    m |= np.where(inside & (j < rec[7]), 32, 0).astype(np.uint32)
    m |= np.where((c < rec[9]) | (c >= W - rec[10]) | (j < rec[11]) | (j >= H - rec[12]), 64, 0).astype(np.uint32)
    m |= np.where((j < rec[13]) & (c >= 0), 128, 0).astype(np.uint32)
    rng = np.random.default_rng(0)
    for cc, jj in zip(rng.integers(0, W, 4000), rng.integers(0, H, 4000)):
        assert L.apt_first_plan_mask_host(ctypes.c_void_p(rec.ctypes.data), W, H, int(cc), int(jj)) == m[cc, jj]
    q = m.ravel()                                  # pixel q = c * H + j
    waves = q[0::2] & q[1::2]
    shares = {k: float(((waves >> k) & 1).mean()) for k in ISA}
    per_pair = {k: shares[k] * ISA[k] for k in ISA}
    segments = 2 * DEPTH                           # a path pair's segments
    out = {
        "what": "gate of the first-bounce plan: wave shares over the C2 frame from the plan's CPU twin, priced with the listing's per-sphere counts",
        "frame": [W, H], "record": [int(v) for v in rec],
        "wave_share_sphere_left_out": {str(k): round(v, 4) for k, v in shares.items()},
        "valu_per_sphere_block": {str(k): v for k, v in ISA.items()},
        "valu_added_per_first_pair_bounce": ADDED,
        "predicted_valu_saved_per_segment_by_sphere": {str(k): round(v / segments, 3) for k, v in per_pair.items()},
        "predicted_valu_saved_per_segment": round((sum(per_pair.values()) - ADDED) / segments, 3),
        "gate": "build when the total is >= 2.0 per segment; drop a sphere below 0.2",
    }
    out["gate_passed"] = out["predicted_valu_saved_per_segment"] >= 2.0 and all(v >= 0.2 for v in out["predicted_valu_saved_per_segment_by_sphere"].values())
    with open(os.path.join(ROOT, "profiles", "first_bounce_plan_counts.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
