#!/usr/bin/env python3
"""How often a whole wave of the headline launch cannot hit either sphere of a pair.  Needs an MI355X and the counting build:

    bash profiles/build_variant.sh pair_count -DAPT_COUNT_PAIR_SKIP
    APT_LIB_PATH=profiles/microbench/lib_pair_count.so python profiles/pair_skip_count.py [--out profiles/pair_skip_counts.json]

One C2 frame (bench.py's headline launch, render_frame_kernel<0, 0, 8, false, true>) with a 128-entry statistics block: the counting
build (pt_trace2.h, APT_COUNT_PAIR_SKIP) adds one to entry [4 + (half * 8 + bounce) * 4 + pair] for every wave in which
pair_misses_wave() holds -- both discriminants of the pair negative or NaN in all 64 lanes -- and one to entry [68] per wave and path pair it traces (the denominator).
`--general`: the bench's general scene (spheres 0 and 6 exchanged), the non-shared-planes arm.
The price model of the table: a pair's root stage is 15 VALU + 2 v_rsq_f32 = 78 cycles, the test 2 VALU = 8 cycles, a pair-bounce 1250
cycles, so a pair pays for itself from P = 0.10 on."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

W, H, S, DEPTH = 1920, 1080, 64, 8
STAGE_CYCLES, TEST_CYCLES, PAIR_BOUNCE_CYCLES = 15 * 4.1 + 2 * 8.3, 2 * 4.1, 1250.0


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "pair_skip_counts.json"))
    ap.add_argument("--general", action="store_true")
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    sph = torch.from_numpy(gen_data.gen_spheres()).cuda()
    if args.general:
        perm = sph.clone().view(-1)[:80].view(10, 8).clone()
        perm[:, [0, 6]] = perm[:, [6, 0]]
        sph[:80] = perm.reshape(-1)
    buf = torch.zeros(128, dtype=torch.int64, device="cuda")
    _lib.lib().apt_set_trace_counter(ctypes.c_void_p(buf.data_ptr()))
    render.render_frame(apt.make_params(W, H, S, depth=DEPTH), sph)
    torch.cuda.synchronize()
    _lib.lib().apt_set_trace_counter(None)
    c = buf.cpu().tolist()
    waves = c[68]
    assert waves > 0, "the library in APT_LIB_PATH is not the counting build"
    table = {}
    for pair in range(4):
        per = {h: [c[4 + (h * 8 + b) * 4 + pair] / waves for b in range(DEPTH)] for h in (0, 1)}
        p_bounce = [round((per[0][b] + per[1][b]) / 2, 4) for b in range(DEPTH)]
        p = sum(p_bounce) / DEPTH
        table[f"pair_{2 * pair}_{2 * pair + 1}"] = {
            "P_per_bounce": p_bounce, "P_path_A_per_bounce": [round(x, 4) for x in per[0]], "P_path_B_per_bounce": [round(x, 4) for x in per[1]],
            "P_mean": round(p, 4),
            # both paths of a pair-bounce: 2 * (P * stage - test) cycles of 1250
            "predicted_net_gain_of_a_pair_bounce": round(2 * (p * STAGE_CYCLES - TEST_CYCLES) / PAIR_BOUNCE_CYCLES, 5),
            "predicted_valu_per_segment": round(p * 15 - 2, 3)}
    out = {"what": "share P of the (wave, path half, bounce) triples of one C2 frame in which no lane can hit either sphere of the pair "
                   "(predicate (a): both discriminants negative or NaN in all 64 lanes)",
           "launch": "render_frame_kernel<0, 0, 8, false, true>", "frame": f"{W}x{H}, S={S}, depth {DEPTH}", "scene": "general (spheres 0 and 6 exchanged)" if args.general else "gen_spheres()",
           "device": torch.cuda.get_device_name(0), "wave_pair_traces": waves, "segments_traced": c[0], "exact_reruns": c[3], "pairs": table}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
