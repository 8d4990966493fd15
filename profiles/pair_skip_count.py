#!/usr/bin/env python3
"""How often a whole wave of the headline launch cannot hit either sphere of a pair.  Needs an MI355X and the counting build:

    bash profiles/build_variant.sh pair_count -DAPT_COUNT_PAIR_SKIP
    APT_LIB_PATH=profiles/microbench/lib_pair_count.so python profiles/pair_skip_count.py [--out profiles/pair_skip_counts.json]

One C2 frame (bench.py's headline launch, render_frame_kernel<0, 0, 8, false, true>) with a 128-entry statistics block: the counting
build (pt_trace2.h, APT_COUNT_PAIR_SKIP) adds one to entry [4 + (half * 8 + bounce) * 4 + pair] for every wave in which
pair_misses_wave() holds -- both discriminants of the pair negative or NaN in all 64 lanes -- and one to entry [68] per wave and path pair it traces (the denominator).
`--general`: the bench's general scene (spheres 0 and 6 exchanged), the non-shared-planes arm.
`--split-out FILE` (profiles/pair67_split_counts.json): pair (6,7) per sphere and with the ray's direction, from the same frame -- the
counting build adds one to entry [72 + (half * 8 + bounce) * 4 + j] per wave in which no lane can hit sphere 6 (j = 0), sphere 7 (1) or
either (2) by pt_trace.h's sphere_reachable_mask(), and (3) either by the unguarded statement "disc < 0 or NaN, or b < 0 and c > 0" --
and the price of every order of tests under the same model (ONE_STAGE_CYCLES: the root stage of one sphere, 11 VALU instructions, one of them v_rsq_f32).
The price model of the table: a pair's root stage is 15 VALU + 2 v_rsq_f32 = 78 cycles, the test 2 VALU = 8 cycles, a pair-bounce 1250
cycles, so a pair pays for itself from P = 0.10 on.
`--ab-out FILE` (profiles/ab_stage_counts.json): every sphere over the lane's TWO paths together, from the same frame -- the counting build
adds one to entry [136 + bounce * 8 + k] per wave in which no lane can hit sphere k in path A or in path B (sphere_reachable_mask()'s
statement), to [200 + ...] the same with the relaxed guard c >= 0, to [264 + ...] / [328 + ...] the two forms that read no discriminant
(b < -2^-60 and c > 2^-60, or c >= 0), and to [392 + bounce * 4 + j] per wave whose 128 paths have all just left one wall (j = 0), where that
wall passes the strict (1) or the relaxed (2) statement, and where the wall opposite passes the strict one (3) -- and the price of a root
stage packed over (A, B) per sphere with a joint test of 3 VALU (walls) or 4 VALU (ball and light, which need the discriminant)."""
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
ONE_STAGE_CYCLES = 11 * 4.1 + 1 * 8.3   # as compiled: the full stage's half for one sphere is 10 instructions, and one v_mov


def split_table(c, waves):
    """Shares and prices of the per-sphere tests of pair (6,7), per path half and bounce.  Cycles per path-bounce of
      now        the pair test, then the full stage                                  T + (1 - Pa) F
      both       test 6, test 7: skip / sphere 7 only / sphere 6 only / full         2T + (P6 - P67) O + (P7 - P67) O + (1 - P6 - P7 + P67) F
      six_first  test 6; if no lane can hit it test 7: skip / sphere 7 only; else full   T + P6 T + (P6 - P67) O + (1 - P6) F
    with T = 2 VALU, F the full stage, O the one-sphere stage."""
    T, F, O = TEST_CYCLES, STAGE_CYCLES, ONE_STAGE_CYCLES
    sites = []
    for h in (0, 1):
        for b in range(DEPTH):
            base = 72 + (h * 8 + b) * 4
            p6, p7, p67, plain = (c[base + j] / waves for j in range(4))
            pa = c[4 + (h * 8 + b) * 4 + 3] / waves
            cost = {"now": T + (1 - pa) * F,
                    "both": 2 * T + (p6 - p67) * O + (p7 - p67) * O + (1 - p6 - p7 + p67) * F,
                    "six_first": T + p6 * T + (p6 - p67) * O + (1 - p6) * F}
            best = min(cost, key=cost.get)
            # what was built from these counts (intersect_ns8_v2's SKIP forms, per path): "now" at the first bounce, "both" from the second on, nothing on path B's last bounce
            last_b = h == 1 and b == DEPTH - 1
            valu_now = 15.0 if last_b else 2 + (1 - pa) * 15
            valu_built = valu_now if (b == 0 or last_b) else 4 + (p6 + p7 - 2 * p67) * 11 + (1 - p6 - p7 + p67) * 15
            cycles_now = F if last_b else cost["now"]
            cycles_built = cycles_now if (b == 0 or last_b) else cost["both"]
            sites.append({"path": "AB"[h], "bounce": b + 1, "U6": round(p6, 4), "U7": round(p7, 4), "U6_and_U7": round(p67, 4),
                          "U6_not_U7": round(p6 - p67, 4), "U7_not_U6": round(p7 - p67, 4), "U6_and_U7_unguarded": round(plain, 4),
                          "present_predicate": round(pa, 4), "cycles": {k: round(v, 2) for k, v in cost.items()}, "cheapest": best,
                          "saving_cycles": round(cost["now"] - cost[best], 2),
                          "built": "unchanged" if (b == 0 or last_b) else "both", "built_saving_cycles": round(cycles_now - cycles_built, 2),
                          "built_valu_instructions_saved": round(valu_now - valu_built, 3)})
    return sites


AB_TEST_WALL, AB_TEST_DISC, AB_DISC_PAIR = 3 * 4.1, 4 * 4.1, 2 * 4.1   # joint tests; the sphere's packed b*b and - c, skipped with the stage
AB_FEWER_PACKED = 3 * 4.1          # 95 instead of 98 packed instructions for the discriminants of both paths
BOUNCE_SHARE_OF_FRAME = 0.86       # (283 + 6 * 286 + 233) / 16 - 4.77 - 1.93 = 132.8 of the 154.33 VALU instructions per segment
AB_GATE = 0.02


def ab_table(c, waves):
    """Per bounce site of a pair-bounce (both paths), in cycles: what a root stage packed over (A, B) per sphere saves against today's
    layout.  An unskipped stage costs what it costs today (six wall stages either way), so a wall k gains P (F + 2 packed) - test where
    its test is on, and nothing where it is off; pair (6,7) is priced against today's pair / per-sphere tests from the same frame."""
    F, O, T2 = STAGE_CYCLES, ONE_STAGE_CYCLES, TEST_CYCLES
    sites = []
    for b in range(DEPTH):
        blk = lambda base: [c[base + b * 8 + k] / waves for k in range(8)]
        strict, relaxed, nodisc, nodisc_relaxed = blk(136), blk(200), blk(264), blk(328)
        walls, wall_gain, wall_gain_relaxed = [], 0.0, 0.0
        for k in range(6):
            g = nodisc[k] * (F + AB_DISC_PAIR) - AB_TEST_WALL
            gr = nodisc_relaxed[k] * (F + AB_DISC_PAIR) - AB_TEST_WALL
            wall_gain += max(g, 0.0)
            wall_gain_relaxed += max(gr, 0.0)
            walls.append({"sphere": k, "P": round(strict[k], 4), "P_relaxed": round(relaxed[k], 4), "P_no_disc": round(nodisc[k], 4),
                          "P_no_disc_relaxed": round(nodisc_relaxed[k], 4), "gain_cycles": round(g, 2), "gain_cycles_relaxed": round(gr, 2),
                          "test": "on" if g > 0 else "off"})
        today67 = 0.0
        for h in (0, 1):   # today's pair (6,7), as built (split_table): pair test at the first bounce, per-sphere from the second, none on B's last
            pa = c[4 + (h * 8 + b) * 4 + 3] / waves
            p6, p7, p67 = (c[72 + (h * 8 + b) * 4 + j] / waves for j in range(3))
            if h == 1 and b == DEPTH - 1:
                today67 += F
            elif b == 0:
                today67 += T2 + (1 - pa) * F
            else:
                today67 += 2 * T2 + (p6 - p67) * O + (p7 - p67) * O + (1 - p6 - p7 + p67) * F
        new67, tests67 = 0.0, []
        for k in (6, 7):
            with_test = AB_TEST_DISC + (1 - strict[k]) * F - strict[k] * AB_DISC_PAIR
            new67 += min(with_test, F)
            tests67.append("on" if with_test < F else "off")
        j = 392 + b * 4
        left = {"waves_share": round(c[j] / waves, 4), "passes_strict": round(c[j + 1] / c[j], 4) if c[j] else None,
                "passes_relaxed": round(c[j + 2] / c[j], 4) if c[j] else None, "opposite_passes_strict": round(c[j + 3] / c[j], 4) if c[j] else None}
        total = wall_gain + (today67 - new67) + AB_FEWER_PACKED
        sites.append({"bounce": b + 1, "walls": walls, "P_sphere_6": round(strict[6], 4), "P_sphere_7": round(strict[7], 4),
                      "P_sphere_6_relaxed": round(relaxed[6], 4), "P_sphere_7_relaxed": round(relaxed[7], 4),
                      "pair67_today_cycles": round(today67, 2), "pair67_new_cycles": round(new67, 2), "pair67_tests": tests67,
                      "just_left_wall": left, "wall_gain_cycles": round(wall_gain, 2), "wall_gain_cycles_relaxed": round(wall_gain_relaxed, 2),
                      "pair67_gain_cycles": round(today67 - new67, 2), "gain_cycles": round(total, 2),
                      "gain_cycles_relaxed": round(total - wall_gain + wall_gain_relaxed, 2)})
    return sites


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "pair_skip_counts.json"))
    ap.add_argument("--general", action="store_true")
    ap.add_argument("--split-out", default=None)
    ap.add_argument("--ab-out", default=None)
    args = ap.parse_args()
    apt = __graft_entry__.build()
    from ascendpathtracing_amd import _lib, gen_data, render
    _lib.require_gpu()
    sph = torch.from_numpy(gen_data.gen_spheres()).cuda()
    if args.general:
        perm = sph.clone().view(-1)[:80].view(10, 8).clone()
        perm[:, [0, 6]] = perm[:, [6, 0]]
        sph[:80] = perm.reshape(-1)
    buf = torch.zeros(512, dtype=torch.int64, device="cuda")
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
    if args.split_out:
        sites = split_table(c, waves)
        per_form = {k: round(sum(s["cycles"]["now"] - s["cycles"][k] for s in sites) / DEPTH, 2) for k in ("both", "six_first")}
        split = {"what": "pair (6,7) of one C2 frame: share of the waves in which every lane satisfies U6 / U7 (the sphere cannot be hit: "
                         "sphere_reachable_mask() is 0), per path half and bounce, and the cycles per path-bounce of each order of tests",
                 "launch": out["launch"], "frame": out["frame"], "scene": out["scene"], "device": out["device"], "wave_pair_traces": waves,
                 "price_model": f"VALU 4.1, transcendental 8.3 cycles: test {TEST_CYCLES:.1f}, full stage {STAGE_CYCLES:.1f}, "
                                f"one-sphere stage {ONE_STAGE_CYCLES:.1f}, pair-bounce {PAIR_BOUNCE_CYCLES:.0f}",
                 "sites": sites,
                 "saving_cycles_per_pair_bounce_one_form_everywhere": per_form,
                 "saving_cycles_per_pair_bounce_cheapest_per_site": round(sum(s["saving_cycles"] for s in sites) / DEPTH, 2),
                 "go_threshold_cycles": round(0.015 * PAIR_BOUNCE_CYCLES, 2),
                 "built_saving_cycles_per_pair_bounce": round(sum(s["built_saving_cycles"] for s in sites) / DEPTH, 2),
                 "built_predicted_valu_instructions_per_segment_saved": round(sum(s["built_valu_instructions_saved"] for s in sites) / (2 * DEPTH), 3)}
        with open(args.split_out, "w") as f:
            json.dump(split, f, indent=1)
            f.write("\n")
        print(json.dumps(split))
    if args.ab_out:
        assert not args.general, "the (A, B) counts are of the shared-planes form"
        sites = ab_table(c, waves)
        mean = sum(s["gain_cycles"] for s in sites) / DEPTH
        mean_relaxed = sum(s["gain_cycles_relaxed"] for s in sites) / DEPTH
        frame = mean / PAIR_BOUNCE_CYCLES * BOUNCE_SHARE_OF_FRAME
        ab = {"what": "one C2 frame: per bounce and sphere, the share P of the waves in which no lane can hit the sphere in path A or in path B "
                      "(disc < 0 or NaN, or b < -2^-60 and c > 2^-60; P_relaxed: c >= 0; P_no_disc: the second clause alone), the wall a whole wave "
                      "has just left, and the price of a root stage packed over (A, B) per sphere with a joint test in front of it",
              "launch": out["launch"], "frame": out["frame"], "scene": out["scene"], "device": out["device"], "wave_pair_traces": waves,
              "price_model": f"VALU 4.1, transcendental 8.3 cycles: stage {STAGE_CYCLES:.1f}, wall test {AB_TEST_WALL:.1f}, test with discriminant "
                             f"{AB_TEST_DISC:.1f}, the skipped sphere's two packed discriminant instructions {AB_DISC_PAIR:.1f}, three packed "
                             f"instructions fewer per pair-bounce {AB_FEWER_PACKED:.1f}, pair-bounce {PAIR_BOUNCE_CYCLES:.0f}; the bounce blocks are "
                             f"{BOUNCE_SHARE_OF_FRAME} of the frame's VALU instructions",
              "sites": sites,
              "gain_cycles_per_pair_bounce": round(mean, 2), "gain_cycles_per_pair_bounce_relaxed_guard": round(mean_relaxed, 2),
              "gain_share_of_pair_bounce": round(mean / PAIR_BOUNCE_CYCLES, 4),
              "priced_share_of_frame": round(frame, 4), "priced_share_of_frame_relaxed_guard": round(mean_relaxed / PAIR_BOUNCE_CYCLES * BOUNCE_SHARE_OF_FRAME, 4),
              "gate_share_of_frame": AB_GATE, "gate": "passed" if frame >= AB_GATE else "not passed"}
        with open(args.ab_out, "w") as f:
            json.dump(ab, f, indent=1)
            f.write("\n")
        print(json.dumps(ab))


if __name__ == "__main__":
    main()
