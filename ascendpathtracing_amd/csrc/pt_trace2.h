// pt_trace2.h -- TWO paths per lane for the full-trace 8-sphere frame kernel (included by pt_kernels.h).
//
// In this kernel a VALU instruction costs one ~4-cycle issue slot whatever it does (profiles/microbench/
// issue_model_mi355x.txt), so the bounce costs its instruction COUNT and a packed
// v_pk_*_f32 is two operations for one slot.  The intersections are already packed (two spheres per
// instruction); the shading step of ONE path only fills the second half for the x/y components.  With two
// paths A and B in a lane, every register pair holds (A, B) of one quantity and the whole shading step runs
// packed: 36 instead of 48 instructions per path and bounce.  The intersections of the general form stay as they are -- eight
// spheres in four packed pairs per path, reading ray component A or B out of its pair through op_sel (free) -- and run for A, then
// for B, so the scalar arg-min masks of A are consumed before B needs the registers.  A table that shares planes is intersected for
// both paths at once, one sphere per instruction (intersect2_ns8_planes below).
//
// Same arithmetic as bounce_ns8_v2 (pt_trace.h), operation for operation: v_pk_{add,mul,fma}_f32 round each half
// like the scalar instruction.  Used for the frame kernel without APT_FLAG_RETIRE and APT_FLAG_RR only.
#pragma once
#include <type_traits>

#include "pt_trace.h"

namespace {

struct PathPair { // .x = path A, .y = path B
    f2 ox, oy, oz, dx, dy, dz; // rays
    f2 rx, ry, rz;             // throughputs
#ifdef APT_COUNT_PAIR_SKIP
    uint32_t hitA, hitB;       // measurement build only: table offset (index * 16) of the sphere each path has just left, ~0u when unknown
#endif
};

// first: the pair has no throughputs yet -- path_init's (1, 1, 1) and alive = 1 stand
__device__ __forceinline__ PathState unpack_path(const PathPair &p, int which, uint64_t alive, bool first) {
    PathState s;
    if (which == 0) path_init(s, p.ox.x, p.oy.x, p.oz.x, p.dx.x, p.dy.x, p.dz.x);
    else path_init(s, p.ox.y, p.oy.y, p.oz.y, p.dx.y, p.dy.y, p.dz.y);
    if (first) return s;
    s.rxy = which == 0 ? f2{p.rx.x, p.ry.x} : f2{p.rx.y, p.ry.y};
    s.rz = which == 0 ? p.rz.x : p.rz.y;
    s.alive = select_const(alive, 1);
    return s;
}

// One path's arg-min state of the (A, B)-packed intersection below: intersect_ns8_v2's best / b0 / b1 / b2 / any, its key update and
// its tail, statement for statement.
template <int MODE>
struct ArgMin8 {
    uint32_t best;
    uint64_t b0 = 0, b1 = 0, b2 = 0, any = 0;
    __device__ __forceinline__ void update64(uint64_t keys, int k) {
        const uint32_t nb = min3_u32(best, (uint32_t)keys, (uint32_t)(keys >> 32));
        const uint64_t better = __builtin_amdgcn_ballot_w64(nb != best); // strict '<': lowest index wins ties
        best = nb;
        b0 = (k & 1) ? (b0 | better) : (b0 & ~better);
        b1 = (k & 2) ? (b1 | better) : (b1 & ~better);
        b2 = (k & 4) ? (b2 | better) : (b2 & ~better);
        if (MODE == kModeOracle) any |= better;
    }
    __device__ __forceinline__ Hit8 finish(const TraceArgs &ta, const KeyConsts &kc) {
        const float tmin = bits_f32(best + kc.bias);
        if (MODE == kModeOracle) { b0 |= ~any; b1 |= ~any; b2 |= ~any; }
        uint32_t addr;
        {
            const uint32_t a0 = select_const(b0, 16), a1 = select_const(b1, 32), a2 = select_const(b2, 64);
            asm("v_or3_b32 %0, %1, %2, %3" : "=v"(addr) : "v"(a0), "v"(a1), "v"(a2));
        }
        uint64_t light_mask = __builtin_amdgcn_ballot_w64(addr == (uint32_t)ta.light * 16u);
        if (MODE == kModeOracle) light_mask &= any;
        return Hit8{tmin, addr, light_mask};
    }
};

// (c, c) - v and v - (c, c), c = half HALF of a scalar register pair: v_pk_add_f32 with the constant broadcast by op_sel.  Left to the
// compiler a broadcast scalar becomes an SGPR pair (c, c) of its own -- two registers per constant, twice what the kernel has.
template <int HALF>
__device__ __forceinline__ f2 pair_half_minus(f2 cpair, f2 v) {
    f2 r;
    if (HALF == 0) asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "s"(cpair), "v"(v));
    else asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "s"(cpair), "v"(v));
    return r;
}
template <int HALF>
__device__ __forceinline__ f2 minus_pair_half(f2 v, f2 cpair) {
    f2 r;
    if (HALF == 0) asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(v), "s"(cpair));
    else asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(r) : "v"(v), "s"(cpair));
    return r;
}

// The spheres whose root stage the (A, B)-packed intersection puts behind the joint test (bit k = sphere k).  Decided by counting
// (profiles/ab_stage_counts.json; one C2 frame, per bounce the share of the waves in which no lane can reach
// the sphere in either path): the ball 0.970 .. 0.795 and the light 0.844 .. 0.539 over eight bounces, at every bounce site, path B
// of the last bounce included (this form compiles without scratch there); no wall -- the room lies INSIDE every wall's sphere
// (c < 0), so a wall is never behind a ray that is in the room: 0 of 4.1 million waves for spheres 2 .. 5, and 0.117 for the side
// walls (waves whose paths have all left the room), below the break-even of 0.14.  The general form has no test: the one-path
// intersection's SKIP forms (pt_trace.h), which the two-path bounce used for pair (6,7) before, are off for every caller now.
constexpr int kAbSkip = 0xC0;

// The intersection half of a bounce for BOTH paths of a lane, shared-planes form: every packed instruction works on the (A, B) pair
// of one quantity of ONE sphere, the sphere's constant broadcast from its SGPR.  Per path and sphere the operations are
// intersect_pre_planes_pairs' and intersect_ns8_v2's full stage, in the same order -- cx - o, its product with d and its square
// once per DISTINCT coordinate (13 of them: 39 packed instructions for both paths), b = (px + py) + pz, c = ((qx + qy) + qz) - r2,
// disc = b*b - c (7 per sphere), then v_rsq_f32 per path, sqrt_rsq_step on the pair, root_pair<0> / <1> = path A's / path B's
// (-t0, t1), one 64-bit add, v_min3_u32 and a compare each -- and the spheres are taken in ascending index, so each path's key
// updates happen in intersect_ns8_v2's order and the strict-'<', lowest-index-wins rule holds as there.  What changes is which
// operations share an instruction, and a packed operation rounds each half like the scalar one.
// SKIP, bit k: sphere k's root stage is branched round (a scalar branch on an opaque flag) when, in every lane and for path A and
// path B, sphere_reachable_mask()'s statement holds: disc < 0 or NaN, or b < -2^-60 and c > 2^-60.  Its exactness argument (above
// intersect_ns8_v2's SKIP) is per path and per sphere and carries over unchanged: such a sphere's keys are >= key(kMissT) in both
// paths, its v_min3_u32 would not have changed either `best`, and its compares would have set no bit.  Two v_med3_f32, one
// v_max_f32 (a NaN drops out: a path whose med3 is NaN is outside the mask, as it is in the one-path form) and one compare.
// amin: per path, |disc| of the walls two spheres per instruction as before; a skipped sphere's share is left out (it could only
// have asked for the exact re-run, which finds the same miss).
// PLAN (the pair's first bounce in the frame kernel): `plan`, bit k, wave-uniform -- sphere k cannot be the first hit of any camera ray
// of the wave's pixels (pt_first_plan.h: the wall, ball and light rules with their proofs; every key of such a sphere is above the
// winner's or >= key(kMissT)).  Sphere k's own-coordinate terms, b, c, disc, joint test and stage then sit behind ONE scalar branch on
// an opaque flag and cost no vector instruction; a wall whose partner is skipped takes its |disc| into `amin` alone, as a tested
// sphere does (the minimum of the same set).  The shared terms x2, y0, z0 stay unconditional, the order stays ascending.
template <int MODE, int SKIP, bool PLAN = false>
__device__ __forceinline__ void intersect2_ns8_planes(const Scene8 &sc, const PathPair &s, const TraceArgs &ta, const KeyConsts &kc,
                                                      float &aminA, float &aminB, Hit8 &hA, Hit8 &hB, uint32_t plan = 0) {
    struct Term { f2 p, q; };   // (c - o) * d and (c - o)^2 of one centre coordinate, both paths
    auto term = [](auto half, f2 cpair, f2 o, f2 d) __attribute__((always_inline)) {
        const f2 t = pair_half_minus<decltype(half)::value>(cpair, o);
        return Term{t * d, t * t};
    };
    struct Pre { f2 b, c, disc; };
    auto pre = [](const Term &x, const Term &y, const Term &z, auto half, f2 r2pair) __attribute__((always_inline)) {
        Pre h;
        h.b = (x.p + y.p) + z.p;
        h.c = minus_pair_half<decltype(half)::value>((x.q + y.q) + z.q, r2pair);
        h.disc = h.b * h.b - h.c;
        return h;
    };
    ArgMin8<MODE> A, B;
    A.best = kc.init; B.best = kc.init;
    auto stage = [&](const Pre &h, int k) __attribute__((always_inline)) {
        const f2 q = sqrt_rn_rsq1_pair(h.disc);
        A.update64(root_pair<0>(h.b, q) + kc.nbias2, k);
        B.update64(root_pair<1>(h.b, q) + kc.nbias2, k);
    };
    auto walls = [&](const Pre &h0, const Pre &h1, int k) __attribute__((always_inline)) {
        aminA = minimum3_abs(aminA, h0.disc.x, h1.disc.x);
        aminB = minimum3_abs(aminB, h0.disc.y, h1.disc.y);
        stage(h0, k);
        stage(h1, k + 1);
    };
    auto tested = [&](const Pre &h, int k) __attribute__((always_inline)) {
        if ((SKIP >> k) & 1) {
            const float mA = __builtin_amdgcn_fmed3f(h.disc.x, h.b.x, -h.c.x), mB = __builtin_amdgcn_fmed3f(h.disc.y, h.b.y, -h.c.y);
            uint32_t run = any_lane(__builtin_amdgcn_ballot_w64(__builtin_fmaxf(mA, mB) >= -kBehindGuard));
            asm("" : "+s"(run));
            if (run == 0u) return;
        }
        aminA = minimum3_abs(aminA, h.disc.x, h.disc.x);
        aminB = minimum3_abs(aminB, h.disc.y, h.disc.y);
        stage(h, k);
    };
    auto wall = [&](const Pre &h, int k) __attribute__((always_inline)) {   // one wall of a pair whose spheres the plan decides one by one
        aminA = minimum3_abs(aminA, h.disc.x, h.disc.x);
        aminB = minimum3_abs(aminB, h.disc.y, h.disc.y);
        stage(h, k);
    };
    // (a copy made HERE, for this intersection alone: the kernel's mask lives across the whole sample loop, is spilled, and read in place
    // it comes back through a v_readlane_b32 in front of every branch; the copy is short-lived and stays in its scalar register)
    uint32_t here = 0;
    if (PLAN) asm volatile("s_mov_b32 %0, %1" : "=s"(here) : "s"(plan));
    auto planned = [&](auto bit) __attribute__((always_inline)) {   // -> 0: the plan leaves sphere decltype(bit)::value out
        // (volatile: made where it is read.  Left to the compiler the seven flags are made once per wave, live in seven spilled
        // scalars, and each first bounce pays a v_readlane_b32 per flag to get them back)
        uint32_t run;
        asm volatile("s_bitcmp0_b32 %1, %2\n\ts_cselect_b32 %0, 1, 0" : "=s"(run) : "s"(here), "n"(decltype(bit)::value) : "scc");
        return run;
    };
    static_assert((SKIP & 0x3F) == 0, "the walls have no test: the room lies inside their spheres");
    using B0 = std::integral_constant<int, 0>; using B1 = std::integral_constant<int, 1>; using B3 = std::integral_constant<int, 3>;
    using B4 = std::integral_constant<int, 4>; using B5 = std::integral_constant<int, 5>; using B6 = std::integral_constant<int, 6>;
    using B7 = std::integral_constant<int, 7>;   // (the bit index is an immediate of the asm statement: a type, not a value the optimiser has to fold)
    // the scalar pairs of intersect_pre_planes(): every constant is one half of an aligned SGPR pair
    const f2 X1 = {sc.cx[0], sc.cx[1]}, X2 = {sc.cx[2], sc.cx[6]}, Y1 = {sc.cy[4], sc.cy[5]}, Y2 = {sc.cy[6], sc.cy[7]}, Y3 = {sc.cy[0], sc.cy[0]};
    const f2 Z1 = {sc.cz[2], sc.cz[3]}, Z2 = {sc.cz[0], sc.cz[6]};
    const f2 R0 = {sc.r2[0], sc.r2[1]}, R1 = {sc.r2[2], sc.r2[3]}, R2 = {sc.r2[4], sc.r2[5]}, R3 = {sc.r2[6], sc.r2[7]};
    using Lo = std::integral_constant<int, 0>;
    using Hi = std::integral_constant<int, 1>;
    const Term x2 = term(Lo{}, X2, s.ox, s.dx), y0 = term(Lo{}, Y3, s.oy, s.dy), z0 = term(Lo{}, Z2, s.oz, s.dz);   // the shared planes
    if (PLAN) {
        if (planned(B0{}) != 0u) wall(pre(term(Lo{}, X1, s.ox, s.dx), y0, z0, Lo{}, R0), 0);
        if (planned(B1{}) != 0u) wall(pre(term(Hi{}, X1, s.ox, s.dx), y0, z0, Hi{}, R0), 1);
        wall(pre(x2, y0, term(Lo{}, Z1, s.oz, s.dz), Lo{}, R1), 2);   // (the wall the camera looks at: no rule)
        if (planned(B3{}) != 0u) wall(pre(x2, y0, term(Hi{}, Z1, s.oz, s.dz), Hi{}, R1), 3);
        if (planned(B4{}) != 0u) wall(pre(x2, term(Lo{}, Y1, s.oy, s.dy), z0, Lo{}, R2), 4);
        if (planned(B5{}) != 0u) wall(pre(x2, term(Hi{}, Y1, s.oy, s.dy), z0, Hi{}, R2), 5);
        if (planned(B6{}) != 0u) tested(pre(term(Hi{}, X2, s.ox, s.dx), term(Lo{}, Y2, s.oy, s.dy), term(Hi{}, Z2, s.oz, s.dz), Lo{}, R3), 6);
        if (planned(B7{}) != 0u) tested(pre(x2, term(Hi{}, Y2, s.oy, s.dy), z0, Hi{}, R3), 7);
    } else {
        walls(pre(term(Lo{}, X1, s.ox, s.dx), y0, z0, Lo{}, R0), pre(term(Hi{}, X1, s.ox, s.dx), y0, z0, Hi{}, R0), 0);
        walls(pre(x2, y0, term(Lo{}, Z1, s.oz, s.dz), Lo{}, R1), pre(x2, y0, term(Hi{}, Z1, s.oz, s.dz), Hi{}, R1), 2);
        walls(pre(x2, term(Lo{}, Y1, s.oy, s.dy), z0, Lo{}, R2), pre(x2, term(Hi{}, Y1, s.oy, s.dy), z0, Hi{}, R2), 4);
        tested(pre(term(Hi{}, X2, s.ox, s.dx), term(Lo{}, Y2, s.oy, s.dy), term(Hi{}, Z2, s.oz, s.dz), Lo{}, R3), 6);
        tested(pre(x2, term(Hi{}, Y2, s.oy, s.dy), z0, Hi{}, R3), 7);
    }
    hA = A.finish(ta, kc);
    hB = B.finish(ta, kc);
}

// One bounce of both paths.  aliveA / aliveB: wave masks (in: before, out: after).  redoA / redoB: wave masks of
// the lanes whose path A / B left the validity range of the fast sequences.  `ones_off`: byte offset, relative to the albedo
// table, of an entry (1, 1, 1) -- a path that is no longer alive multiplies its throughput by it (x1 is exact).
// FIRST: the first bounce of a pair.  Both paths are alive and their throughput is (1, 1, 1) by definition: s.rx / ry / rz and
// the incoming masks are not read, the new masks are ~light, and the new throughput IS the albedo entry (or the (1, 1, 1) entry
// for a path that hit the light) -- no products.
// PLAN (with FIRST and PLANES only): `plan` is the wave's first-bounce plan, see intersect2_ns8_planes.
template <int MODE, bool PLANES, bool FIRST, bool PLAN = false>
__device__ __forceinline__ void bounce2_ns8_t(const Scene8 &sc, const Tab8 tab, const PathPair &s, PathPair &n,
                                              const TraceArgs &ta, const KeyConsts &kc, uint32_t ones_off,
                                              uint64_t &aliveA, uint64_t &aliveB, uint64_t &redoA, uint64_t &redoB, uint32_t plan = 0) {
    float aminA = 1.0f, aminB = 1.0f; // per path: a finished path's request for the exact form can be ignored (trace2_ns8)
    Hit8 hA, hB;
    if (PLANES) {
        intersect2_ns8_planes<MODE, kAbSkip, PLAN && FIRST>(sc, s, ta, kc, aminA, aminB, hA, hB, plan);
    } else {
        hA = intersect_ns8_v2<MODE>(sc, s.ox.x, s.oy.x, s.oz.x, s.dx.x, s.dy.x, s.dz.x, ta, kc, aminA);
        hB = intersect_ns8_v2<MODE>(sc, s.ox.y, s.oy.y, s.oz.y, s.dx.y, s.dy.y, s.dz.y, ta, kc, aminB);
    }
    if (FIRST) {
        aliveA = ~hA.light;
        aliveB = ~hB.light;
    } else {
        aliveA &= ~hA.light;                // rt_helper.h:773-787  alive &= idx != light
        aliveB &= ~hB.light;
    }
    // centre and albedo of the two hit spheres: dword reads from the LDS table straight into (A, B) pairs
    const char *geo = reinterpret_cast<const char *>(tab.geo);
    uint32_t cA, cB; // albedo entry, or the (1,1,1) entry once the path is not alive (rt_helper.h:799-810: ret *= alive ? albedo : 1)
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(cA) : "v"(ones_off), "v"(hA.addr), "s"(aliveA));
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(cB) : "v"(ones_off), "v"(hB.addr), "s"(aliveB));
    // Twelve ds_read_b32 in one asm block, each landing in its half of an (A, B) pair.  Left to the compiler the reads of one
    // path are merged into ds_read2_b32 -- an (x, y) pair of ONE path, which then costs six v_mov per pair-bounce (VALU slots) to
    // shuffle into the (A, B) layout; LDS issue is not what binds this kernel.  The block waits for its own reads (the
    // compiler's s_waitcnt insertion does not see them); the other waves of the SIMD cover the latency.
    const uint32_t gA = (uint32_t)(uintptr_t)geo + hA.addr, gB = (uint32_t)(uintptr_t)geo + hB.addr;
    const uint32_t aA = (uint32_t)(uintptr_t)geo + cA, aB = (uint32_t)(uintptr_t)geo + cB; // + 128 below: alb = geo + 8 entries (load_scene8)
    float cxA, cyA, czA, cxB, cyB, czB, axA, ayA, azA, axB, ayB, azB;
    asm volatile("ds_read_b32 %0, %12\n ds_read_b32 %1, %12 offset:4\n ds_read_b32 %2, %12 offset:8\n"
                 "ds_read_b32 %3, %13\n ds_read_b32 %4, %13 offset:4\n ds_read_b32 %5, %13 offset:8\n"
                 "ds_read_b32 %6, %14 offset:128\n ds_read_b32 %7, %14 offset:132\n ds_read_b32 %8, %14 offset:136\n"
                 "ds_read_b32 %9, %15 offset:128\n ds_read_b32 %10, %15 offset:132\n ds_read_b32 %11, %15 offset:136\n"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(cxA), "=&v"(cyA), "=&v"(czA), "=&v"(cxB), "=&v"(cyB), "=&v"(czB), "=&v"(axA), "=&v"(ayA), "=&v"(azA),
                   "=&v"(axB), "=&v"(ayB), "=&v"(azB)
                 : "v"(gA), "v"(gB), "v"(aA), "v"(aB)
                 : "memory");
    const f2 cx = {cxA, cxB}, cy = {cyA, cyB}, cz = {czA, czB};
    const f2 ax = {axA, axB}, ay = {ayA, ayB}, az = {azA, azB};
    // GenerateNewRays, rt_helper.h:504-709 (see bounce_ns8_v2 for the single-path form)
    const f2 t = {hA.tmin, hB.tmin};
    const f2 hx = s.ox + s.dx * t, hy = s.oy + s.dy * t, hz = s.oz + s.dz * t;   // :513-518
    const f2 nx = hx - cx, ny = hy - cy, nz = hz - cz;                            // :635-637
    f2 len2;
    if (MODE == kModeOracle) {
        const f2 p0 = nx * nx, p1 = ny * ny, p2 = nz * nz;
        len2 = f2{sum3_f64(p0.x, p1.x, p2.x), sum3_f64(p0.y, p1.y, p2.y)};
    } else {
        len2 = nx * nx + ny * ny;                                                  // :641-649 (0 + x^2 is x^2)
        len2 = len2 + nz * nz;
    }
    const f2 r0 = {__builtin_amdgcn_rsqf(len2.x), __builtin_amdgcn_rsqf(len2.y)};
    aminA = minimum3_abs_after_trans(aminA, r0.x, nx.x);        // validity of the fast sqrt / divide sequences: see kFastMin (pt_trace.h)
    aminA = minimum3_abs(aminA, ny.x, nz.x);
    aminB = minimum3_abs_after_trans(aminB, r0.y, nx.y);
    aminB = minimum3_abs(aminB, ny.y, nz.y);
    const f2 L = sqrt_rsq_step(len2, r0);                       // sqrt_rn_rsq1 on both paths
    // the three quotients of both paths, the reciprocal refined from the square root's own seed (pt_core.h): no v_rcp_f32.  A lane
    // whose divisor has an all-ones mantissa can come out with e1 == 2^-24 and then joins the exact re-run below.
    f2 ux, uy, uz, e1;
    div3_seeded_packed2(nx, ny, nz, L, r0, ux, uy, uz, e1);
    f2 dot;
    if (MODE == kModeOracle) {
        const f2 p0 = s.dx * ux, p1 = s.dy * uy, p2 = s.dz * uz;
        dot = f2{sum3_f64(p0.x, p1.x, p2.x), sum3_f64(p0.y, p1.y, p2.y)};
    } else {
        dot = s.dx * ux;                                                           // :690 Duplicate(0): twice_canonical() below; :694-696
        dot = dot + s.dy * uy;
        dot = dot + s.dz * uz;
    }
    const f2 k2 = twice_canonical(dot);                                            // :697
    n.dx = s.dx - ux * k2; n.dy = s.dy - uy * k2; n.dz = s.dz - uz * k2;           // :699-704
    n.ox = hx; n.oy = hy; n.oz = hz;                                               // :706-708
    if (FIRST) { n.rx = ax; n.ry = ay; n.rz = az; }
    else { n.rx = ax * s.rx; n.ry = ay * s.ry; n.rz = az * s.rz; }                 // :804-810 (albedo or 1)
    // something too small, len2 > 2^60, or a NaN; or the reciprocal of an all-ones divisor that did not converge
    redoA = __builtin_amdgcn_ballot_w64(!(aminA >= kFastMin)) | __builtin_amdgcn_ballot_w64(e1.x == kDiv3SeededStuck);
    redoB = __builtin_amdgcn_ballot_w64(!(aminB >= kFastMin)) | __builtin_amdgcn_ballot_w64(e1.y == kDiv3SeededStuck);
#ifdef APT_COUNT_PAIR_SKIP
    n.hitA = hA.addr; n.hitB = hB.addr;
#endif
}
template <int MODE, bool PLANES>
__device__ __forceinline__ void bounce2_ns8(const Scene8 &sc, const Tab8 tab, const PathPair &s, PathPair &n,
                                            const TraceArgs &ta, const KeyConsts &kc, uint32_t ones_off,
                                            uint64_t &aliveA, uint64_t &aliveB, uint64_t &redoA, uint64_t &redoB) {
    bounce2_ns8_t<MODE, PLANES, false>(sc, tab, s, n, ta, kc, ones_off, aliveA, aliveB, redoA, redoB);
}
template <int MODE, bool PLANES>
__device__ __forceinline__ void bounce2_ns8_first(const Scene8 &sc, const Tab8 tab, const PathPair &s, PathPair &n,
                                                  const TraceArgs &ta, const KeyConsts &kc, uint32_t ones_off,
                                                  uint64_t &aliveA, uint64_t &aliveB, uint64_t &redoA, uint64_t &redoB) {
    bounce2_ns8_t<MODE, PLANES, true>(sc, tab, s, n, ta, kc, ones_off, aliveA, aliveB, redoA, redoB);
}

// The LAST bounce of both paths.  Nothing traces the ray it would produce (the callers read the throughputs only), so of a
// bounce it keeps what reaches the frame: the arg-min, alive &= idx != light, and the throughput times the hit sphere's
// albedo (or 1) -- rx / ry / rz receive those products.  No hit point, normal, square root, quotient or reflection; only the
// albedo entries are read from LDS; the validity chain ends with the discriminants (nothing else here uses a fast sequence).
// FIRST (depth 1: the last bounce is also the first): as in bounce2_ns8_t.
template <int MODE, bool PLANES, bool FIRST = false, bool PLAN = false>
__device__ __forceinline__ void bounce2_ns8_last(const Scene8 &sc, const Tab8 tab, const PathPair &s, f2 &rx, f2 &ry, f2 &rz,
                                                 const TraceArgs &ta, const KeyConsts &kc, uint32_t ones_off,
                                                 uint64_t &aliveA, uint64_t &aliveB, uint64_t &redoA, uint64_t &redoB, uint32_t plan = 0) {
    float aminA = 1.0f, aminB = 1.0f;
    Hit8 hA, hB;
    if (PLANES) {
        intersect2_ns8_planes<MODE, kAbSkip, PLAN && FIRST>(sc, s, ta, kc, aminA, aminB, hA, hB, plan);
    } else {
        hA = intersect_ns8_v2<MODE>(sc, s.ox.x, s.oy.x, s.oz.x, s.dx.x, s.dy.x, s.dz.x, ta, kc, aminA);
        hB = intersect_ns8_v2<MODE>(sc, s.ox.y, s.oy.y, s.oz.y, s.dx.y, s.dy.y, s.dz.y, ta, kc, aminB);
    }
    if (FIRST) {
        aliveA = ~hA.light;
        aliveB = ~hB.light;
    } else {
        aliveA &= ~hA.light;                // rt_helper.h:773-787  alive &= idx != light
        aliveB &= ~hB.light;
    }
    uint32_t cA, cB; // as in bounce2_ns8
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(cA) : "v"(ones_off), "v"(hA.addr), "s"(aliveA));
    asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(cB) : "v"(ones_off), "v"(hB.addr), "s"(aliveB));
    const char *geo = reinterpret_cast<const char *>(tab.geo);
    const uint32_t aA = (uint32_t)(uintptr_t)geo + cA, aB = (uint32_t)(uintptr_t)geo + cB; // + 128 below: alb = geo + 8 entries (load_scene8)
    float axA, ayA, azA, axB, ayB, azB;
    asm volatile("ds_read_b32 %0, %6 offset:128\n ds_read_b32 %1, %6 offset:132\n ds_read_b32 %2, %6 offset:136\n"
                 "ds_read_b32 %3, %7 offset:128\n ds_read_b32 %4, %7 offset:132\n ds_read_b32 %5, %7 offset:136\n"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(axA), "=&v"(ayA), "=&v"(azA), "=&v"(axB), "=&v"(ayB), "=&v"(azB)
                 : "v"(aA), "v"(aB)
                 : "memory");
    if (FIRST) { rx = f2{axA, axB}; ry = f2{ayA, ayB}; rz = f2{azA, azB}; }
    else { rx = f2{axA, axB} * s.rx; ry = f2{ayA, ayB} * s.ry; rz = f2{azA, azB} * s.rz; } // :804-810 (albedo or 1)
    redoA = __builtin_amdgcn_ballot_w64(!(aminA >= kFastMin)); // a discriminant too small, or a NaN
    redoB = __builtin_amdgcn_ballot_w64(!(aminB >= kFastMin));
}

// All bounces of both paths (full trace: no retirement, no roulette).  The hot loop has no merge with the exact
// form and no state copies (two bounces per turn, ping-pong): see trace_ns8.  On entry `s` holds the two rays; its throughputs
// are not read (a fresh path's is (1, 1, 1), and the first bounce is a form of its own that knows it).  On return only the
// throughputs of `s` are meaningful: depth - 1 bounces produce a ray, the last one (bounce2_ns8_last) does not.
//   depth 0: throughput 1.   depth 1: last<first>(s).   depth >= 2: first(s -> n), ping-pong steps from n, last from whichever
//   half holds the state.
template <int MODE, bool PLANES, bool PLAN = false>
__device__ __forceinline__ void trace2_ns8_t(const Scene8 &sc, const Tab8 tab, PathPair &s, const TraceArgs &ta, uint32_t plan = 0) {
    const KeyConsts kc = make_key_consts(ta.eps);
    uint32_t ones_off = 8 * 16; // the entry after the 8 albedos (load_scene8 writes it)
    asm volatile("" : "+v"(ones_off));
    uint64_t aliveA = __builtin_amdgcn_ballot_w64(true), aliveB = aliveA;
    // The exact form of a bounce is a COLD BLOCK INSIDE the loop (the wave redoes that one bounce of both paths
    // with sqrtf() and '/', writes the same registers, and goes on with fast bounces).  The loop then has no exits besides its
    // end -- the round-2 form left the loop for a "rest of the path, exact" tail, and every such exit edge kept the state of
    // both ping-pong halves alive across the back edge.  (Four bounces per turn -- half as many back-edge copies -- measured in
    // round 3: C2 20.40 against 19.95 ms, the longer body costs the ray-generate part more registers than the copies cost; not kept.)
    const bool fast_ok = eps_allows_rootkey(ta.eps);
    // the request of a path that is already finished (alive bit cleared or throughput zero) is ignored: it cannot
    // reach any output any more (deep all-miss paths, |n| ~ 1e20, are of that kind).  A path at its first bounce is never finished.
    auto redo_stands = [&](const PathPair &in, uint64_t redoA, uint64_t redoB, bool first) __attribute__((always_inline)) {
        if (first) return (redoA | redoB) != 0;
        const bool finA = select_const(aliveA, 1) == 0 || (in.rx.x == 0.0f && in.ry.x == 0.0f && in.rz.x == 0.0f);
        const bool finB = select_const(aliveB, 1) == 0 || (in.rx.y == 0.0f && in.ry.y == 0.0f && in.rz.y == 0.0f);
        return __builtin_amdgcn_ballot_w64((select_const(redoA, 1) != 0 && !finA) || (select_const(redoB, 1) != 0 && !finB)) != 0;
    };
    auto exact_pair = [&](const PathPair &in, PathState &na, PathState &nb, bool first) __attribute__((always_inline)) {
        PathState a = unpack_path(in, 0, aliveA, first), b = unpack_path(in, 1, aliveB, first);
        bounce_ns8_exact<MODE>(sc, tab, a, na, ta);
        bounce_ns8_exact<MODE>(sc, tab, b, nb, ta);
        if (ta.traced && (threadIdx.x & 63) == 0) atomicAdd(ta.traced + 3, 1ull); // statistics: exact re-runs of a wave-bounce
    };
#ifdef APT_COUNT_PAIR_SKIP   // measurement build only (make variant ... EXTRA=-DAPT_COUNT_PAIR_SKIP, profiles/pair_skip_count.py): how often
    // pair_misses_wave() holds, per path half, bounce and sphere pair.  The statistics block must then have 4 + 8 * 8 + 1 entries:
    // [4 + (half * 8 + min(bounce, 7)) * 4 + pair] += 1 per wave where it holds, [68] += 1 per wave and path pair it traces.
    uint32_t count_bounce = 0;
    auto count_pairs = [&](const PathPair &in) __attribute__((always_inline)) {
        if (!ta.traced) return;
        const bool lane0 = (threadIdx.x & 63) == 0;
        for (int half = 0; half < 2; ++half) {
            const float ox = half ? in.ox.y : in.ox.x, oy = half ? in.oy.y : in.oy.x, oz = half ? in.oz.y : in.oz.x;
            const float dx = half ? in.dx.y : in.dx.x, dy = half ? in.dy.y : in.dy.x, dz = half ? in.dz.y : in.dz.x;
            HitPre2 hp[4];
            f2 c67 = {0.0f, 0.0f};
            if (PLANES) intersect_pre_planes<true>(sc, ox, oy, oz, dx, dy, dz, hp, &c67);
            for (int k = 0; k < 8; k += 2) {
                const HitPre2 h = PLANES ? hp[k / 2]
                                         : intersect_pre2(f2{sc.cx[k], sc.cx[k + 1]}, f2{sc.cy[k], sc.cy[k + 1]}, f2{sc.cz[k], sc.cz[k + 1]},
                                                          f2{sc.r2[k], sc.r2[k + 1]}, ox, oy, oz, dx, dy, dz);
                const uint32_t slot = 4u + (uint32_t)(half * 8 + (count_bounce < 7u ? count_bounce : 7u)) * 4u + (uint32_t)(k / 2);
                if (pair_misses_wave(h.disc) && lane0) atomicAdd(ta.traced + slot, 1ull);
                if (PLANES && k == 6) {   // pair (6,7) per sphere, with direction (profiles/pair67_split_counts.json): the block then needs 72 + 16 * 4 entries
                    // [72 + (half * 8 + bounce) * 4 + j] += 1 per wave where no lane can hit  j = 0: sphere 6   1: sphere 7   2: either
                    // (sphere_reachable_mask, what the kernel tests);  3: either, by the unguarded statement disc < 0 or NaN or (b < 0 and c > 0)
                    const uint32_t s67 = 72u + (uint32_t)(half * 8 + (count_bounce < 7u ? count_bounce : 7u)) * 4u;
                    const bool u6 = sphere_reachable_mask(h.disc.x, h.b.x, c67.x) == 0, u7 = sphere_reachable_mask(h.disc.y, h.b.y, c67.y) == 0;
                    const bool r6 = h.disc.x >= 0.0f && !(h.b.x < 0.0f && c67.x > 0.0f), r7 = h.disc.y >= 0.0f && !(h.b.y < 0.0f && c67.y > 0.0f);
                    const bool plain = __builtin_amdgcn_ballot_w64(r6 || r7) == 0;
                    if (u6 && lane0) atomicAdd(ta.traced + s67, 1ull);
                    if (u7 && lane0) atomicAdd(ta.traced + s67 + 1, 1ull);
                    if (u6 && u7 && lane0) atomicAdd(ta.traced + s67 + 2, 1ull);
                    if (plain && lane0) atomicAdd(ta.traced + s67 + 3, 1ull);
                }
            }
        }
        if (PLANES) {   // per SPHERE, over the lane's two paths together (profiles/ab_stage_counts.json): the block then needs 424 entries.
            // With bb = min(bounce, 7), one per wave in which, in all 64 lanes and for path A and path B, sphere k
            //   [136 + bb * 8 + k]  cannot be hit by sphere_reachable_mask()'s statement: disc < 0 or NaN, or b < -2^-60 and c > 2^-60
            //   [200 + bb * 8 + k]  the same with the relaxed guard c >= 0
            //   [264 + bb * 8 + k]  has b < -2^-60 and c > 2^-60 (the form that reads no discriminant)
            //   [328 + bb * 8 + k]  has b < -2^-60 and c >= 0
            // and, from the second bounce on, [392 + bb * 4 + j] per wave whose 128 paths have all just left ONE wall w (sphere 0 .. 5):
            //   j = 0 every such wave;  1: w passes the first statement;  2: w passes the relaxed one;  3: the wall opposite w passes the first.
            // b, c and disc are intersect_pre2's, operation for operation (the shared-planes form computes the same per sphere).
            const uint32_t bb = count_bounce < 7u ? count_bounce : 7u;
            auto bcd = [&](int k, float ox, float oy, float oz, float dx, float dy, float dz, float &b, float &c, float &disc) {
                const float x = sc.cx[k] - ox, y = sc.cy[k] - oy, z = sc.cz[k] - oz;
                b = x * dx; b = b + y * dy; b = b + z * dz;
                c = x * x; c = c + y * y; c = c + z * z; c = c - sc.r2[k];
                disc = b * b; disc = disc - c;
            };
            bool strict[8], relaxed[8];
            for (int k = 0; k < 8; ++k) {
                float bA, cA, dA, bB, cB, dB;
                bcd(k, in.ox.x, in.oy.x, in.oz.x, in.dx.x, in.dy.x, in.dz.x, bA, cA, dA);
                bcd(k, in.ox.y, in.oy.y, in.oz.y, in.dx.y, in.dy.y, in.dz.y, bB, cB, dB);
                const bool behindA = bA < -kBehindGuard, behindB = bB < -kBehindGuard;
                const bool reach_s = __builtin_amdgcn_fmed3f(dA, bA, -cA) >= -kBehindGuard || __builtin_amdgcn_fmed3f(dB, bB, -cB) >= -kBehindGuard;
                const bool reach_r = (dA >= 0.0f && !(behindA && cA >= 0.0f)) || (dB >= 0.0f && !(behindB && cB >= 0.0f));
                const bool reach_ns = !(behindA && cA > kBehindGuard && behindB && cB > kBehindGuard);
                const bool reach_nr = !(behindA && cA >= 0.0f && behindB && cB >= 0.0f);
                strict[k] = __builtin_amdgcn_ballot_w64(reach_s) == 0;
                relaxed[k] = __builtin_amdgcn_ballot_w64(reach_r) == 0;
                if (strict[k] && lane0) atomicAdd(ta.traced + 136u + bb * 8u + (uint32_t)k, 1ull);
                if (relaxed[k] && lane0) atomicAdd(ta.traced + 200u + bb * 8u + (uint32_t)k, 1ull);
                if (__builtin_amdgcn_ballot_w64(reach_ns) == 0 && lane0) atomicAdd(ta.traced + 264u + bb * 8u + (uint32_t)k, 1ull);
                if (__builtin_amdgcn_ballot_w64(reach_nr) == 0 && lane0) atomicAdd(ta.traced + 328u + bb * 8u + (uint32_t)k, 1ull);
            }
            if (count_bounce > 0) {
                const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)in.hitA);
                if (w < 6u * 16u && __builtin_amdgcn_ballot_w64(in.hitA != w || in.hitB != w) == 0) {
                    const uint32_t k = w / 16u;
                    bool s = false, r = false, opp = false;
                    for (uint32_t j = 0; j < 6; ++j) {   // (wave-uniform selects: the arrays stay in registers)
                        if (j == k) { s = strict[j]; r = relaxed[j]; }
                        if (j == (k ^ 1u)) opp = strict[j];
                    }
                    if (lane0) {
                        atomicAdd(ta.traced + 392u + bb * 4u, 1ull);
                        if (s) atomicAdd(ta.traced + 393u + bb * 4u, 1ull);
                        if (r) atomicAdd(ta.traced + 394u + bb * 4u, 1ull);
                        if (opp) atomicAdd(ta.traced + 395u + bb * 4u, 1ull);
                    }
                }
            }
        }
        if (count_bounce == 0 && lane0) atomicAdd(ta.traced + 68, 1ull);
        ++count_bounce;
    };
#endif
    auto step = [&](const PathPair &in, PathPair &out, auto first_tag) __attribute__((always_inline)) {
        constexpr bool first = decltype(first_tag)::value;
#ifdef APT_COUNT_PAIR_SKIP
        count_pairs(in);
#endif
        uint64_t oa = aliveA, ob = aliveB;
        bool redo_any = !fast_ok;
        if (__builtin_expect(fast_ok, 1)) {
            uint64_t redoA, redoB;
            bounce2_ns8_t<MODE, PLANES, first, PLAN && PLANES>(sc, tab, in, out, ta, kc, ones_off, oa, ob, redoA, redoB, plan);
            if (__builtin_expect((redoA | redoB) != 0, 0)) redo_any = redo_stands(in, redoA, redoB, first);
        }
        if (__builtin_expect(redo_any, 0)) {
            PathState na, nb;
            exact_pair(in, na, nb, first);
            out.ox = f2{na.oxy.x, nb.oxy.x}; out.oy = f2{na.oxy.y, nb.oxy.y}; out.oz = f2{na.oz, nb.oz};
            out.dx = f2{na.dxy.x, nb.dxy.x}; out.dy = f2{na.dxy.y, nb.dxy.y}; out.dz = f2{na.dz, nb.dz};
            out.rx = f2{na.rxy.x, nb.rxy.x}; out.ry = f2{na.rxy.y, nb.rxy.y}; out.rz = f2{na.rz, nb.rz};
            oa = __builtin_amdgcn_ballot_w64(na.alive != 0);
            ob = __builtin_amdgcn_ballot_w64(nb.alive != 0);
#ifdef APT_COUNT_PAIR_SKIP
            out.hitA = ~0u; out.hitB = ~0u;   // the exact form does not say which sphere it hit: such a wave counts under no wall
#endif
        }
        aliveA = oa; aliveB = ob;
    };
    // The last bounce, state in `in`: throughputs -> s.  Its exact form is the whole exact bounce with the ray ignored.
    auto last = [&](const PathPair &in, auto first_tag) __attribute__((always_inline)) {
        constexpr bool first = decltype(first_tag)::value;
#ifdef APT_COUNT_PAIR_SKIP
        count_pairs(in);
#endif
        uint64_t oa = aliveA, ob = aliveB; // (nothing reads the alive masks after this bounce: they are not written back)
        f2 rx, ry, rz;
        bool redo_any = !fast_ok;
        if (__builtin_expect(fast_ok, 1)) {
            uint64_t redoA, redoB;
            bounce2_ns8_last<MODE, PLANES, first, PLAN && PLANES>(sc, tab, in, rx, ry, rz, ta, kc, ones_off, oa, ob, redoA, redoB, plan);
            if (__builtin_expect((redoA | redoB) != 0, 0)) redo_any = redo_stands(in, redoA, redoB, first);
        }
        if (__builtin_expect(redo_any, 0)) {
            PathState na, nb;
            exact_pair(in, na, nb, first);
            rx = f2{na.rxy.x, nb.rxy.x}; ry = f2{na.rxy.y, nb.rxy.y}; rz = f2{na.rz, nb.rz};
        }
        s.rx = rx; s.ry = ry; s.rz = rz;
    };
    using Yes = std::true_type;   // "this is the pair's first bounce", as a type: the lambdas pick their bounce form by it
    using No = std::false_type;
    if (ta.depth == 0) {
        const f2 one = {1.0f, 1.0f};
        s.rx = one; s.ry = one; s.rz = one;                    // render.cpp:116-121
        return;
    }
    if (ta.depth == 1) {
        last(s, Yes{});
        return;
    }
    const uint32_t full = ta.depth - 1; // bounces whose ray is traced on (>= 1)
    PathPair n;
    step(s, n, Yes{});
    uint32_t d = 1;
    for (; d + 2 <= full; d += 2) { // render.cpp:140-188
        step(n, s, No{});
        step(s, n, No{});
    }
    if (d < full) {
        step(n, s, No{});
        last(s, No{});
    } else {
        last(n, No{});
    }
}

// `planes`: scene8_shares_planes(sc), evaluated once per wave by the kernel (wave-uniform branch around two copies of the loop)
// PLAN: the caller's rays are camera rays and `plan` their wave's first-bounce plan (the frame kernel); read by the shared-planes arm only.
template <int MODE, bool PLAN = false>
__device__ __forceinline__ void trace2_ns8(const Scene8 &sc, const Tab8 tab, PathPair &s, const TraceArgs &ta, bool planes, uint32_t plan = 0) {
    if (planes) {
        // scene8_shares_planes() compared these bit for bit: naming each shared coordinate ONCE lets this arm -- its exact cold block
        // included -- keep 13 centre coordinates in scalar registers instead of 24 (the (A, B)-packed intersection holds both paths'
        // index accumulators at once and has no room for the rest).
        Scene8 p = sc;
        p.cx[3] = p.cx[4] = p.cx[5] = p.cx[7] = sc.cx[2];
        p.cy[1] = p.cy[2] = p.cy[3] = sc.cy[0];
        p.cz[1] = p.cz[4] = p.cz[5] = p.cz[7] = sc.cz[0];
        trace2_ns8_t<MODE, true, PLAN>(p, tab, s, ta, plan);
    } else {
        trace2_ns8_t<MODE, false>(sc, tab, s, ta);
    }
}

} // namespace
