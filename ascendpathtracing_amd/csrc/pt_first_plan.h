// pt_first_plan.h -- the first-bounce plan of the two-path frame kernel (pt_trace2.h): which of the 8 spheres of the reference room a
// pixel's camera rays cannot hit FIRST, decided from the pixel's column and row alone.  One text for the kernel that makes the record
// (first_plan.hip first_plan_kernel), the frame kernel that reads it (first_plan_mask) and the CPU twin (first_plan_host.cpp
// apt_first_plan_host).  Everything is float64 interval arithmetic over a pixel RANGE's whole jitter footprint: sub-pixel offsets span
// [i - 0.25, i + 1.25) (camera_ray_t: ((sx + 0.5 + tent) / 2 + i, sx in {0, 1}, tent in [-1, 1)), and with the reference's camera frame
// (cx = (cx0, 0, 0), cy = (0, cy1, cy2), g = (0, g1, g2): camera_init checks it) d0 depends on the column and d1, d2 on the row only,
// each linearly, so the bounds of a range are its endpoints'.  Every entry of the record is the largest range for which a predicate
// holds OVER THE WHOLE RANGE, found by bisection; the entry returned is one the predicate was evaluated for, so the record is sound
// whether or not the predicate is monotone.  Compiled with -ffp-contract=off.
//
// The record (kFirstPlanWords int32; all zero = skip nothing, and so is every entry a failed premise returns):
//   [0], [1]  wall_cols [lo, hi)     [2], [3]  wall_rows [lo, hi): where the wall rules may be used at all
//   [4]  sphere 0 (centre beyond +x): the last [4] columns     [5]  sphere 1 (beyond -x): the first [5] columns
//   [6]  sphere 4 (beyond +y): the last [6] rows               [7]  sphere 5 (beyond -y): the first [7] rows
//   [8]  sphere 3 (beyond -z: every camera ray runs towards its centre): a flag
//   [9] .. [12]  the ball (sphere 6) is out of reach in the first [9] / last [10] columns and the first [11] / last [12] rows
//   [13] the light (sphere 7) is out of reach in the first [13] rows
//
// PREMISES (first_plan_setup; one fails -> skip nothing): the reference camera frame with d2 < 0 everywhere; the table passes
// scene8_shares_planes()'s pattern; 0 < eps <= 1; spheres 0 .. 5 are the room -- radius in [5e4, 1.3e5], centres beyond the room on
// +x, -x, +z, -z, +y, -y in that order, the room box [xlo, xhi] x [ylo, yhi] x [zlo, zhi] between their near faces no larger than
// 1000, the centre pixel's origins at least m inside it -- so that |C - o|^2 < 2^34 and the fp32 error bounds below hold.
//
// WALL RULE.  Skipped wall k, pixel inside wall_cols x wall_rows, any ray (o, d) of the pixel, fp32 quantities as the kernel computes
// them (b = (px + py) + pz, c = ((qx + qy) + qz) - r2, disc = b*b - c, q = RN(sqrt(disc)), keys of -t0 = q - b and t1 = b + q):
//  (a) o lies inside the room box and at least m = 4 inside each of the six wall spheres: exact c_j <= -(2 R_j m - m^2) - 3072 for
//      every j.  The fp32 error of c_j is < 3072: the one large coordinate difference t (|t| < 2^17, error <= 2^-8) squares to
//      < 2^34 with error <= 2 * 2^17 * 2^-8 + 512, the two additions round by <= 512 each, the subtraction of r2 is exact or rounds
//      by <= 512 (3 ulp(2^33) in all).  So every computed c_j < 0.  The room is the intersection of the six balls and lies in
//      the box, so in exact arithmetic the ray leaves it through some wall j at t1_j in [m, D], D the box's diagonal; j is not k
//      (by (b), t1_k > D).  For that j, |b_j| <= max(q_j, D) and q_j >= sqrt(2 R_j m - m^2) >= 632, so the computed root differs from
//      t1_j by < 3072 / (2 * 632) + 0.1 < 2.6: it lies in (1.4, D + 4] = (eps, T_hi], and its key is <= key(T_hi).
//  (b) computed b_k >= B_lo - 1 > T_hi: the term along k's own axis is >= |C_k - far face| * |d_axis|_min / |d|_max, the other two are
//      bounded by the room's extent (|d component| <= 1), and the fp32 error of b is < 0.1 (three products < 2^17, each operand
//      rounded once).  With the computed c_k < 0: disc >= RN(b*b), q >= |b|, so -t0 = q - b >= 0 -- t0 <= 0 <= eps, its key is
//      >= key(kMissT) -- and t1 = RN(b + q) >= b > T_hi.  Both keys are strictly above the winner's: sphere k's v_min3_u32 leaves
//      the FINAL `best` what it is and sets no bit that survives (a later, strictly smaller key rewrites all three index bits and, in
//      O-mode, `any` has the winner's lane either way), and no tie rule is touched.
//  (c) k's share of `amin` could only have asked for the exact re-run, which finds the same winner (pt_trace.h, above
//      intersect_ns8_v2's SKIP).
// BALL RULE (and the light's first form).  Every camera ray lies on a line through cam.pos (o = pos + 140 d).  Projected on the
// (x, z) or (y, z) plane -- a projection shortens no distance, so a projected miss is a miss -- the line passes the centre at more than
// rho, rho^2 = r2 + 4 + r2 * 2^-12: N^2 < (|w|^2 - rho^2) |d|^2 with w = C - pos, N = w . d, bounded over the range.  Then the exact
// disc <= -(4 + r2 * 2^-12), against an fp32 error of disc below 0.01 (ball: magnitudes <= 2^15) / 1 (light: <= 2^20), the rounding of
// o and d included: the computed disc is negative, sphere_reachable_mask()'s case (a).
// LIGHT RULE, second form: c >= 4 + r2 * 2^-12 and b <= -1 over the range, far above 2^-60: sphere_reachable_mask()'s case (b).
#pragma once
#include "pt_core.h"

namespace apt {

constexpr int kFirstPlanWords = 16;
// Where a context keeps its records on a device: kFirstPlanSlots records of kFirstPlanWords 64-bit entries behind its status word, from
// 32-bit word kFirstPlanBase of that allocation on.  An entry is (value, low 32 bits of the launch's ticket), written with ONE 64-bit
// store.  A launch of the two-path frame kernel takes a ticket (a 64-bit count that starts at 1 and never repeats), its plan kernel
// writes slot ticket % kFirstPlanSlots, and the frame kernel takes a record only when EVERY entry it reads carries its own ticket
// (pt_kernels.h: one entry per lane, one ballot): a slot that another launch has taken since -- 64 launches later on another stream, or an eager launch cycling
// through the slot a captured graph keeps -- shows a foreign ticket in the entries that launch has written, and the wave that sees one
// skips nothing.  So a record is never read as another launch's, whatever runs at the same time; sharing a slot can only cost speed.
// (Two tickets agree in their low 32 bits only 2^32 launches apart.)
constexpr uint32_t kFirstPlanBase = 16, kFirstPlanSlots = 64;
constexpr uint32_t kFirstPlanAllocWords = kFirstPlanBase + kFirstPlanSlots * (uint32_t)kFirstPlanWords * 2u;
APT_HD uint64_t first_plan_pack(int32_t value, uint64_t ticket) { return (uint64_t)(uint32_t)value | ((uint64_t)(uint32_t)ticket << 32); }
APT_HD uint32_t first_plan_slot_word(uint64_t ticket) { return kFirstPlanBase + (uint32_t)(ticket % kFirstPlanSlots) * (uint32_t)kFirstPlanWords * 2u; }
constexpr double kFirstPlanDepth = 4.0;      // m of (a)
constexpr double kFirstPlanCErr = 3072.0;    // fp32 error bound of a wall's c
constexpr double kFirstPlanMaxEps = 1.0;
constexpr uint32_t kFirstPlanMaxSide = 1u << 24;   // a wider or higher frame has no plan: no record (first_plan_setup), no ticket (render_kernels.hip), no mask

struct FpIv { double lo, hi; };
APT_HD FpIv fp_lin(double c, FpIv x, double g) { return c >= 0 ? FpIv{c * x.lo + g, c * x.hi + g} : FpIv{c * x.hi + g, c * x.lo + g}; }
APT_HD double fp_min(double a, double b) { return a < b ? a : b; }
APT_HD double fp_max(double a, double b) { return a > b ? a : b; }
APT_HD double fp_minabs(FpIv x) { return (x.lo <= 0 && x.hi >= 0) ? 0.0 : fp_min(fabs(x.lo), fabs(x.hi)); }
APT_HD double fp_maxabs(FpIv x) { return fp_max(fabs(x.lo), fabs(x.hi)); }
APT_HD FpIv fp_mul(FpIv a, FpIv b) {
    const double p0 = a.lo * b.lo, p1 = a.lo * b.hi, p2 = a.hi * b.lo, p3 = a.hi * b.hi;
    return FpIv{fp_min(fp_min(p0, p1), fp_min(p2, p3)), fp_max(fp_max(p0, p1), fp_max(p2, p3))};
}
APT_HD FpIv fp_from(double c, FpIv x) { return FpIv{c - x.hi, c - x.lo}; }   // c - x

// What every entry is made from.  ok == false: skip nothing.
struct FirstPlanGeom {
    bool ok;
    double cx0, cy1, cy2, g1, g2, pos[3];
    int32_t w, h;
    double C[8][3], r2[8], R[6];
    double lo[3], hi[3];       // the room box
    double D;                  // its diagonal
    double nmin2, nmax;        // bounds of |d|^2 / |d| over the frame
    FpIv d0all, d1all, d2all;
};

// the jitter footprint of columns / rows [i0, i1] as camera_ray_t's a / b, widened by 1e-9
APT_HD FpIv fp_footprint(int32_t i0, int32_t i1, int32_t n) {
    return FpIv{((double)i0 - 0.25) / (double)n - 0.5 - 1e-9, ((double)i1 + 1.25) / (double)n - 0.5 + 1e-9};
}
APT_HD FpIv fp_d0(const FirstPlanGeom &g, int32_t i0, int32_t i1) { return fp_lin(g.cx0, fp_footprint(i0, i1, g.w), 0.0); }
APT_HD FpIv fp_d1(const FirstPlanGeom &g, int32_t j0, int32_t j1) { return fp_lin(g.cy1, fp_footprint(j0, j1, g.h), g.g1); }
APT_HD FpIv fp_d2(const FirstPlanGeom &g, int32_t j0, int32_t j1) { return fp_lin(g.cy2, fp_footprint(j0, j1, g.h), g.g2); }
// the origins pos + 140 d of a range, widened by more than their fp32 rounding
APT_HD FpIv fp_origin(double pos, FpIv d) { return FpIv{pos + 140.0 * d.lo - 0x1p-10, pos + 140.0 * d.hi + 0x1p-10}; }

// sph: the device table's layout, [10][8] floats, rows r2, x, y, z, ...
APT_HD void first_plan_setup(const Camera &cam, uint32_t width, uint32_t height, const float *sph, float eps, FirstPlanGeom &g) {
    g.ok = false;
    if (!(cam.cx[1] == 0 && cam.cx[2] == 0 && cam.cy[0] == 0 && cam.g[0] == 0 && cam.cx[0] > 0)) return;
    if (!(width >= 1 && height >= 1 && width <= kFirstPlanMaxSide && height <= kFirstPlanMaxSide)) return;
    if (!(eps_allows_rootkey(eps) && (double)eps <= kFirstPlanMaxEps)) return;
    g.cx0 = cam.cx[0]; g.cy1 = cam.cy[1]; g.cy2 = cam.cy[2]; g.g1 = cam.g[1]; g.g2 = cam.g[2];
    g.pos[0] = cam.pos[0]; g.pos[1] = cam.pos[1]; g.pos[2] = cam.pos[2];
    g.w = (int32_t)width; g.h = (int32_t)height;
    const float *fx = sph + 8, *fy = sph + 16, *fz = sph + 24;
    auto eq = [](float a, float b) { return f32_bits(a) == f32_bits(b); };   // scene8_shares_planes()'s pattern
    if (!(eq(fx[2], fx[3]) && eq(fx[2], fx[4]) && eq(fx[2], fx[5]) && eq(fx[2], fx[7]) && eq(fy[0], fy[1]) && eq(fy[0], fy[2]) &&
          eq(fy[0], fy[3]) && eq(fz[0], fz[1]) && eq(fz[0], fz[4]) && eq(fz[0], fz[5]) && eq(fz[0], fz[7]))) return;
    for (int k = 0; k < 8; ++k) {
        g.r2[k] = (double)sph[k]; g.C[k][0] = (double)fx[k]; g.C[k][1] = (double)fy[k]; g.C[k][2] = (double)fz[k];
        if (!(g.r2[k] > 0 && g.r2[k] < 0x1p60 && fabs(g.C[k][0]) < 0x1p30 && fabs(g.C[k][1]) < 0x1p30 && fabs(g.C[k][2]) < 0x1p30)) return;
    }
    for (int k = 0; k < 6; ++k) {
        g.R[k] = sqrt(g.r2[k]);
        if (!(g.R[k] >= 5e4 && g.R[k] <= 1.3e5)) return;
    }
    // the room: spheres 0 / 1 beyond +x / -x, 2 / 3 beyond +z / -z, 4 / 5 beyond +y / -y
    g.lo[0] = g.C[0][0] - g.R[0]; g.hi[0] = g.C[1][0] + g.R[1];
    g.lo[2] = g.C[2][2] - g.R[2]; g.hi[2] = g.C[3][2] + g.R[3];
    g.lo[1] = g.C[4][1] - g.R[4]; g.hi[1] = g.C[5][1] + g.R[5];
    for (int a = 0; a < 3; ++a)
        if (!(g.hi[a] - g.lo[a] >= 2 * kFirstPlanDepth && g.hi[a] - g.lo[a] <= 1000.0 && fabs(g.lo[a]) <= 1000.0 && fabs(g.hi[a]) <= 1000.0)) return;
    if (!(g.C[0][0] > g.hi[0] && g.C[1][0] < g.lo[0] && g.C[2][2] > g.hi[2] && g.C[3][2] < g.lo[2] && g.C[4][1] > g.hi[1] && g.C[5][1] < g.lo[1])) return;
    // the walls' other coordinates lie within 1000 of the room as well (the shared planes do: checked, not assumed)
    for (int k = 0; k < 6; ++k) {
        const int own = k < 2 ? 0 : (k < 4 ? 2 : 1);
        for (int a = 0; a < 3; ++a)
            if (a != own && !(fabs(g.C[k][a]) <= 1000.0)) return;
    }
    const double ex = g.hi[0] - g.lo[0], ey = g.hi[1] - g.lo[1], ez = g.hi[2] - g.lo[2];
    g.D = sqrt(ex * ex + ey * ey + ez * ez);
    g.d0all = fp_d0(g, 0, g.w - 1); g.d1all = fp_d1(g, 0, g.h - 1); g.d2all = fp_d2(g, 0, g.h - 1);
    if (!(g.d2all.hi < 0)) return;
    const double a0 = fp_maxabs(g.d0all), a1 = fp_maxabs(g.d1all), a2 = fp_maxabs(g.d2all);
    const double i0 = fp_minabs(g.d0all), i1 = fp_minabs(g.d1all), i2 = fp_minabs(g.d2all);
    g.nmax = sqrt(a0 * a0 + a1 * a1 + a2 * a2) * (1 + 1e-9);
    g.nmin2 = (i0 * i0 + i1 * i1 + i2 * i2) * (1 - 1e-9);
    if (!(g.nmin2 > 0x1p-20 && g.nmax < 0x1p10)) return;
    g.ok = true;
}

// The last premise, made after the setup above (it needs the predicates below): the centre pixel's origins lie in the room.  A camera
// whose origins do not is not the one the rules were written for, and the record then skips nothing at all.
APT_HD void first_plan_premise_origin(FirstPlanGeom &g);

// largest n in [0, nmax] with P(n); P(0) is not evaluated (an empty range).  The n returned is 0 or one P held for.
template <class F>
APT_HD int32_t fp_largest(int32_t nmax, F P) {
    int32_t lo = 0, hi = nmax;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (P(mid)) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// (a) for the walls of one axis set: the origin coordinates `o` (axis ax; for rows both y and z are handed in through two calls) lie in
// the box, and wall k's c is below the bound when the other coordinates are anywhere in the box.
APT_HD bool fp_inside_wall(const FirstPlanGeom &g, int k, int ax, FpIv o) {
    if (!(o.lo >= g.lo[ax] && o.hi <= g.hi[ax])) return false;
    double s = 0;
    for (int a = 0; a < 3; ++a) {
        const FpIv span = a == ax ? o : FpIv{g.lo[a], g.hi[a]};
        const double m = fp_maxabs(fp_from(g.C[k][a], span));
        s = s + m * m;
    }
    const double need = 2 * g.R[k] * kFirstPlanDepth - kFirstPlanDepth * kFirstPlanDepth + kFirstPlanCErr;
    return s - g.r2[k] <= -need;
}
// (a) for a column range: the c of the two x walls with x from the range, y and z anywhere in the box
APT_HD bool fp_cols_inside(const FirstPlanGeom &g, int32_t i0, int32_t i1) {
    const FpIv o = fp_origin(g.pos[0], fp_d0(g, i0, i1));
    return fp_inside_wall(g, 0, 0, o) && fp_inside_wall(g, 1, 0, o);   // (the other four walls: fp_rows_inside, x anywhere in the box)
}
// (a) for a row range: the c of the z and y walls with y and z from the range, x anywhere in the box
APT_HD bool fp_rows_inside(const FirstPlanGeom &g, int32_t j0, int32_t j1) {
    const FpIv oy = fp_origin(g.pos[1], fp_d1(g, j0, j1)), oz = fp_origin(g.pos[2], fp_d2(g, j0, j1));
    if (!(oy.lo >= g.lo[1] && oy.hi <= g.hi[1] && oz.lo >= g.lo[2] && oz.hi <= g.hi[2])) return false;
    bool ok = true;
    for (int k = 2; k < 6; ++k) {
        double s = 0;
        for (int a = 0; a < 3; ++a) {
            const FpIv span = a == 1 ? oy : (a == 2 ? oz : FpIv{g.lo[0], g.hi[0]});
            const double m = fp_maxabs(fp_from(g.C[k][a], span));
            s = s + m * m;
        }
        const double need = 2 * g.R[k] * kFirstPlanDepth - kFirstPlanDepth * kFirstPlanDepth + kFirstPlanCErr;
        ok = ok && s - g.r2[k] <= -need;
    }
    return ok;
}
APT_HD void first_plan_premise_origin(FirstPlanGeom &g) {
    if (g.ok && !(fp_cols_inside(g, g.w / 2, g.w / 2) && fp_rows_inside(g, g.h / 2, g.h / 2))) g.ok = false;
}
// (b) for wall k on axis ax with its centre on side sgn: dcomp is the range's unnormalised direction component along ax
APT_HD bool fp_wall_far(const FirstPlanGeom &g, int k, int ax, double sgn, FpIv dcomp) {
    const double toward = sgn > 0 ? dcomp.lo : -dcomp.hi;            // the least component towards the centre
    if (!(toward > 0)) return false;
    const double reach = sgn > 0 ? g.C[k][ax] - g.hi[ax] : g.lo[ax] - g.C[k][ax];   // centre to the far face of the box
    double other = 0;
    for (int a = 0; a < 3; ++a)
        if (a != ax) other = other + fp_maxabs(fp_from(g.C[k][a], FpIv{g.lo[a], g.hi[a]})) * (1 + 0x1p-20);
    const double blo = reach * toward / g.nmax - other - 1.0;
    return blo > g.D + 4.0 + 1.0;
}
// The projected miss of sphere k on the plane (ax, z): dp / dz the range's unnormalised components
APT_HD bool fp_line_misses(const FirstPlanGeom &g, int k, int ax, FpIv dp, FpIv dz) {
    const double wp = g.C[k][ax] - g.pos[ax], wz = g.C[k][2] - g.pos[2];
    const double rho2 = g.r2[k] + 4.0 + g.r2[k] * 0x1p-12;
    const double gap = wp * wp + wz * wz - rho2;
    if (!(gap > 0)) return false;
    const FpIv tp = fp_lin(wp, dp, 0.0), tz = fp_lin(wz, dz, 0.0);
    const double nabs = fp_max(fabs(tp.lo + tz.lo), fabs(tp.hi + tz.hi)) * (1 + 1e-9);
    const double ip = fp_minabs(dp), iz = fp_minabs(dz);
    return nabs * nabs < gap * (ip * ip + iz * iz) * (1 - 1e-9);
}
// The light behind every ray of rows [j0, j1], all columns: c >= margin and b <= -1
APT_HD bool fp_light_behind(const FirstPlanGeom &g, int32_t j0, int32_t j1) {
    const FpIv d[3] = {g.d0all, fp_d1(g, j0, j1), fp_d2(g, j0, j1)};
    double cmin = 0, bhi = 0;
    for (int a = 0; a < 3; ++a) {
        const FpIv t = fp_from(g.C[7][a], fp_origin(g.pos[a], d[a]));
        const double m = fp_minabs(t);
        cmin = cmin + m * m;
        bhi = bhi + fp_mul(t, d[a]).hi;
    }
    if (!(cmin - g.r2[7] >= 4.0 + g.r2[7] * 0x1p-12)) return false;
    return bhi < 0 && bhi / g.nmax <= -1.0;
}

// Entry `which` of the record.
APT_HD int32_t first_plan_entry(const FirstPlanGeom &g, int which) {
    if (!g.ok || which < 0 || which > 13) return 0;
    const int32_t w = g.w, h = g.h, mc = w / 2, mr = h / 2;
    switch (which) {
    case 0: case 1: {
        if (!fp_cols_inside(g, mc, mc)) return 0;
        if (which == 0) return mc - fp_largest(mc, [&](int32_t n) { return fp_cols_inside(g, mc - n, mc); });
        return mc + 1 + fp_largest(w - 1 - mc, [&](int32_t n) { return fp_cols_inside(g, mc, mc + n); });
    }
    case 2: case 3: {
        if (!fp_rows_inside(g, mr, mr)) return 0;
        if (which == 2) return mr - fp_largest(mr, [&](int32_t n) { return fp_rows_inside(g, mr - n, mr); });
        return mr + 1 + fp_largest(h - 1 - mr, [&](int32_t n) { return fp_rows_inside(g, mr, mr + n); });
    }
    case 4: return fp_largest(w, [&](int32_t n) { return fp_wall_far(g, 0, 0, 1.0, fp_d0(g, w - n, w - 1)); });
    case 5: return fp_largest(w, [&](int32_t n) { return fp_wall_far(g, 1, 0, -1.0, fp_d0(g, 0, n - 1)); });
    case 6: return fp_largest(h, [&](int32_t n) { return fp_wall_far(g, 4, 1, 1.0, fp_d1(g, h - n, h - 1)); });
    case 7: return fp_largest(h, [&](int32_t n) { return fp_wall_far(g, 5, 1, -1.0, fp_d1(g, 0, n - 1)); });
    case 8: return fp_wall_far(g, 3, 2, -1.0, g.d2all) ? 1 : 0;
    case 9: return fp_largest(w, [&](int32_t n) { return fp_line_misses(g, 6, 0, fp_d0(g, 0, n - 1), g.d2all); });
    case 10: return fp_largest(w, [&](int32_t n) { return fp_line_misses(g, 6, 0, fp_d0(g, w - n, w - 1), g.d2all); });
    case 11: return fp_largest(h, [&](int32_t n) { return fp_line_misses(g, 6, 1, fp_d1(g, 0, n - 1), fp_d2(g, 0, n - 1)); });
    case 12: return fp_largest(h, [&](int32_t n) { return fp_line_misses(g, 6, 1, fp_d1(g, h - n, h - 1), fp_d2(g, h - n, h - 1)); });
    default: {
        const int32_t miss = fp_largest(h, [&](int32_t n) { return fp_line_misses(g, 7, 1, fp_d1(g, 0, n - 1), fp_d2(g, 0, n - 1)); });
        const int32_t behind = fp_largest(h, [&](int32_t n) { return fp_light_behind(g, 0, n - 1); });
        return miss > behind ? miss : behind;
    }
    }
}

// The spheres a pixel's camera rays cannot hit first (bit k = sphere k), from the record -- in two steps, so that the frame kernel can take
// the first one entry per lane: first_plan_cond(k, ...) is entry k's own comparison with the pixel's column or row, and
// first_plan_combine() makes the mask from the 14 results (bit k of `conds` = entry k's).
// (int32 comparisons: for width, height <= kFirstPlanMaxSide only.  From 2^31 on n - r wraps and the all-zero record would mark the ball
// everywhere; such a launch gets no ticket and never comes here, and first_plan_mask() answers 0 for it.)
APT_HD bool first_plan_cond(uint32_t k, int32_t r, uint32_t width, uint32_t height, uint32_t col, uint32_t row) {
    const bool on_col = k == 0 || k == 1 || k == 4 || k == 5 || k == 9 || k == 10;
    const int32_t x = on_col ? (int32_t)col : (int32_t)row, n = on_col ? (int32_t)width : (int32_t)height;
    const bool from_end = k == 4 || k == 6 || k == 10 || k == 12;          // "the last r": x >= n - r
    const bool at_least = k == 0 || k == 2 || from_end;
    const int32_t t = from_end ? n - r : r;
    if (k == 8) return r != 0;
    return at_least ? x >= t : x < t;
}
APT_HD uint32_t first_plan_combine(uint32_t conds) {
    uint32_t m = 0;
    if ((conds & 0xFu) == 0xFu)                                             // inside wall_cols x wall_rows
        m = ((conds >> 4) & 1u) | (((conds >> 5) & 1u) << 1) | (((conds >> 8) & 1u) << 3) | (((conds >> 6) & 1u) << 4) | (((conds >> 7) & 1u) << 5);
    m |= (conds & 0x1E00u) ? 64u : 0u;                                      // outside the ball's rectangle on any side
    m |= ((conds >> 13) & 1u) << 7;
    return m;
}
APT_HD uint32_t first_plan_mask(const int32_t *r, uint32_t width, uint32_t height, uint32_t col, uint32_t row) {
    if (width > kFirstPlanMaxSide || height > kFirstPlanMaxSide) return 0;
    uint32_t conds = 0;
    for (uint32_t k = 0; k < 14; ++k) conds |= first_plan_cond(k, r[k], width, height, col, row) ? 1u << k : 0u;
    return first_plan_combine(conds);
}

} // namespace apt
