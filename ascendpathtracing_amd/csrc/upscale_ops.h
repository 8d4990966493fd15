// upscale_ops.h -- the arithmetic of libupscale_mi355x.so (include/render_mi355x_upscale.h), each step once and per pixel: the header's
// coordinates one float64 operation per line, its prepare, guided sum, decision and patch one fp32 operation per line
// (-ffp-contract=off on both sides).  upscale.hip's kernels are a lane mapping and a call, upscale_host.cpp's CPU twins a loop and the
// same call: that is why they give the same bits.  Nothing of HIP is needed to compile it.
//
// The work buffer holds per-low-pixel 16-byte records, pixel (x, y) at x * lo_height + y as in every plane: ci = (i.rgb, cov),
// gn = (n.xyz, z), ga = (A.rgb, 0).
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/render_mi355x_upscale.h"
#include "apt_hd.h"
#include "film_stage_ops.h"

namespace apt {

constexpr uint32_t kUpBlock = 256;   // lanes per workgroup of the three kernels

using UpRec = FsRec;                 // one record of the work buffer

struct UpArgs {
    const float *lo, *lf, *hf;       // the low mean [3][Nl], the low and the full planes
    UpRec *ci, *gn, *ga;             // the three record arrays of `work`
    float *out;
    uint32_t *resolved;
    uint32_t lw, lh, w, h;
    float sn, sz, sc, sa, albedo_floor, min_weight;
};

// ---- prepare: the three records of low pixel i of n ----------------------------------------------------------------------------------
APT_HD void up_prepare(const UpArgs &A, uint64_t n, uint64_t i) {
    const float cov = A.lf[APT_FEATURE_COVERAGE * n + i];
    const float u = fs_uncovered(cov);
    float al[3], il[3];
    APT_UNROLL
    for (uint64_t ch = 0; ch < 3; ++ch) {
        al[ch] = fs_albedo(A.lf[(APT_FEATURE_ALBEDO + ch) * n + i], u, A.albedo_floor);
        il[ch] = A.lo[ch * n + i] / al[ch];
    }
    A.ci[i] = UpRec{il[0], il[1], il[2], cov};
    A.gn[i] = UpRec{A.lf[APT_FEATURE_NORMAL * n + i], A.lf[(APT_FEATURE_NORMAL + 1) * n + i], A.lf[(APT_FEATURE_NORMAL + 2) * n + i],
                    A.lf[APT_FEATURE_DEPTH * n + i]};
    A.ga[i] = UpRec{al[0], al[1], al[2], 0.0f};
}

// One axis of the coordinates: pixel k of `full` pixels over `low` ones -> the first tap's coordinate k0 and the fraction f.
APT_HD void up_axis(uint32_t k, uint32_t low, uint32_t full, double *k0, double *f) {
    const double c = (double)k + 0.5;
    const double s = c * (double)low;
    const double u = s / (double)full - 0.5;
    *k0 = floor(u);
    *f = u - *k0;
}

// ---- upsample: pixel (x, y) of the full image, p = x * h + y ---------------------------------------------------------------------------
// The fallback's sums (g = 1) run beside the guided ones over the same taps in the same order.
APT_HD void up_pixel(const UpArgs &A, uint32_t x, uint32_t y) {
    const uint64_t n = (uint64_t)A.w * A.h;
    const uint64_t p = (uint64_t)x * A.h + y;
    const float cov_p = A.hf[APT_FEATURE_COVERAGE * n + p];
    const float z_p = A.hf[APT_FEATURE_DEPTH * n + p];
    const float nx = A.hf[APT_FEATURE_NORMAL * n + p], ny = A.hf[(APT_FEATURE_NORMAL + 1) * n + p], nz = A.hf[(APT_FEATURE_NORMAL + 2) * n + p];
    const float u1 = fs_uncovered(cov_p);
    float Ap[3];
    APT_UNROLL
    for (uint64_t ch = 0; ch < 3; ++ch) Ap[ch] = fs_albedo(A.hf[(APT_FEATURE_ALBEDO + ch) * n + p], u1, A.albedo_floor);
    const float zz = z_p + 1e-6f;
    const float iz = 1.0f / zz;
    const FsGuide gp = {nx, ny, nz, z_p, cov_p, Ap[0], Ap[1], Ap[2]};

    double x0, fx, y0, fy;
    up_axis(x, A.lw, A.w, &x0, &fx);
    up_axis(y, A.lh, A.h, &y0, &fy);
    const double xmax = (double)A.lw - 1.0, ymax = (double)A.lh - 1.0;

    float Wg = 0.0f, Sg[3] = {0.0f, 0.0f, 0.0f};
    float Wf = 0.0f, Sf[3] = {0.0f, 0.0f, 0.0f};
    APT_UNROLL
    for (int ex = 0; ex < 2; ++ex)
        APT_UNROLL
        for (int ey = 0; ey < 2; ++ey) {
            const double qx = x0 + (double)ex, qy = y0 + (double)ey;
            const float b = (float)((ex ? fx : 1.0 - fx) * (ey ? fy : 1.0 - fy));
            if (!(qx >= 0.0 && qx <= xmax && qy >= 0.0 && qy <= ymax)) continue;
            const uint64_t q = (uint64_t)(uint32_t)qx * A.lh + (uint32_t)qy;        // inside the low image: the compares above
            const UpRec c_q = A.ci[q], n_q = A.gn[q], a_q = A.ga[q];
            const FsGuide gq = {n_q.x, n_q.y, n_q.z, n_q.w, c_q.w, a_q.x, a_q.y, a_q.z};
            const FsSigma gs = {A.sn, A.sz, A.sc, A.sa};   // read at the tap, as before: it keeps the kernel's instructions
            const float g = fs_edge_falloff(fs_edge_sum(gp, iz, gq, gs));
            const float w = b * g;
            if (w > 0.0f) {
                Wg = Wg + w;
                Sg[0] = Sg[0] + w * c_q.x;
                Sg[1] = Sg[1] + w * c_q.y;
                Sg[2] = Sg[2] + w * c_q.z;
            }
            if (b > 0.0f) {
                Wf = Wf + b;
                Sf[0] = Sf[0] + b * c_q.x;
                Sf[1] = Sf[1] + b * c_q.y;
                Sf[2] = Sf[2] + b * c_q.z;
            }
        }
    const bool ok = Wg >= A.min_weight;
    const float W = ok ? Wg : Wf;
    APT_UNROLL
    for (uint64_t ch = 0; ch < 3; ++ch) {
        const float ip = (ok ? Sg[ch] : Sf[ch]) / W;
        A.out[ch * n + p] = ip * Ap[ch];
    }
    A.resolved[p] = ok ? 1u : 0u;
}

// ---- patch: entry i of the list's `count` replaces pixel list[i] of n; an entry beyond the image is skipped ----------------------------
APT_HD void up_patch(const float *sums, const uint32_t *list, uint64_t count, float K, uint64_t n, float *out, uint64_t i) {
    const uint64_t p = list[i];
    if (p >= n) return;
    APT_UNROLL
    for (uint64_t c = 0; c < 3; ++c) out[c * n + p] = sums[c * count + i] / K;
}

} // namespace apt
