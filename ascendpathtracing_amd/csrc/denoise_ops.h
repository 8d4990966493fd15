// denoise_ops.h -- the arithmetic of libdenoise_mi355x.so (include/render_mi355x_denoise.h), each step once and per pixel: the header's
// operations one fp32 operation per line (-ffp-contract=off on both sides).  denoise.hip's kernels are a lane mapping and a call,
// denoise_host.cpp's CPU twins a loop and the same call: that is why they give the same bits.  Nothing of HIP is needed to compile it.
//
// The work buffer holds per-pixel 16-byte records, pixel (x, y) at x * height + y as in every plane: g0 = (n.xyz, z), g1 = (A.rgb, cov)
// and two images c = (i.rgb, vi) that the iterations ping-pong between; prepare writes c[0], iteration j reads c[j & 1].
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/render_mi355x_denoise.h"
#include "apt_hd.h"
#include "film_stage_ops.h"

namespace apt {

using DnRec = FsRec;                              // one record of the work buffer
struct DnSigma { float n, z, c, a, l; };          // apt_film_denoise's edge-stopping sigmas: normal, depth, coverage, albedo, luminance

// ---- moments: pixel i of n joins the film and its luminance moments; the first pass stores ------------------------------------------
APT_HD void dn_accumulate(const float *pass, float *film, float *mom, uint64_t n, uint64_t i, bool first) {
    const float r = pass[i], g = pass[n + i], b = pass[2 * n + i];
    const float l = fs_lum(r, g, b);
    const float l2 = l * l;
    if (first) {
        film[i] = r; film[n + i] = g; film[2 * n + i] = b;
        mom[i] = l; mom[n + i] = l2;
    } else {
        film[i] = film[i] + r; film[n + i] = film[n + i] + g; film[2 * n + i] = film[2 * n + i] + b;
        mom[i] = mom[i] + l; mom[n + i] = mom[n + i] + l2;
    }
}

// ---- prepare: the three records of pixel i from the planes; K = passes, K1 = passes - 1 ----------------------------------------------
APT_HD void dn_prepare(const float *film, const float *mom, const float *feat, DnRec *g0, DnRec *g1, DnRec *c0, uint64_t n, uint32_t i, float K,
                       float K1, float albedo_floor) {
    const float cov = feat[APT_FEATURE_COVERAGE * n + i];
    const float u = fs_uncovered(cov);
    float A[3], il[3];
    APT_UNROLL
    for (uint64_t ch = 0; ch < 3; ++ch) {
        const float cm = film[ch * n + i] / K;
        A[ch] = fs_albedo(feat[(APT_FEATURE_ALBEDO + ch) * n + i], u, albedo_floor);
        il[ch] = cm / A[ch];
    }
    const float lm = mom[i] / K, q = mom[n + i] / K;
    const float v = fs_max(q - lm * lm, 0.0f) / K1;
    const float LA = fs_lum(A[0], A[1], A[2]);
    const float vi = v / (LA * LA);
    g0[i] = DnRec{feat[APT_FEATURE_NORMAL * n + i], feat[(APT_FEATURE_NORMAL + 1) * n + i], feat[(APT_FEATURE_NORMAL + 2) * n + i],
                  feat[APT_FEATURE_DEPTH * n + i]};
    g1[i] = DnRec{A[0], A[1], A[2], cov};
    c0[i] = DnRec{il[0], il[1], il[2], vi};
}

// ---- one a-trous iteration at pixel (x, y) of the W x H image, taps `s` apart: in -> out ---------------------------------------------
// 0 <= x < W, 0 <= y < H.  32-bit indices, on the host too: every index is x * H + y of a pixel inside the image, < W * H <= 2^28 (the
// entries' check), and a tap's coordinate is at most 2 * s <= 32 outside it (s <= 16: at most five iterations).  A coordinate is inside
// when it passes ONE unsigned compare (a negative one is huge).  The B3 and box weights are selected by the loop counters: constants
// of the kernel's unrolled loops.
APT_HD void dn_iterate(const DnRec *g0, const DnRec *g1, const DnRec *in, DnRec *out, int32_t W, int32_t H, int32_t s, const DnSigma &sg,
                       int32_t x, int32_t y) {
    const int32_t ip = x * H + y;

    float sv = 0.0f, sw = 0.0f;
    APT_UNROLL
    for (int32_t ex = -1; ex <= 1; ++ex)
        APT_UNROLL
        for (int32_t ey = -1; ey <= 1; ++ey) {
            const int32_t qx = x + ex, qy = y + ey;
            if ((uint32_t)qx < (uint32_t)W && (uint32_t)qy < (uint32_t)H) {
                const float b = (ex == 0 ? 2.0f : 1.0f) * (ey == 0 ? 2.0f : 1.0f);
                sv = sv + b * in[qx * H + qy].w;
                sw = sw + b;
            }
        }
    const float gv = sv / sw;
    float e = sqrtf(gv) * sg.l;
    e = e + 1e-6f;
    const float isd = 1.0f / e;
    const DnRec n_p = g0[ip], a_p = g1[ip], c_p = in[ip];
    const FsGuide gp = {n_p.x, n_p.y, n_p.z, n_p.w, a_p.w, a_p.x, a_p.y, a_p.z};
    const float zz = n_p.w + 1e-6f;
    const float iz = 1.0f / zz;
    const float lp = fs_lum(c_p.x, c_p.y, c_p.z);

    float Wt = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, V = 0.0f;
    APT_UNROLL
    for (int32_t dx = -2; dx <= 2; ++dx)
        APT_UNROLL
        for (int32_t dy = -2; dy <= 2; ++dy) {
            const int32_t qx = x + dx * s, qy = y + dy * s;                   // s <= 16: no overflow
            if ((uint32_t)qx < (uint32_t)W && (uint32_t)qy < (uint32_t)H) {
                const int32_t iq = qx * H + qy;
                const DnRec n_q = g0[iq], a_q = g1[iq], c_q = in[iq];
                const FsGuide gq = {n_q.x, n_q.y, n_q.z, n_q.w, a_q.w, a_q.x, a_q.y, a_q.z};
                const FsSigma gs = {sg.n, sg.z, sg.c, sg.a};   // read at the tap, as before: it keeps the kernel's instructions
                float xs = fs_edge_sum(gp, iz, gq, gs);
                const float lq = fs_lum(c_q.x, c_q.y, c_q.z);
                const float xl = fabsf(lp - lq) * isd;
                xs = xs + xl;
                const float t = fs_edge_falloff(xs);                          // of every tap, selected below: as before
                const float g = dx == 0 && dy == 0 ? 1.0f : t;                // the centre tap: x = 0 by definition (compile time)
                const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
                const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
                const float w = (hx * hy) * g;
                Wt = Wt + w;
                Sr = Sr + w * c_q.x;
                Sg = Sg + w * c_q.y;
                Sb = Sb + w * c_q.z;
                V = V + (w * w) * c_q.w;
            }
        }
    out[ip] = DnRec{Sr / Wt, Sg / Wt, Sb / Wt, V / (Wt * Wt)};
}

// ---- finish: pixel i's filtered illumination times its albedo ------------------------------------------------------------------------
APT_HD void dn_finish(const DnRec *g1, const DnRec *c, float *out, uint64_t n, uint32_t i) {
    const DnRec ci = c[i], gi = g1[i];
    out[i] = ci.x * gi.x;
    out[n + i] = ci.y * gi.y;
    out[2 * n + i] = ci.z * gi.z;
}

} // namespace apt
