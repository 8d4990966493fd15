// history_ops.h -- the arithmetic of libhistory_mi355x.so (include/render_mi355x_history.h), each step once and per pixel: the header's
// geometry one float64 operation per line, its blend and its export one fp32 operation per line (-ffp-contract=off on both sides).
// history.hip's kernels are a lane mapping and a call, history_host.cpp's CPU twins a loop and the same call: that is why they give
// the same bits.  Nothing of HIP is needed to compile it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/render_mi355x_history.h"
#include "apt_hd.h"
#include "film_stage_ops.h"

namespace apt {

constexpr uint32_t kHsBlock = 256;   // lanes per workgroup of both kernels

// What the geometry reads of an apt_camera, checked, with the three squared lengths the projection divides by.
struct HsCam {
    double pos[3], g[3], cx[3], cy[3], offset;
    double gg, xx, yy;               // dot(g, g), dot(cx, cx), dot(cy, cy)
};

struct HsArgs {
    const float *cur, *cf, *pf, *ph; // ph null: the first frame
    float *out;
    uint32_t w, h;
    float min_weight, max_history;   // (float)max_history: exact, <= 2^24
    double tol_plane, tol_normal;    // widened exactly
    HsCam cc, pc;
};

APT_HD double hs_dot(const double *p, const double *q) { return (p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]; }

APT_HD HsCam hs_cam(const apt_camera &c) {
    HsCam k;
    for (int i = 0; i < 3; ++i) { k.pos[i] = c.pos[i]; k.g[i] = c.g[i]; k.cx[i] = c.cx[i]; k.cy[i] = c.cy[i]; }
    k.offset = c.offset;
    k.gg = hs_dot(k.g, k.g); k.xx = hs_dot(k.cx, k.cx); k.yy = hs_dot(k.cy, k.cy);
    return k;
}

// The world point X of pixel (x, y) of camera c, whose planes hold `cov` and `depth` there (w, h: the image's size as doubles).
APT_HD void hs_world(const HsCam &c, double w, double h, double x, double y, double cov, double depth, double *X) {
    const double a = (x + 0.5) / w - 0.5;
    const double b = (y + 0.5) / h - 0.5;
    double d[3];
    APT_UNROLL
    for (int k = 0; k < 3; ++k) d[k] = (c.cx[k] * a + c.cy[k] * b) + c.g[k];
    const double nd = sqrt(hs_dot(d, d));
    const double t = depth / cov;
    APT_UNROLL
    for (int k = 0; k < 3; ++k) {
        const double o = c.pos[k] + d[k] * c.offset;
        X[k] = o + (d[k] / nd) * t;
    }
}

// ---- reproject and blend: pixel (x, y) of the image, i = x * h + y -------------------------------------------------------------------
APT_HD void hs_pixel(const HsArgs &A, uint32_t x, uint32_t y) {
    const uint64_t n = (uint64_t)A.w * A.h;
    const uint64_t i = (uint64_t)x * A.h + y;
    const float cr = A.cur[i], cg = A.cur[n + i], cb = A.cur[2 * n + i];
    const float l = fs_lum(cr, cg, cb);
    const float nw[5] = {cr, cg, cb, l, l * l};
    float S[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float W = 0.0f, Sh = 0.0f;
    if (A.ph) {
        const double w = (double)A.w, h = (double)A.h;
        const double cov = (double)A.cf[APT_FEATURE_COVERAGE * n + i];
        double X[3], np_[3], vp[3], wv[3];
        hs_world(A.cc, w, h, (double)x, (double)y, cov, (double)A.cf[APT_FEATURE_DEPTH * n + i], X);
        APT_UNROLL
        for (int k = 0; k < 3; ++k) {
            np_[k] = (double)A.cf[(APT_FEATURE_NORMAL + k) * n + i] / cov;
            vp[k] = X[k] - A.cc.pos[k];
            wv[k] = X[k] - A.pc.pos[k];
        }
        const double r = sqrt(hs_dot(vp, vp));
        const double f = hs_dot(wv, A.pc.g) / A.pc.gg;
        const double ap = hs_dot(wv, A.pc.cx) / (f * A.pc.xx);
        const double bp = hs_dot(wv, A.pc.cy) / (f * A.pc.yy);
        const double u = (ap + 0.5) * w - 0.5;
        const double v = (bp + 0.5) * h - 0.5;
        const double x0 = floor(u), y0 = floor(v);
        const double fx = u - x0, fy = v - y0;
        const double bound = A.tol_plane * r;
        const bool front = f > 0.0 && cov > 0.0;
        APT_UNROLL
        for (int ex = 0; ex < 2; ++ex)
            APT_UNROLL
            for (int ey = 0; ey < 2; ++ey) {
                const double qx = x0 + (double)ex, qy = y0 + (double)ey;
                const float wq = (float)((ex ? fx : 1.0 - fx) * (ey ? fy : 1.0 - fy));
                if (!(front && qx >= 0.0 && qx <= w - 1.0 && qy >= 0.0 && qy <= h - 1.0)) continue;
                const uint64_t q = (uint64_t)(uint32_t)qx * A.h + (uint32_t)qy;      // inside the image: the compares above
                const double covq = (double)A.pf[APT_FEATURE_COVERAGE * n + q];
                const float hq = A.ph[5 * n + q];
                if (!(covq > 0.0 && hq >= 1.0f)) continue;
                double Xq[3], dx[3], nq[3];
                hs_world(A.pc, w, h, qx, qy, covq, (double)A.pf[APT_FEATURE_DEPTH * n + q], Xq);
                APT_UNROLL
                for (int k = 0; k < 3; ++k) {
                    dx[k] = Xq[k] - X[k];
                    nq[k] = (double)A.pf[(APT_FEATURE_NORMAL + k) * n + q] / covq;
                }
                if (!(fabs(hs_dot(dx, np_)) <= bound && hs_dot(np_, nq) >= A.tol_normal)) continue;
                W = W + wq;
                APT_UNROLL
                for (int j = 0; j < 5; ++j) S[j] = S[j] + wq * A.ph[j * n + q];
                Sh = Sh + wq * hq;
            }
    }
    if (W >= A.min_weight) {
        const float hl = Sh / W;
        const float t = hl + 1.0f;
        const float hn = t < A.max_history ? t : A.max_history;
        const float alpha = 1.0f / hn;
        APT_UNROLL
        for (int j = 0; j < 5; ++j) {
            const float H = S[j] / W;
            A.out[j * n + i] = H + alpha * (nw[j] - H);
        }
        A.out[5 * n + i] = hn;
    } else {
        APT_UNROLL
        for (int j = 0; j < 5; ++j) A.out[j * n + i] = nw[j];
        A.out[5 * n + i] = 1.0f;
    }
}

// ---- export: pixel i of n, for the denoiser with passes = 2 -----------------------------------------------------------------------------
APT_HD void hs_export(const float *hist, float *film, float *mom, uint64_t n, uint64_t i) {
    APT_UNROLL
    for (int c = 0; c < 3; ++c) {
        const float v = hist[c * n + i];
        film[c * n + i] = v + v;
    }
    const float lm = hist[3 * n + i], q = hist[4 * n + i], h = hist[5 * n + i];
    const float l2 = lm * lm;
    const float hm = h - 1.0f;
    float var = q;
    if (hm >= 1.0f) {
        const float d = q - l2;
        var = (d > 0.0f ? d : 0.0f) / hm;
    }
    const float qq = l2 + var;
    mom[i] = lm + lm;
    mom[n + i] = qq + qq;
}

} // namespace apt
