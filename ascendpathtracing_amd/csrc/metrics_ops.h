// metrics_ops.h -- the arithmetic of libmetrics_mi355x.so (include/render_mi355x_metrics.h), each step once: the header's operations
// one fp32 operation per line (-ffp-contract=off on both sides).  metrics.hip's kernels are a lane mapping and a call,
// metrics_host.cpp's CPU twins a loop and the same call: that is why they give the same bits.  Nothing of HIP is needed to compile it.
//
// The sums.  A kernel reduces an aligned chunk of kMxChunk terms per workgroup (four consecutive terms a lane, the wave's xor
// butterfly, the waves in pairs) and a fold launch kMxFoldRows rows per workgroup; the twins push term after term onto MxTree, a binary
// counter of partial sums.  Both are the header's tree: T(i, l + 1) = T(2 i, l) + T(2 i + 1, l), padded with +0.0.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/render_mi355x_metrics.h"
#include "apt_hd.h"
#include "film_stage_ops.h"

namespace apt {

APT_HD uint32_t mx_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}
APT_HD float mx_abs(float f) {                                       // the sign bit cleared: exact, and a NaN never comes here
    const uint32_t u = mx_bits(f) & 0x7FFFFFFFu;
    float r;
    memcpy(&r, &u, sizeof r);
    return r;
}
APT_HD float mx_clip01(float e) {
    const float t = e > 0.0f ? e : 0.0f;
    return t < 1.0f ? t : 1.0f;
}
// |v| >= 2^60, an infinity or a NaN: the biased exponent field is 187 or more
APT_HD bool mx_is_bad(float v) { return ((mx_bits(v) >> 23) & 255u) >= 187u; }

// ---- compare: what ONE pixel gives ---------------------------------------------------------------------------------------------------------
// the checked record as the arithmetic reads it.  inv_a, inv_b: 1 / K where K is a power of two, else 0 (mx_mean)
struct MxRec { float Ka, Kb, exposure, eps, inv_a, inv_b; };
inline MxRec mx_rec(uint32_t passes_a, uint32_t passes_b, float exposure, float eps) {
    MxRec r;
    r.Ka = (float)passes_a; r.Kb = (float)passes_b; r.exposure = exposure; r.eps = eps;
    r.inv_a = (passes_a & (passes_a - 1)) == 0 ? 1.0f / r.Ka : 0.0f;      // passes <= 2^24: K and 1 / K are exact
    r.inv_b = (passes_b & (passes_b - 1)) == 0 ? 1.0f / r.Kb : 0.0f;
    return r;
}
// v / K.  For K = 2^m the product v * 2^-m is the same float: both are the exact quotient rounded once (subnormal results, infinities
// and NaNs included), and it spares the kernels six of their nine divisions a pixel in the common cases (means: K = 1).
APT_HD float mx_mean(float v, float K, float inv) { return inv != 0.0f ? v * inv : v / K; }
struct MxTerms {
    float se, cse, rse, ae;                                          // +0 for a bad pixel
    uint64_t key;                                                    // 0 for a bad pixel
    uint32_t bad;                                                    // 1 for a bad pixel
};

APT_HD MxTerms mx_pixel(const float a[3], const float b[3], uint32_t i, const MxRec &p) {
    float x[3], y[3];
    bool bad = false;
    APT_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
        x[ch] = mx_mean(a[ch], p.Ka, p.inv_a);
        y[ch] = mx_mean(b[ch], p.Kb, p.inv_b);
        bad = bad || mx_is_bad(x[ch]) || mx_is_bad(y[ch]);
    }
    MxTerms t;
    if (bad) {
        t.se = 0.0f; t.cse = 0.0f; t.rse = 0.0f; t.ae = 0.0f; t.key = 0; t.bad = 1;
        return t;
    }
    float dd[3], ad[3], r[3], cc[3];
    APT_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
        const float d = x[ch] - y[ch];
        dd[ch] = d * d;
        ad[ch] = mx_abs(d);
        const float yy = y[ch] * y[ch];
        r[ch] = dd[ch] / (yy + p.eps);
        const float cx = mx_clip01(x[ch] * p.exposure), cy = mx_clip01(y[ch] * p.exposure);
        const float c = cx - cy;
        cc[ch] = c * c;
    }
    t.se = (dd[0] + dd[1]) + dd[2];
    t.cse = (cc[0] + cc[1]) + cc[2];
    t.rse = (r[0] + r[1]) + r[2];
    t.ae = (ad[0] + ad[1]) + ad[2];
    const float m = fs_max(fs_max(ad[0], ad[1]), ad[2]);
    t.key = ((uint64_t)mx_bits(m) << 32) | (uint64_t)(0xFFFFFFFFu - i);
    t.bad = 0;
    return t;
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------------------
// the 11 weights: exp(-(k - 5)^2 / 4.5) normalised in float64, rounded once (tests/metrics_ref.py computes them; a test holds these to it)
APT_HD float mx_weight(int k) {
    switch (k < 5 ? k : 10 - k) {
    case 0: return 0x1.0d956cp-10f;
    case 1: return 0x1.f1fe02p-8f;
    case 2: return 0x1.26eb18p-5f;
    case 3: return 0x1.bff0fep-4f;
    case 4: return 0x1.b43c4p-3f;
    default: return 0x1.10656p-2f;
    }
}
constexpr float kMxC1 = 1e-4f, kMxC2 = 9e-4f;

// the display luminance of a film's pixel (r, g, b) over K frames
APT_HD float mx_display_lum(float r, float g, float b, float K, float inv, float exposure) {
    const float mr = mx_mean(r, K, inv), mg = mx_mean(g, K, inv), mb = mx_mean(b, K, inv);
    return fs_lum(mx_clip01(mr * exposure), mx_clip01(mg * exposure), mx_clip01(mb * exposure));
}

// one step of a pass of the filter over the five planes, from the luminances (ya, yb) of ONE source pixel (the x pass) ...
APT_HD void mx_tap_source(float acc[5], float w, float ya, float yb) {
    const float aa = ya * ya, bb = yb * yb, ab = ya * yb;
    acc[0] = acc[0] + w * ya;
    acc[1] = acc[1] + w * yb;
    acc[2] = acc[2] + w * aa;
    acc[3] = acc[3] + w * bb;
    acc[4] = acc[4] + w * ab;
}
// ... and from the x pass's five results at one pixel (the y pass)
APT_HD void mx_tap_planes(float acc[5], float w, const float h[5]) {
    APT_UNROLL
    for (int p = 0; p < 5; ++p) acc[p] = acc[p] + w * h[p];
}
// a window's s from its five filtered planes (ma, mb, Eaa, Ebb, Eab)
APT_HD float mx_ssim(const float f[5]) {
    const float maa = f[0] * f[0], mbb = f[1] * f[1], mab = f[0] * f[1];
    const float saa = f[2] - maa, sbb = f[3] - mbb, sab = f[4] - mab;
    const float n0 = 2.0f * mab + kMxC1, n1 = 2.0f * sab + kMxC2;
    const float d0 = (maa + mbb) + kMxC1, d1 = (saa + sbb) + kMxC2;
    return (n0 * n1) / (d0 * d1);
}

// ---- what the launches and the twins' loops are made from ----------------------------------------------------------------------------------
constexpr uint32_t kMxChunk = 1024;                                  // terms a workgroup of a reducing kernel takes: 256 lanes x 4
constexpr uint32_t kMxFoldRows = 4096;                               // rows a workgroup of the fold takes: 1024 lanes x 4
constexpr uint32_t kMxCompareRowWords = 6;                           // se, cse, rse, ae, key, bad

// the rows of a reduction of n terms, level by level: r0 workgroup rows, then r1 rows of a first fold when r0 > kMxFoldRows (the last
// fold always stores the result itself); n <= 2^28: r1 <= 64
struct MxRows { uint32_t r0, r1; };
inline MxRows mx_rows(uint64_t n) {
    MxRows r;
    r.r0 = (uint32_t)((n + kMxChunk - 1) / kMxChunk);
    r.r1 = r.r0 > kMxFoldRows ? (r.r0 + kMxFoldRows - 1) / kMxFoldRows : 0u;
    return r;
}

// the header's tree over terms pushed in order, kS sums at once: level l holds the sum of a finished block of 2^l terms
template <int kS>
struct MxTree {
    double level[29][kS];                                            // n <= 2^28
    uint64_t count = 0;
    void push(const float t[kS]) {
        double v[kS];
        for (int s = 0; s < kS; ++s) v[s] = (double)t[s];
        int l = 0;
        for (uint64_t c = count; c & 1; c >>= 1, ++l)
            for (int s = 0; s < kS; ++s) v[s] = level[l][s] + v[s];
        for (int s = 0; s < kS; ++s) level[l][s] = v[s];
        ++count;
    }
    // -> T(0, L), count >= 1.  v is the node of level l that holds the last terms and the padding after them; the finished block of
    // level l (bit l of count) is its left sibling; without one v is itself a left child and its sibling is padding: + 0.0.
    void finish(double out[kS]) const {
        bool have = false;
        double v[kS];
        for (int s = 0; s < kS; ++s) v[s] = 0.0;
        for (int l = 0; l < 29; ++l) {
            const uint64_t rest = count >> l;
            if (rest == 0) break;
            if (rest == 1 && !have) {                                // count is 2^l: the block is the tree
                for (int s = 0; s < kS; ++s) v[s] = level[l][s];
                break;
            }
            if (rest & 1) {
                for (int s = 0; s < kS; ++s) v[s] = have ? level[l][s] + v[s] : level[l][s] + 0.0;
                have = true;
            } else if (have) {
                for (int s = 0; s < kS; ++s) v[s] = v[s] + 0.0;
            }
            if ((rest >> 1) == 0) break;
        }
        for (int s = 0; s < kS; ++s) out[s] = v[s];
    }
};

} // namespace apt
