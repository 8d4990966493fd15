// post_ops.h -- the arithmetic of libpost_mi355x.so (include/render_mi355x_post.h), each step once and per pixel: the header's
// operations one fp32 operation per line (-ffp-contract=off on both sides).  post.hip's kernels are a lane mapping and a call,
// post_host.cpp's CPU twins a loop and the same call: that is why they give the same bits.  Nothing of HIP is needed to compile it.
//
// The bloom's work buffer holds the pyramid levels one after the other, level j as wd_j * hd_j 16-byte records (r, g, b, 0), pixel
// (x, y) at x * hd_j + y as in every plane.  U_j is written over D_j: a pixel of U_j reads D_j at itself alone.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/render_mi355x_post.h"
#include "apt_hd.h"
#include "film_stage_ops.h"

namespace apt {

using PoRec = FsRec;                              // one record of a pyramid level
APT_HD uint32_t po_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

// ---- metering: the histogram word of a pixel whose film values are (r, g, b); K = passes -------------------------------------------------
APT_HD uint32_t po_meter_bin(float r, float g, float b, float K) {
    const float cr = r / K, cg = g / K, cb = b / K;
    const float l = fs_lum(cr, cg, cb);
    if (!(l > 0.0f)) return APT_METER_BINS;                       // zero, negative, NaN: word 256
    const int32_t e = (int32_t)(po_bits(l) >> 20) - 888;          // l > 0: the sign bit is clear, bits >> 20 <= 0x7F8
    return (uint32_t)(e < 0 ? 0 : (e > 255 ? 255 : e));
}

// ---- bloom -------------------------------------------------------------------------------------------------------------------------------
// 32-bit indices, on the host too: every index is x * h + y of a pixel inside an image of at most 2^28 pixels (the entries' check), and
// a tap's coordinate is at most 2 * x + 2 <= 2^29 + 2.  A coordinate is inside when it passes ONE unsigned compare (a negative one is huge).
struct PoBright { float K, cap, threshold; };

// the bright-pass of film pixel i of n -> v
APT_HD void po_bright(const float *film, uint32_t n, uint32_t i, const PoBright &p, float v[3]) {
    float x[3];
    APT_UNROLL
    for (uint32_t ch = 0; ch < 3; ++ch) {
        const float m = film[(size_t)ch * n + i] / p.K;
        float t = m > 0.0f ? m : 0.0f;
        t = t < p.cap ? t : p.cap;
        x[ch] = t;
    }
    const float l = fs_lum(x[0], x[1], x[2]);
    const float g = fs_max(l - p.threshold, 0.0f) / fs_max(l, 1e-6f);
    APT_UNROLL
    for (uint32_t ch = 0; ch < 3; ++ch) v[ch] = x[ch] * g;
}

// the two sources of a down step: the bright image of the film, or the level before
struct PoFilmSrc {
    const float *film;
    uint32_t n;
    PoBright p;
    APT_HD void get(uint32_t i, float v[3]) const { po_bright(film, n, i, p, v); }
};
struct PoRecSrc {
    const PoRec *rec;
    APT_HD void get(uint32_t i, float v[3]) const {
        const PoRec r = rec[i];
        v[0] = r.x; v[1] = r.y; v[2] = r.z;
    }
};

// down: pixel (x, y) of the destination from the ws x hs source
template <class Src>
APT_HD PoRec po_down(const Src &src, int32_t ws, int32_t hs, int32_t x, int32_t y) {
    float W = 0.0f, S0 = 0.0f, S1 = 0.0f, S2 = 0.0f;
    APT_UNROLL
    for (int32_t dx = -1; dx <= 2; ++dx)
        APT_UNROLL
        for (int32_t dy = -1; dy <= 2; ++dy) {
            const int32_t qx = 2 * x + dx, qy = 2 * y + dy;
            if ((uint32_t)qx < (uint32_t)ws && (uint32_t)qy < (uint32_t)hs) {
                const float w = ((dx == 0 || dx == 1) ? 3.0f : 1.0f) * ((dy == 0 || dy == 1) ? 3.0f : 1.0f);
                float v[3];
                src.get((uint32_t)(qx * hs + qy), v);
                W = W + w;
                S0 = S0 + w * v[0];
                S1 = S1 + w * v[1];
                S2 = S2 + w * v[2];
            }
        }
    return PoRec{S0 / W, S1 / W, S2 / W, 0.0f};                   // (the tap (2x, 2y) is always inside: W >= 1)
}

// up: the wc x hc level `c` at the fine pixel (x, y) -> u
APT_HD void po_up(const PoRec *c, int32_t wc, int32_t hc, int32_t x, int32_t y, float u[3]) {
    const int32_t x0 = (x - 1) >> 1, y0 = (y - 1) >> 1;           // arithmetic shifts: -1 for a fine index 0
    const float wx0 = (x & 1) ? 0.75f : 0.25f, wy0 = (y & 1) ? 0.75f : 0.25f;
    u[0] = 0.0f; u[1] = 0.0f; u[2] = 0.0f;
    APT_UNROLL
    for (int32_t tx = 0; tx < 2; ++tx)
        APT_UNROLL
        for (int32_t ty = 0; ty < 2; ++ty) {
            int32_t qx = x0 + tx, qy = y0 + ty;
            qx = qx < 0 ? 0 : (qx > wc - 1 ? wc - 1 : qx);
            qy = qy < 0 ? 0 : (qy > hc - 1 ? hc - 1 : qy);
            const float w = (tx ? 1.0f - wx0 : wx0) * (ty ? 1.0f - wy0 : wy0);      // (1 - 0.25, 1 - 0.75 and the products are exact)
            const PoRec r = c[qx * hc + qy];
            u[0] = u[0] + w * r.x;
            u[1] = u[1] + w * r.y;
            u[2] = u[2] + w * r.z;
        }
}

// combine: U_j over D_j at pixel (x, y) of the wf x hf level `d`, from the wc x hc level `c` = U_(j+1)
APT_HD void po_combine(PoRec *d, const PoRec *c, int32_t hf, int32_t wc, int32_t hc, float spread, int32_t x, int32_t y) {
    float u[3];
    po_up(c, wc, hc, x, y, u);
    const int32_t i = x * hf + y;
    const PoRec r = d[i];
    d[i] = PoRec{r.x + spread * u[0], r.y + spread * u[1], r.z + spread * u[2], 0.0f};
}

// composite: out at pixel (x, y) of the W x H image from the film and U_0 (wc x hc)
APT_HD void po_composite(const float *film, const PoRec *c, float *out, int32_t W, int32_t H, int32_t wc, int32_t hc, float K, float intensity,
                         int32_t x, int32_t y) {
    float u[3];
    po_up(c, wc, hc, x, y, u);
    const uint32_t n = (uint32_t)(W * H), i = (uint32_t)(x * H + y);
    APT_UNROLL
    for (uint32_t ch = 0; ch < 3; ++ch) {
        const float m = film[(size_t)ch * n + i] / K;
        out[(size_t)ch * n + i] = m + intensity * u[ch];
    }
}

// ---- what the launches and the twins' loops are made from ----------------------------------------------------------------------------------
constexpr uint32_t kPoMaxLevels = 6;
constexpr uint32_t kPoMeterMaxRows = 512;
// the rows of the meter's work buffer = its workgroups: one per 1024 pixels, at most 512
inline uint32_t po_meter_rows(uint64_t pixel_count) {
    const uint64_t r = (pixel_count + 1023) / 1024;
    return (uint32_t)(r < kPoMeterMaxRows ? r : kPoMeterMaxRows);
}

// a checked bloom call: the record's values as the arithmetic reads them, the sizes of the levels and where they start in work
struct PoBloom {
    const float *film;
    float *out;
    PoRec *level[kPoMaxLevels];
    int32_t w[kPoMaxLevels], h[kPoMaxLevels];
    int32_t W, H;
    uint32_t levels;
    PoBright bright;
    float spread, intensity;
};

} // namespace apt
