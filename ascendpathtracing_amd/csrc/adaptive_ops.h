// adaptive_ops.h -- the arithmetic of libadaptive_mi355x.so (include/render_mi355x_adaptive.h), each step once and per pixel: the
// header's operations one fp32 operation per line (-ffp-contract=off on both sides).  adaptive.hip's kernels are a lane mapping and a
// call, adaptive_host.cpp's CPU twins a loop and the same call: that is why they give the same bits.  Nothing of HIP is needed to
// compile it.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/render_mi355x_adaptive.h"
#include "apt_hd.h"
#include "film_stage_ops.h"

namespace apt {

constexpr uint32_t kAdBlock = 256;   // pixels per workgroup of the select: one word of its work buffer each

struct AdSelect { uint32_t base, min_passes, max_passes; float threshold, floor_; };   // apt_film_select, checked

// ---- select: does the pixel with these moments and this many extra passes get another one? --------------------------------------------
APT_HD bool ad_selected(float m0, float m1, uint32_t extra, const AdSelect &s) {
    const uint64_t nu = (uint64_t)s.base + extra;
    if (nu >= s.max_passes) return false;
    if (nu < s.min_passes) return true;
    const float n = (float)(uint32_t)nu;            // < 2^24: exact
    const float lm = m0 / n;
    const float sq = m1 / n;
    const float d = fs_max(sq - lm * lm, 0.0f);
    const float v = d / (float)((uint32_t)nu - 1u);
    const float e = sqrtf(v);
    const float r = fs_max(lm, s.floor_);
    const float t = s.threshold * r;
    return e > t;
}

// ---- accumulate: entry i of the list's `count` joins pixel list[i] of n; an entry beyond the image is skipped ---------------------------
APT_HD void ad_accumulate(const float *pass, const uint32_t *list, uint64_t count, float *film, float *mom, uint32_t *extra, uint64_t n,
                          uint64_t i) {
    const uint64_t p = list[i];
    if (p >= n) return;
    const float r = pass[i], g = pass[count + i], b = pass[2 * count + i];
    const float l = fs_lum(r, g, b);
    const float l2 = l * l;
    film[p] = film[p] + r; film[n + p] = film[n + p] + g; film[2 * n + p] = film[2 * n + p] + b;
    mom[p] = mom[p] + l; mom[n + p] = mom[n + p] + l2;
    extra[p] = extra[p] + 1u;
}

// ---- mean: pixel i's sums over its own number of passes; extra null: no pixel has any ----------------------------------------------
APT_HD void ad_mean(const float *film, const uint32_t *extra, uint32_t base, float *out, uint64_t n, uint64_t i) {
    const float k = (float)((uint64_t)base + (extra ? extra[i] : 0u));
    out[i] = film[i] / k;
    out[n + i] = film[n + i] / k;
    out[2 * n + i] = film[2 * n + i] / k;
}

} // namespace apt
