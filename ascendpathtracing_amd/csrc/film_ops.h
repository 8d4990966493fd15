// film_ops.h -- the arithmetic of the film's resolve (include/render_mi355x.h "film"), once: film.hip's kernel runs it for its lane's
// pixel, host_helpers.cpp's apt_film_resolve_host in its loop.  The header's operations one fp32 operation per line
// (-ffp-contract=off on both sides); nothing of HIP is needed to compile it.
#pragma once
#include <stdint.h>

#include "apt_hd.h"

namespace apt {

// What turns a value of the film into y: apt_film_resolve's passes (as a float), exposure and 1 / white^2, and whether the tone operator
// is Reinhard's (launch-uniform).
struct FilmTone {
    float fpasses, exposure, inv_white2;
    uint32_t reinhard;
};

// One value of the film -> y in [0, 1]: the mean over the passes, the exposure, the tone operator, the clip.
APT_HD float film_tone(float s, const FilmTone &a) {
    const float m = s / a.fpasses;
    float x = m * a.exposure;
    x = x > 0.0f ? x : 0.0f;
    float y = x;
    if (a.reinhard) {
        float t = x * a.inv_white2;
        t = 1.0f + t;
        const float num = x * t;
        const float den = 1.0f + x;
        y = x == __builtin_inff() ? 1.0f : num / den;
    }
    return y < 1.0f ? y : 1.0f;
}

// y -> its 8-bit code: the last of the curve table's 256 ascending thresholds that is <= y, found in 8 steps.
APT_HD uint32_t film_code(const float *table, float y) {
    uint32_t code = 0;
    APT_UNROLL
    for (uint32_t b = 128; b; b >>= 1) code += table[code + b] <= y ? b : 0u;
    return code;
}

} // namespace apt
