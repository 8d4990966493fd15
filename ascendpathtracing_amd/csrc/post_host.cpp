// post_host.cpp -- the host side of libpost_mi355x.so (include/render_mi355x_post.h): the checks that the device and the host form of each entry share, the defaults, the exposure (host only) and the CPU twins.  Compiled
// with the product's -ffp-contract=off -fno-fast-math: a twin is a loop over the pixels and the call of post_ops.h that post.hip's
// kernel makes for its lane, so both give the same bits.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/render_mi355x_post.h"
#include "post_host.h"
#include "post_ops.h"

namespace {
bool positive(float v) { return std::isfinite(v) && v > 0.0f; }
bool not_negative(float v) { return std::isfinite(v) && v >= 0.0f; }
}

using apt::kMaxPixels;

namespace apt {
// the whole record, whichever entry takes it
static int meter_record_check(const apt_film_meter *m, const char *what) {
    if (m->struct_size != sizeof(apt_film_meter)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_film_meter.struct_size mismatch", what);
    if (int rc = stage_passes_check(m->passes, "passes", what)) return rc;
    if (!(1 <= m->low_q && m->low_q <= m->high_q && m->high_q <= 65536))
        return stage_set_error(APT_ERR_ARG, "%s: the percentiles must satisfy 1 <= low_q <= high_q <= 65536", what);
    if (!positive(m->key) || !positive(m->min_exposure) || !positive(m->max_exposure))
        return stage_set_error(APT_ERR_ARG, "%s: key, min_exposure and max_exposure must be finite and positive", what);
    if (m->min_exposure > m->max_exposure) return stage_set_error(APT_ERR_ARG, "%s: min_exposure must not exceed max_exposure", what);
    if (!(m->adapt >= 0.0f && m->adapt <= 1.0f)) return stage_set_error(APT_ERR_ARG, "%s: adapt must lie in [0, 1]", what);
    return APT_OK;
}

int film_meter_check(const apt_film_meter *m, const void *film, uint64_t pixel_count, const void *work, bool need_work, const void *hist,
                     const char *what) {
    if (!m || !hist) return stage_set_error(APT_ERR_ARG, "%s: m/hist must be non-null", what);
    if (pixel_count != 0 && (!film || (need_work && !work))) return stage_set_error(APT_ERR_ARG, "%s: film/work must be non-null", what);
    if (int rc = meter_record_check(m, what)) return rc;
    if (pixel_count > kMaxPixels) return stage_set_error(APT_ERR_ARG, "%s: pixel_count must not exceed 2^28", what);
    return APT_OK;
}

int film_bloom_check(const apt_film_bloom *b, const float *film, uint32_t width, uint32_t height, float *work, float *out, PoBloom *args,
                     const char *what) {
    if (!b || !film || !work || !out) return stage_set_error(APT_ERR_ARG, "%s: b/film/work/out must be non-null", what);
    if (b->struct_size != sizeof(apt_film_bloom)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_film_bloom.struct_size mismatch", what);
    if (int rc = stage_pixels_check((uint64_t)width * height, "width * height", what)) return rc;
    if ((uintptr_t)work % 16 != 0) return stage_set_error(APT_ERR_ARG, "%s: work must be 16-byte aligned", what);
    if (out == film) return stage_set_error(APT_ERR_ARG, "%s: out must not be film", what);
    if (int rc = stage_passes_check(b->passes, "passes", what)) return rc;
    if (b->levels < 1 || b->levels > kPoMaxLevels) return stage_set_error(APT_ERR_ARG, "%s: levels must lie in [1, 6]", what);
    if (!not_negative(b->threshold) || !not_negative(b->spread) || !not_negative(b->intensity))
        return stage_set_error(APT_ERR_ARG, "%s: threshold, spread and intensity must be finite and not negative", what);
    if (!positive(b->cap)) return stage_set_error(APT_ERR_ARG, "%s: cap must be finite and positive", what);
    args->film = film; args->out = out; args->W = (int32_t)width; args->H = (int32_t)height; args->levels = b->levels;
    args->bright = PoBright{(float)b->passes, b->cap, b->threshold};
    args->spread = b->spread; args->intensity = b->intensity;
    PoRec *at = reinterpret_cast<PoRec *>(work);
    int32_t w = (int32_t)width, h = (int32_t)height;
    for (uint32_t j = 0; j < kPoMaxLevels; ++j) {
        w = (w + 1) >> 1; h = (h + 1) >> 1;
        args->w[j] = w; args->h[j] = h; args->level[j] = at;
        if (j < b->levels) at += (size_t)w * h;
    }
    return APT_OK;
}
} // namespace apt
using apt::stage_set_error;

extern "C" {

const char *apt_film_post_last_error(void) { return apt::stage_last_error(); }

int apt_film_meter_default_host(apt_film_meter *m, uint32_t passes) {
    apt::stage_clear_error();
    if (!m) return stage_set_error(APT_ERR_ARG, "%s: the record is null", "apt_film_meter_default_host");
    if (int rc = apt::stage_passes_check(passes, "passes", "apt_film_meter_default_host")) return rc;
    memset(m, 0, sizeof *m);
    m->struct_size = sizeof *m;
    m->passes = passes;
    m->low_q = 6554; m->high_q = 58982;                           // 10 % .. 90 % of 65536
    m->key = 0.18f;
    m->min_exposure = 0.000244140625f; m->max_exposure = 4096.0f; // 2^-12, 2^12
    m->adapt = 1.0f;
    return APT_OK;
}

uint64_t apt_film_meter_work_words(uint64_t pixel_count) {
    if (pixel_count > kMaxPixels) return 0;
    return (uint64_t)apt::po_meter_rows(pixel_count) * APT_METER_WORDS;
}

int apt_film_meter_host(const apt_film_meter *m, const float *film, uint64_t pixel_count, uint32_t *hist) {
    apt::stage_clear_error();
    const int rc = apt::film_meter_check(m, film, pixel_count, nullptr, false, hist, "apt_film_meter_host");
    if (rc) return rc;
    memset(hist, 0, APT_METER_WORDS * sizeof(uint32_t));
    const float K = (float)m->passes;
    for (uint64_t i = 0; i < pixel_count; ++i) hist[apt::po_meter_bin(film[i], film[pixel_count + i], film[2 * pixel_count + i], K)] += 1;
    return APT_OK;
}

int apt_film_exposure_host(const apt_film_meter *m, const uint32_t *hist, float prev, float *exposure) {
    apt::stage_clear_error();
    const char *what = "apt_film_exposure_host";
    if (!m || !hist || !exposure) return stage_set_error(APT_ERR_ARG, "%s: m/hist/exposure must be non-null", what);
    if (int rc = apt::meter_record_check(m, what)) return rc;
    if (!(std::isfinite(prev) && prev >= 0.0f)) return stage_set_error(APT_ERR_ARG, "%s: prev must be finite and not negative", what);
    uint64_t n = 0;
    for (int b = 0; b < APT_METER_BINS; ++b) n += hist[b];
    if (n == 0) { *exposure = prev; return APT_OK; }
    // the percentile bins: n <= 256 * (2^32 - 1) < 2^40, so cum * 65536 and q * n stay below 2^57
    int b_lo = -1, b_hi = -1;
    uint64_t cum = 0;
    for (int b = 0; b < APT_METER_BINS; ++b) {
        cum += hist[b];
        if (b_lo < 0 && cum * 65536 >= (uint64_t)m->low_q * n) b_lo = b;
        if (b_hi < 0 && cum * 65536 >= (uint64_t)m->high_q * n) b_hi = b;
    }
    uint64_t C = 0, S = 0;                                        // hist[b_lo] > 0: cum first reaches a positive bound there
    for (int b = b_lo; b <= b_hi; ++b) { C += hist[b]; S += (uint64_t)hist[b] * (uint64_t)(2 * b + 1); }
    const uint32_t m2 = (uint32_t)(S / C);                        // 1 .. 511
    const uint32_t lbits = (888u << 20) + (m2 << 19);
    float L;
    memcpy(&L, &lbits, sizeof L);
    float t = m->key / L;
    t = t < m->max_exposure ? t : m->max_exposure;
    t = t > m->min_exposure ? t : m->min_exposure;
    if (m->adapt >= 1.0f) { *exposure = t; return APT_OK; }
    const float d = t - prev;
    *exposure = prev + d * m->adapt;
    return APT_OK;
}

int apt_film_bloom_default_host(apt_film_bloom *b, uint32_t passes) {
    apt::stage_clear_error();
    if (!b) return stage_set_error(APT_ERR_ARG, "%s: the record is null", "apt_film_bloom_default_host");
    if (int rc = apt::stage_passes_check(passes, "passes", "apt_film_bloom_default_host")) return rc;
    memset(b, 0, sizeof *b);
    b->struct_size = sizeof *b;
    b->passes = passes;
    b->levels = 5;
    b->threshold = 1.0f; b->cap = 65536.0f; b->spread = 1.0f; b->intensity = 0.05f;   // DESIGN.md "Post": not tuned
    return APT_OK;
}

uint64_t apt_film_bloom_work_floats(uint32_t width, uint32_t height, uint32_t levels) {
    if (width == 0 || height == 0 || (uint64_t)width * height > kMaxPixels || levels < 1 || levels > apt::kPoMaxLevels) return 0;
    uint64_t records = 0, w = width, h = height;
    for (uint32_t j = 0; j < levels; ++j) {
        w = (w + 1) >> 1; h = (h + 1) >> 1;
        records += w * h;
    }
    return 4 * records;
}

int apt_film_bloom_host(const apt_film_bloom *b, const float *film, uint32_t width, uint32_t height, float *work, float *out) {
    apt::stage_clear_error();
    apt::PoBloom a;
    const int rc = apt::film_bloom_check(b, film, width, height, work, out, &a, "apt_film_bloom_host");
    if (rc) return rc;
    const uint32_t n = width * height;
    for (uint32_t j = 0; j < a.levels; ++j)
        for (int32_t x = 0; x < a.w[j]; ++x)
            for (int32_t y = 0; y < a.h[j]; ++y)
                a.level[j][x * a.h[j] + y] = j == 0 ? apt::po_down(apt::PoFilmSrc{film, n, a.bright}, a.W, a.H, x, y)
                                                    : apt::po_down(apt::PoRecSrc{a.level[j - 1]}, a.w[j - 1], a.h[j - 1], x, y);
    for (int32_t j = (int32_t)a.levels - 2; j >= 0; --j)
        for (int32_t x = 0; x < a.w[j]; ++x)
            for (int32_t y = 0; y < a.h[j]; ++y) apt::po_combine(a.level[j], a.level[j + 1], a.h[j], a.w[j + 1], a.h[j + 1], a.spread, x, y);
    for (int32_t x = 0; x < a.W; ++x)
        for (int32_t y = 0; y < a.H; ++y) apt::po_composite(film, a.level[0], out, a.W, a.H, a.w[0], a.h[0], a.bright.K, a.intensity, x, y);
    return APT_OK;
}

} // extern "C"
