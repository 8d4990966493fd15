// adaptive_host.cpp -- the host side of libadaptive_mi355x.so (include/render_mi355x_adaptive.h): the checks that the device and the host form of each entry share, the defaults and the CPU twins.  Compiled with the
// product's -ffp-contract=off -fno-fast-math: a twin is a loop over the pixels and the call of adaptive_ops.h that adaptive.hip's
// kernel makes for its lane, so both give the same bits.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/render_mi355x_adaptive.h"
#include "adaptive_host.h"
#include "adaptive_ops.h"

using apt::kMaxPasses;

namespace apt {

int film_select_check(const apt_film_select *s, const void *moments, const void *extra, uint64_t pixel_count, const void *work, const void *list,
                      const void *count, const char *what) {
    if (!s || !moments || !extra || !work || !list || !count)
        return stage_set_error(APT_ERR_ARG, "%s: s/moments/extra/work/list/count must be non-null", what);
    if (s->struct_size != sizeof(apt_film_select)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_film_select.struct_size mismatch", what);
    if (int rc = stage_pixels_check(pixel_count, "pixel_count", what)) return rc;
    if (s->base_passes < 2 || s->base_passes > kMaxPasses) return stage_set_error(APT_ERR_ARG, "%s: base_passes must lie in [2, 2^24]", what);
    if (s->min_passes < 2 || s->max_passes > kMaxPasses || s->min_passes > s->max_passes)
        return stage_set_error(APT_ERR_ARG, "%s: 2 <= min_passes <= max_passes <= 2^24 must hold", what);
    if (!(std::isfinite(s->threshold) && s->threshold >= 0.0f) || !(std::isfinite(s->floor) && s->floor >= 0.0f))
        return stage_set_error(APT_ERR_ARG, "%s: threshold and floor must be finite and not negative", what);
    return APT_OK;
}

int film_accumulate_list_check(const void *pass_planes, const void *list, uint64_t list_count, uint64_t pixel_count, const void *film,
                               const void *moments, const void *extra, const char *what) {
    if (!pass_planes || !list || !film || !moments || !extra)
        return stage_set_error(APT_ERR_ARG, "%s: pass_planes/list/film/moments/extra must be non-null", what);
    if (int rc = stage_pixels_check(pixel_count, "pixel_count", what)) return rc;
    if (list_count > pixel_count) return stage_set_error(APT_ERR_ARG, "%s: list_count is larger than pixel_count", what);
    return APT_OK;
}

int film_mean_check(const void *film, uint32_t base_passes, uint64_t pixel_count, const void *out, const char *what) {
    if (!film || !out) return stage_set_error(APT_ERR_ARG, "%s: film/out must be non-null", what);
    if (int rc = stage_pixels_check(pixel_count, "pixel_count", what)) return rc;
    if (base_passes < 2 || base_passes > kMaxPasses) return stage_set_error(APT_ERR_ARG, "%s: base_passes must lie in [2, 2^24]", what);
    return APT_OK;
}
} // namespace apt
using apt::stage_set_error;

extern "C" {

const char *apt_film_adaptive_last_error(void) { return apt::stage_last_error(); }

int apt_film_select_default_host(apt_film_select *s, uint32_t base_passes) {
    apt::stage_clear_error();
    if (!s) return stage_set_error(APT_ERR_ARG, "%s: the record is null", "apt_film_select_default_host");
    if (base_passes < 2 || base_passes > kMaxPasses) return stage_set_error(APT_ERR_ARG, "%s: base_passes must lie in [2, 2^24]", "apt_film_select_default_host");
    memset(s, 0, sizeof *s);
    s->struct_size = sizeof *s;
    s->base_passes = base_passes;
    s->min_passes = base_passes > 4u ? base_passes : 4u;
    const uint64_t cap = 16ull * base_passes < kMaxPasses ? 16ull * base_passes : kMaxPasses;
    s->max_passes = cap > s->min_passes ? (uint32_t)cap : s->min_passes;
    s->threshold = 0.1f; s->floor = 0.0625f;   // DESIGN.md "Adaptive sampling": what the values rest on
    return APT_OK;
}

uint64_t apt_film_select_work_words(uint64_t pixel_count) { return (pixel_count + apt::kAdBlock - 1) / apt::kAdBlock; }

int apt_film_select_host(const apt_film_select *s, const float *moments, const uint32_t *extra, uint64_t pixel_count, uint32_t *work,
                         uint32_t *list, uint32_t *count) {
    apt::stage_clear_error();
    const int rc = apt::film_select_check(s, moments, extra, pixel_count, work, list, count, "apt_film_select_host");
    if (rc) return rc;
    const apt::AdSelect sel = {s->base_passes, s->min_passes, s->max_passes, s->threshold, s->floor};
    uint32_t k = 0;
    for (uint64_t p = 0; p < pixel_count; ++p)
        if (apt::ad_selected(moments[p], moments[pixel_count + p], extra[p], sel)) list[k++] = (uint32_t)p;
    *count = k;
    return APT_OK;
}

int apt_film_accumulate_list_host(const float *pass_planes, const uint32_t *list, uint64_t list_count, uint64_t pixel_count, float *film,
                                  float *moments, uint32_t *extra) {
    apt::stage_clear_error();
    const int rc = apt::film_accumulate_list_check(pass_planes, list, list_count, pixel_count, film, moments, extra, "apt_film_accumulate_list_host");
    if (rc) return rc;
    for (uint64_t i = 0; i < list_count; ++i) apt::ad_accumulate(pass_planes, list, list_count, film, moments, extra, pixel_count, i);
    return APT_OK;
}

int apt_film_mean_host(const float *film, const uint32_t *extra, uint32_t base_passes, uint64_t pixel_count, float *out) {
    apt::stage_clear_error();
    const int rc = apt::film_mean_check(film, base_passes, pixel_count, out, "apt_film_mean_host");
    if (rc) return rc;
    for (uint64_t i = 0; i < pixel_count; ++i) apt::ad_mean(film, extra, base_passes, out, pixel_count, i);
    return APT_OK;
}

} // extern "C"
