// upscale_host.cpp -- the host side of libupscale_mi355x.so (include/render_mi355x_upscale.h): the checks that the device and the host form of each entry share, the defaults and the CPU twins.  Compiled with the
// product's -ffp-contract=off -fno-fast-math: a twin is a loop over the pixels and the call of upscale_ops.h that upscale.hip's
// kernel makes for its lane, so both give the same bits.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/render_mi355x_upscale.h"
#include "upscale_host.h"
#include "upscale_ops.h"

namespace apt {
int film_upscale_check(const apt_film_upscale *rec, const float *lo, const float *lo_features, uint32_t lo_width, uint32_t lo_height,
                       const float *hi_features, uint32_t width, uint32_t height, float *work, float *out, uint32_t *resolved, UpArgs *args,
                       const char *what) {
    if (!rec || !lo || !lo_features || !hi_features || !work || !out || !resolved)
        return stage_set_error(APT_ERR_ARG, "%s: rec/lo/lo_features/hi_features/work/out/resolved must be non-null", what);
    if (rec->struct_size != sizeof(apt_film_upscale)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_film_upscale.struct_size mismatch", what);
    if (lo_width == 0 || lo_height == 0 || width == 0 || height == 0) return stage_set_error(APT_ERR_ARG, "%s: a width or height is zero", what);
    if (lo_width > width || lo_height > height) return stage_set_error(APT_ERR_ARG, "%s: the low size must not exceed the full size", what);
    if (int rc = stage_pixels_check((uint64_t)width * height, "width * height", what)) return rc;
    if ((uintptr_t)work & 15u) return stage_set_error(APT_ERR_ARG, "%s: work must be 16-byte aligned", what);
    const void *ins[3] = {lo, lo_features, hi_features};
    const void *outs[3] = {work, out, resolved};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j)
            if (outs[i] == ins[j]) return stage_set_error(APT_ERR_ARG, "%s: work, out and resolved must not be an input", what);
        for (int j = i + 1; j < 3; ++j)
            if (outs[i] == outs[j]) return stage_set_error(APT_ERR_ARG, "%s: work, out and resolved must be three buffers", what);
    }
    const float sig[4] = {rec->sigma_n, rec->sigma_z, rec->sigma_c, rec->sigma_a};
    for (float s : sig)
        if (!(std::isfinite(s) && s >= 0.0f)) return stage_set_error(APT_ERR_ARG, "%s: a sigma must be finite and not negative", what);
    if (!(std::isfinite(rec->albedo_floor) && rec->albedo_floor > 0.0f))
        return stage_set_error(APT_ERR_ARG, "%s: albedo_floor must be finite and > 0", what);
    if (!(rec->min_weight > 0.0f && rec->min_weight <= 1.0f)) return stage_set_error(APT_ERR_ARG, "%s: min_weight must lie in (0, 1]", what);
    const uint64_t nl = (uint64_t)lo_width * lo_height;
    args->lo = lo; args->lf = lo_features; args->hf = hi_features;
    args->ci = reinterpret_cast<UpRec *>(work); args->gn = args->ci + nl; args->ga = args->gn + nl;
    args->out = out; args->resolved = resolved;
    args->lw = lo_width; args->lh = lo_height; args->w = width; args->h = height;
    args->sn = rec->sigma_n; args->sz = rec->sigma_z; args->sc = rec->sigma_c; args->sa = rec->sigma_a;
    args->albedo_floor = rec->albedo_floor; args->min_weight = rec->min_weight;
    return APT_OK;
}

int film_upscale_patch_check(const void *sums, const void *list, uint64_t list_count, uint32_t passes, uint64_t pixel_count, const void *out,
                             const char *what) {
    if (!sums || !list || !out) return stage_set_error(APT_ERR_ARG, "%s: sums/list/out must be non-null", what);
    if (int rc = stage_passes_check(passes, "passes", what)) return rc;
    if (int rc = stage_pixels_check(pixel_count, "pixel_count", what)) return rc;
    if (list_count > kMaxPixels) return stage_set_error(APT_ERR_ARG, "%s: list_count must not exceed 2^28", what);
    if (out == sums) return stage_set_error(APT_ERR_ARG, "%s: out must not be sums", what);
    return APT_OK;
}
} // namespace apt
using apt::stage_set_error;

extern "C" {

const char *apt_film_upscale_last_error(void) { return apt::stage_last_error(); }

int apt_film_upscale_default_host(apt_film_upscale *rec) {
    apt::stage_clear_error();
    if (!rec) return stage_set_error(APT_ERR_ARG, "%s: the record is null", "apt_film_upscale_default_host");
    memset(rec, 0, sizeof *rec);
    rec->struct_size = sizeof *rec;
    rec->sigma_n = 32.0f; rec->sigma_z = 10.0f; rec->sigma_c = 8.0f; rec->sigma_a = 8.0f;   // the denoiser's values: not tuned for this use
    rec->albedo_floor = 0.03125f;
    rec->min_weight = 0.015625f;
    return APT_OK;
}

uint64_t apt_film_upscale_work_floats(uint32_t lo_width, uint32_t lo_height) { return 12ull * lo_width * lo_height; }

int apt_film_upscale_host(const apt_film_upscale *rec, const float *lo, const float *lo_features, uint32_t lo_width, uint32_t lo_height,
                          const float *hi_features, uint32_t width, uint32_t height, float *work, float *out, uint32_t *resolved) {
    apt::stage_clear_error();
    apt::UpArgs a;
    const int rc = apt::film_upscale_check(rec, lo, lo_features, lo_width, lo_height, hi_features, width, height, work, out, resolved, &a,
                                           "apt_film_upscale_host");
    if (rc) return rc;
    const uint64_t nl = (uint64_t)lo_width * lo_height;
    for (uint64_t i = 0; i < nl; ++i) apt::up_prepare(a, nl, i);
    for (uint32_t x = 0; x < width; ++x)
        for (uint32_t y = 0; y < height; ++y) apt::up_pixel(a, x, y);
    return APT_OK;
}

int apt_film_upscale_patch_host(const float *sums, const uint32_t *list, uint64_t list_count, uint32_t passes, uint64_t pixel_count,
                                float *out) {
    apt::stage_clear_error();
    const int rc = apt::film_upscale_patch_check(sums, list, list_count, passes, pixel_count, out, "apt_film_upscale_patch_host");
    if (rc) return rc;
    for (uint64_t i = 0; i < list_count; ++i) apt::up_patch(sums, list, list_count, (float)passes, pixel_count, out, i);
    return APT_OK;
}

} // extern "C"
