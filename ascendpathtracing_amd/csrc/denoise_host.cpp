// denoise_host.cpp -- the host side of libdenoise_mi355x.so (include/render_mi355x_denoise.h): the checks that the device and the host form of each entry share, the defaults and the CPU twins.  Compiled with the
// product's -ffp-contract=off -fno-fast-math: a twin is a loop over the pixels and the call of denoise_ops.h that denoise.hip's
// kernel makes for its lane, so both give the same bits.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/render_mi355x_denoise.h"
#include "denoise_host.h"
#include "denoise_ops.h"

using apt::stage_set_error;

extern "C" const char *apt_film_denoise_last_error(void) { return apt::stage_last_error(); }

namespace apt {
int film_accumulate_check(const void *pass_planes, uint64_t pixel_count, const void *film, const void *moments, const char *what) {
    if (!pass_planes || !film || !moments) return stage_set_error(APT_ERR_ARG, "%s: pass_planes/film/moments must be non-null", what);
    if ((pixel_count + 255) / 256 > 0x7fffffffull) return stage_set_error(APT_ERR_ARG, "%s: pixel_count too large for one launch; shard it", what);
    return APT_OK;
}

int film_denoise_check(const apt_film_denoise *d, const void *film, const void *moments, const void *features, uint32_t width, uint32_t height,
                       const void *work, const void *out, const char *what) {
    if (!d || !film || !moments || !features || !work || !out)
        return stage_set_error(APT_ERR_ARG, "%s: d/film/moments/features/work/out must be non-null", what);
    if (d->struct_size != sizeof(apt_film_denoise)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_film_denoise.struct_size mismatch", what);
    if ((uintptr_t)work & 15u) return stage_set_error(APT_ERR_ARG, "%s: work must be 16-byte aligned", what);
    if (!width || !height) return stage_set_error(APT_ERR_ARG, "%s: width/height must be non-zero", what);
    if (d->passes < 2 || d->passes > kMaxPasses) return stage_set_error(APT_ERR_ARG, "%s: passes must lie in [2, 2^24]", what);
    if (d->iterations < 1 || d->iterations > 5) return stage_set_error(APT_ERR_ARG, "%s: iterations must lie in [1, 5]", what);
    const float sig[5] = {d->sigma_n, d->sigma_z, d->sigma_c, d->sigma_a, d->sigma_l};
    for (float s : sig)
        if (!(std::isfinite(s) && s >= 0.0f)) return stage_set_error(APT_ERR_ARG, "%s: every sigma must be finite and not negative", what);
    if (!(std::isfinite(d->albedo_floor) && d->albedo_floor > 0.0f)) return stage_set_error(APT_ERR_ARG, "%s: albedo_floor must be finite and > 0", what);
    if ((uint64_t)width * height > kMaxPixels) return stage_set_error(APT_ERR_ARG, "%s: more than 2^28 pixels: too large for one launch", what);
    return APT_OK;
}
} // namespace apt

using apt::DnRec;

extern "C" {

int apt_film_accumulate_host(const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass) {
    apt::stage_clear_error();
    const int rc = apt::film_accumulate_check(pass_planes, pixel_count, film, moments, "apt_film_accumulate_host");
    if (rc) return rc;
    for (uint64_t i = 0; i < pixel_count; ++i) apt::dn_accumulate(pass_planes, film, moments, pixel_count, i, pass == 0);
    return APT_OK;
}

int apt_film_denoise_default_host(apt_film_denoise *d, uint32_t passes) {
    apt::stage_clear_error();
    if (!d) return stage_set_error(APT_ERR_ARG, "%s: the record is null", "apt_film_denoise_default_host");
    memset(d, 0, sizeof *d);
    d->struct_size = sizeof *d;
    d->passes = passes;
    d->iterations = 5;
    d->sigma_n = 32.0f; d->sigma_z = 10.0f; d->sigma_c = 8.0f; d->sigma_a = 8.0f; d->sigma_l = 3.0f;   // DESIGN.md "Denoise": the tuning
    d->albedo_floor = 0.03125f;
    return APT_OK;
}

uint64_t apt_film_denoise_work_floats(uint32_t width, uint32_t height) { return 16ull * width * height; }

int apt_film_denoise_host(const apt_film_denoise *d, const float *film, const float *moments, const float *features, uint32_t width,
                          uint32_t height, float *work, float *out) {
    apt::stage_clear_error();
    const int rc = apt::film_denoise_check(d, film, moments, features, width, height, work, out, "apt_film_denoise_host");
    if (rc) return rc;
    const uint32_t n = width * height;                                            // <= 2^28: the check above
    DnRec *const g0 = reinterpret_cast<DnRec *>(work), *const g1 = g0 + n, *const c[2] = {g1 + n, g1 + 2 * (size_t)n};
    const float K = (float)d->passes, K1 = (float)(d->passes - 1);
    for (uint32_t i = 0; i < n; ++i) apt::dn_prepare(film, moments, features, g0, g1, c[0], n, i, K, K1, d->albedo_floor);
    const apt::DnSigma sg = {d->sigma_n, d->sigma_z, d->sigma_c, d->sigma_a, d->sigma_l};
    for (uint32_t j = 0; j < d->iterations; ++j)
        for (int32_t x = 0; x < (int32_t)width; ++x)
            for (int32_t y = 0; y < (int32_t)height; ++y)
                apt::dn_iterate(g0, g1, c[j & 1], c[(j + 1) & 1], (int32_t)width, (int32_t)height, 1 << j, sg, x, y);
    for (uint32_t i = 0; i < n; ++i) apt::dn_finish(g1, c[d->iterations & 1], out, n, i);
    return APT_OK;
}

} // extern "C"
