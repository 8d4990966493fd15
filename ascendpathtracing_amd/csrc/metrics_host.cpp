// metrics_host.cpp -- the host side of libmetrics_mi355x.so (include/render_mi355x_metrics.h): the checks that the device and the host form of each entry share, the defaults, the work sizes and the CPU twins.  Compiled
// with the product's -ffp-contract=off -fno-fast-math: a twin is a loop over the pixels and the call of metrics_ops.h that
// metrics.hip's kernel makes for its lane, and its sums are metrics_ops.h's MxTree, the header's tree: so both give the same bits.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/render_mi355x_metrics.h"
#include "metrics_host.h"
#include "metrics_ops.h"

namespace {
constexpr uint32_t kMinSide = APT_SSIM_TAPS;

bool positive(float v) { return std::isfinite(v) && v > 0.0f; }
}

using apt::kMaxPixels;

namespace apt {
// both pass counts of a record, under the one name the message gives them
static int passes_check(uint32_t passes_a, uint32_t passes_b, const char *what) {
    if (int rc = stage_passes_check(passes_a, "passes_a and passes_b", what)) return rc;
    return stage_passes_check(passes_b, "passes_a and passes_b", what);
}

static int record_check(const apt_film_compare *c, MxRec *rec, const char *what) {
    if (c->struct_size != sizeof(apt_film_compare)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_film_compare.struct_size mismatch", what);
    if (int rc = passes_check(c->passes_a, c->passes_b, what)) return rc;
    if (!positive(c->exposure) || !positive(c->eps)) return stage_set_error(APT_ERR_ARG, "%s: exposure and eps must be finite and positive", what);
    *rec = mx_rec(c->passes_a, c->passes_b, c->exposure, c->eps);
    return APT_OK;
}

int film_compare_check(const apt_film_compare *c, const float *a, const float *b, uint64_t pixel_count, const void *work, bool need_work,
                       const void *result, const void *err_map, MxRec *rec, const char *what) {
    if (!c || !a || !b || !result || (need_work && !work)) return stage_set_error(APT_ERR_ARG, "%s: c/a/b/work/result must be non-null", what);
    if (int rc = record_check(c, rec, what)) return rc;
    if (int rc = stage_pixels_check(pixel_count, "pixel_count", what)) return rc;
    if (need_work && (uintptr_t)work % 8 != 0) return stage_set_error(APT_ERR_ARG, "%s: work must be 8-byte aligned", what);
    if (result == a || result == b || (err_map && (err_map == a || err_map == b || err_map == result)) ||
        (need_work && (work == a || work == b || work == result || work == err_map)))
        return stage_set_error(APT_ERR_ARG, "%s: result, err_map and work must be neither an input nor one another", what);
    return APT_OK;
}

int film_ssim_check(const apt_film_compare *c, const float *a, const float *b, uint32_t width, uint32_t height, const void *work,
                    bool need_work, const void *result, const void *ssim_map, MxRec *rec, const char *what) {
    if (!c || !a || !b || !result || (need_work && !work)) return stage_set_error(APT_ERR_ARG, "%s: c/a/b/work/result must be non-null", what);
    if (int rc = record_check(c, rec, what)) return rc;
    if (width < kMinSide || height < kMinSide) return stage_set_error(APT_ERR_ARG, "%s: width and height must be at least 11", what);
    if ((uint64_t)width * height > kMaxPixels) return stage_set_error(APT_ERR_ARG, "%s: width * height must not exceed 2^28", what);
    if (need_work && (uintptr_t)work % 16 != 0) return stage_set_error(APT_ERR_ARG, "%s: work must be 16-byte aligned", what);
    if (result == a || result == b || (ssim_map && (ssim_map == a || ssim_map == b || ssim_map == result)) ||
        (need_work && (work == a || work == b || work == result || work == ssim_map)))
        return stage_set_error(APT_ERR_ARG, "%s: result, ssim_map and work must be neither an input nor one another", what);
    return APT_OK;
}
} // namespace apt
using apt::stage_set_error;

extern "C" {

const char *apt_film_metrics_last_error(void) { return apt::stage_last_error(); }

int apt_film_compare_default_host(apt_film_compare *c, uint32_t passes_a, uint32_t passes_b) {
    apt::stage_clear_error();
    const char *what = "apt_film_compare_default_host";
    if (!c) return stage_set_error(APT_ERR_ARG, "%s: the record is null", what);
    if (int rc = apt::passes_check(passes_a, passes_b, what)) return rc;
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;
    c->passes_a = passes_a; c->passes_b = passes_b;
    c->exposure = 1.0f; c->eps = 1e-2f;
    return APT_OK;
}

uint64_t apt_film_compare_work_doubles(uint64_t pixel_count) {
    if (pixel_count < 1 || pixel_count > kMaxPixels) return 0;
    const apt::MxRows r = apt::mx_rows(pixel_count);
    return (uint64_t)apt::kMxCompareRowWords * (r.r0 + r.r1);
}

int apt_film_compare_host(const apt_film_compare *c, const float *a, const float *b, uint64_t pixel_count, uint64_t *result, float *err_map) {
    apt::stage_clear_error();
    apt::MxRec p;
    const int rc = apt::film_compare_check(c, a, b, pixel_count, nullptr, false, result, err_map, &p, "apt_film_compare_host");
    if (rc) return rc;
    const uint64_t n = pixel_count;
    apt::MxTree<4> tree;
    uint64_t key = 0, bad = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const float pa[3] = {a[i], a[n + i], a[2 * n + i]}, pb[3] = {b[i], b[n + i], b[2 * n + i]};
        const apt::MxTerms t = apt::mx_pixel(pa, pb, (uint32_t)i, p);
        const float terms[4] = {t.se, t.cse, t.rse, t.ae};
        tree.push(terms);
        key = t.key > key ? t.key : key;
        bad += t.bad;
        if (err_map) err_map[i] = t.se;
    }
    double sums[4];
    tree.finish(sums);
    for (int s = 0; s < 4; ++s) memcpy(&result[s], &sums[s], sizeof(double));
    result[4] = key; result[5] = bad; result[6] = n; result[7] = 0;
    return APT_OK;
}

int apt_film_ssim_weights_host(float *w) {
    apt::stage_clear_error();
    if (!w) return stage_set_error(APT_ERR_ARG, "%s: w is null", "apt_film_ssim_weights_host");
    for (int k = 0; k < APT_SSIM_TAPS; ++k) w[k] = apt::mx_weight(k);
    return APT_OK;
}

uint64_t apt_film_ssim_work_bytes(uint32_t width, uint32_t height) {
    if (width < kMinSide || height < kMinSide || (uint64_t)width * height > kMaxPixels) return 0;
    const uint64_t windows = (uint64_t)(width - 10) * (height - 10);
    const apt::MxRows r = apt::mx_rows(windows);
    const uint64_t rows = ((uint64_t)r.r0 + r.r1 + 1) & ~1ull;     // an even number of doubles: the map after them is 16-byte aligned
    return 8 * rows + 4 * ((windows + 3) & ~3ull);
}

int apt_film_ssim_host(const apt_film_compare *c, const float *a, const float *b, uint32_t width, uint32_t height, uint64_t *result,
                       float *ssim_map) {
    apt::stage_clear_error();
    apt::MxRec p;
    const int rc = apt::film_ssim_check(c, a, b, width, height, nullptr, false, result, ssim_map, &p, "apt_film_ssim_host");
    if (rc) return rc;
    const uint64_t W = width, H = height, N = W * H, wh = H - 10;
    apt::MxTree<1> tree;
    // window column ox: the x pass at every y in turn, its last 11 results kept in a ring; from y = 10 on a window is complete
    for (uint64_t ox = 0; ox + 10 < W; ++ox) {
        float ring[APT_SSIM_TAPS][5];
        for (uint64_t y = 0; y < H; ++y) {
            float *h = ring[y % APT_SSIM_TAPS];
            for (int q = 0; q < 5; ++q) h[q] = 0.0f;
            for (int k = 0; k < APT_SSIM_TAPS; ++k) {
                const uint64_t i = (ox + k) * H + y;
                const float ya = apt::mx_display_lum(a[i], a[N + i], a[2 * N + i], p.Ka, p.inv_a, p.exposure);
                const float yb = apt::mx_display_lum(b[i], b[N + i], b[2 * N + i], p.Kb, p.inv_b, p.exposure);
                apt::mx_tap_source(h, apt::mx_weight(k), ya, yb);
            }
            if (y < 10) continue;
            const uint64_t oy = y - 10;
            float f[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < APT_SSIM_TAPS; ++k) apt::mx_tap_planes(f, apt::mx_weight(k), ring[(oy + k) % APT_SSIM_TAPS]);
            const float s = apt::mx_ssim(f);
            tree.push(&s);
            if (ssim_map) ssim_map[ox * wh + oy] = s;
        }
    }
    double sum;
    tree.finish(&sum);
    memcpy(&result[0], &sum, sizeof sum);
    result[1] = (W - 10) * wh;
    return APT_OK;
}

} // extern "C"
