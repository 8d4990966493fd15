// denoise_host.cpp -- the host side of libdenoise_mi355x.so (include/render_mi355x_denoise.h): the library's own per-thread error
// record, the checks that the device and the host form of each entry share, the defaults and the CPU twins.  Compiled with the
// product's -ffp-contract=off -fno-fast-math: the twins are denoise.hip's kernels' text and give the same bits.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <string>

#include "../../include/render_mi355x_denoise.h"
#include "denoise_host.h"

namespace {
thread_local std::string t_dn_err;
}

namespace apt {
void dn_clear_error() { t_dn_err.clear(); }
int dn_set_error(int code, const char *fmt, const char *what) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, what);
    t_dn_err = buf;
    return code;
}
} // namespace apt
using apt::dn_set_error;

extern "C" const char *apt_film_denoise_last_error(void) { return t_dn_err.c_str(); }

namespace apt {
int film_accumulate_check(const void *pass_planes, uint64_t pixel_count, const void *film, const void *moments, const char *what) {
    if (!pass_planes || !film || !moments) return dn_set_error(APT_ERR_ARG, "%s: pass_planes/film/moments must be non-null", what);
    if ((pixel_count + 255) / 256 > 0x7fffffffull) return dn_set_error(APT_ERR_ARG, "%s: pixel_count too large for one launch; shard it", what);
    return APT_OK;
}

int film_denoise_check(const apt_film_denoise *d, const void *film, const void *moments, const void *features, uint32_t width, uint32_t height,
                       const void *work, const void *out, const char *what) {
    if (!d || !film || !moments || !features || !work || !out)
        return dn_set_error(APT_ERR_ARG, "%s: d/film/moments/features/work/out must be non-null", what);
    if (d->struct_size != sizeof(apt_film_denoise)) return dn_set_error(APT_ERR_STRUCT, "%s: apt_film_denoise.struct_size mismatch", what);
    if ((uintptr_t)work & 15u) return dn_set_error(APT_ERR_ARG, "%s: work must be 16-byte aligned", what);
    if (!width || !height) return dn_set_error(APT_ERR_ARG, "%s: width/height must be non-zero", what);
    if (d->passes < 2 || d->passes > (1u << 24)) return dn_set_error(APT_ERR_ARG, "%s: passes must lie in [2, 2^24]", what);
    if (d->iterations < 1 || d->iterations > 5) return dn_set_error(APT_ERR_ARG, "%s: iterations must lie in [1, 5]", what);
    const float sig[5] = {d->sigma_n, d->sigma_z, d->sigma_c, d->sigma_a, d->sigma_l};
    for (float s : sig)
        if (!(std::isfinite(s) && s >= 0.0f)) return dn_set_error(APT_ERR_ARG, "%s: every sigma must be finite and not negative", what);
    if (!(std::isfinite(d->albedo_floor) && d->albedo_floor > 0.0f)) return dn_set_error(APT_ERR_ARG, "%s: albedo_floor must be finite and > 0", what);
    if ((uint64_t)width * height > (1ull << 28)) return dn_set_error(APT_ERR_ARG, "%s: more than 2^28 pixels: too large for one launch", what);
    return APT_OK;
}
} // namespace apt

// The header's operations one at a time; denoise.hip's kernels are the same text.
static inline float dn_lum(float r, float g, float b) {
    float l = 0.2126f * r;
    l = l + 0.7152f * g;
    return l + 0.0722f * b;
}
static inline float dn_max(float a, float b) { return a > b ? a : b; }

namespace {
struct DnRec { float a, b, c, d; };   // one 16-byte record of the work buffer

// One a-trous iteration of the header at pixel (x, y): g0 = (n, z), g1 = (A, cov), in = (i, vi).
DnRec dn_iterate(const apt_film_denoise &p, const DnRec *g0, const DnRec *g1, const DnRec *in, int32_t W, int32_t H, int32_t s, int32_t x,
                 int32_t y) {
    static const float B[3] = {1.0f, 2.0f, 1.0f};
    static const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sv = 0.0f, sw = 0.0f;
    for (int32_t ex = -1; ex <= 1; ++ex)
        for (int32_t ey = -1; ey <= 1; ++ey) {
            const int32_t qx = x + ex, qy = y + ey;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float b = B[ex + 1] * B[ey + 1];
            sv = sv + b * in[(size_t)qx * H + qy].d;
            sw = sw + b;
        }
    const float gv = sv / sw;
    float e = sqrtf(gv) * p.sigma_l;
    e = e + 1e-6f;
    const float isd = 1.0f / e;
    const size_t ip = (size_t)x * H + y;
    const DnRec n_p = g0[ip], a_p = g1[ip], c_p = in[ip];
    const float zz = n_p.d + 1e-6f;
    const float iz = 1.0f / zz;
    const float lp = dn_lum(c_p.a, c_p.b, c_p.c);
    float Wt = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, V = 0.0f;
    for (int32_t dx = -2; dx <= 2; ++dx)
        for (int32_t dy = -2; dy <= 2; ++dy) {
            const int64_t qx = (int64_t)x + (int64_t)dx * s, qy = (int64_t)y + (int64_t)dy * s;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const size_t iq = (size_t)qx * H + (size_t)qy;
            const DnRec n_q = g0[iq], a_q = g1[iq], c_q = in[iq];
            const float cc = a_p.d * a_q.d;
            float dt = 0.0f + n_p.a * n_q.a;
            dt = dt + n_p.b * n_q.b;
            dt = dt + n_p.c * n_q.c;
            const float xn = p.sigma_n * dn_max(cc - dt, 0.0f);
            const float xz = (p.sigma_z * fabsf(n_p.d - n_q.d)) * iz;
            const float xc = p.sigma_c * fabsf(a_p.d - a_q.d);
            float da = fabsf(a_p.a - a_q.a) + fabsf(a_p.b - a_q.b);
            da = da + fabsf(a_p.c - a_q.c);
            const float xa = p.sigma_a * da;
            const float lq = dn_lum(c_q.a, c_q.b, c_q.c);
            const float xl = fabsf(lp - lq) * isd;
            float xs = xn + xz;
            xs = xs + xc;
            xs = xs + xa;
            xs = xs + xl;
            float t = dn_max(1.0f - xs * 0.125f, 0.0f);
            t = t * t;
            t = t * t;
            const float g = dx == 0 && dy == 0 ? 1.0f : t * t;                // the centre tap: x = 0 by definition
            const float w = (h[dx + 2] * h[dy + 2]) * g;
            Wt = Wt + w;
            Sr = Sr + w * c_q.a;
            Sg = Sg + w * c_q.b;
            Sb = Sb + w * c_q.c;
            V = V + (w * w) * c_q.d;
        }
    return {Sr / Wt, Sg / Wt, Sb / Wt, V / (Wt * Wt)};
}
} // namespace

extern "C" {

int apt_film_accumulate_host(const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass) {
    apt::dn_clear_error();
    const int rc = apt::film_accumulate_check(pass_planes, pixel_count, film, moments, "apt_film_accumulate_host");
    if (rc) return rc;
    const uint64_t n = pixel_count;
    for (uint64_t i = 0; i < n; ++i) {
        const float r = pass_planes[i], g = pass_planes[n + i], b = pass_planes[2 * n + i];
        const float l = dn_lum(r, g, b);
        const float l2 = l * l;
        if (pass == 0) {
            film[i] = r; film[n + i] = g; film[2 * n + i] = b;
            moments[i] = l; moments[n + i] = l2;
        } else {
            film[i] = film[i] + r; film[n + i] = film[n + i] + g; film[2 * n + i] = film[2 * n + i] + b;
            moments[i] = moments[i] + l; moments[n + i] = moments[n + i] + l2;
        }
    }
    return APT_OK;
}

int apt_film_denoise_default_host(apt_film_denoise *d, uint32_t passes) {
    apt::dn_clear_error();
    if (!d) return dn_set_error(APT_ERR_ARG, "%s: the record is null", "apt_film_denoise_default_host");
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
    apt::dn_clear_error();
    const int rc = apt::film_denoise_check(d, film, moments, features, width, height, work, out, "apt_film_denoise_host");
    if (rc) return rc;
    const size_t n = (size_t)width * height;
    DnRec *g0 = reinterpret_cast<DnRec *>(work), *g1 = g0 + n, *c[2] = {g1 + n, g1 + 2 * n};
    const float K = (float)d->passes, K1 = (float)(d->passes - 1);
    for (size_t i = 0; i < n; ++i) {                                              // prepare
        const float cov = features[APT_FEATURE_COVERAGE * n + i];
        const float u = 1.0f - cov;
        float A[3], il[3];
        for (size_t ch = 0; ch < 3; ++ch) {
            const float cm = film[ch * n + i] / K;
            A[ch] = dn_max(features[(APT_FEATURE_ALBEDO + ch) * n + i] + u, d->albedo_floor);
            il[ch] = cm / A[ch];
        }
        const float lm = moments[i] / K, q = moments[n + i] / K;
        const float v = dn_max(q - lm * lm, 0.0f) / K1;
        const float LA = dn_lum(A[0], A[1], A[2]);
        const float vi = v / (LA * LA);
        g0[i] = {features[APT_FEATURE_NORMAL * n + i], features[(APT_FEATURE_NORMAL + 1) * n + i], features[(APT_FEATURE_NORMAL + 2) * n + i],
                 features[APT_FEATURE_DEPTH * n + i]};
        g1[i] = {A[0], A[1], A[2], cov};
        c[0][i] = {il[0], il[1], il[2], vi};
    }
    for (uint32_t j = 0; j < d->iterations; ++j)
        for (int32_t x = 0; x < (int32_t)width; ++x)
            for (int32_t y = 0; y < (int32_t)height; ++y)
                c[(j + 1) & 1][(size_t)x * height + y] = dn_iterate(*d, g0, g1, c[j & 1], (int32_t)width, (int32_t)height, 1 << j, x, y);
    const DnRec *fin = c[d->iterations & 1];
    for (size_t i = 0; i < n; ++i) {                                              // finish
        out[i] = fin[i].a * g1[i].a;
        out[n + i] = fin[i].b * g1[i].b;
        out[2 * n + i] = fin[i].c * g1[i].c;
    }
    return APT_OK;
}

} // extern "C"
