// upscale_driver.cpp -- CPU sanitizer driver for the host code of guided film upscaling (include/render_mi355x_upscale.h;
// tests/test_film_stage_sanitizers.py builds it with -fsanitize=address,undefined together with csrc/upscale_host.cpp and csrc/film_stage_host.cpp; no GPU, no HIP):
// apt_film_upscale_host and apt_film_upscale_patch_host on the sizes of the CPU test, every buffer an exactly sized heap block (a
// stray access is ASan's to see), `work` from posix_memalign, with NaN and zero-coverage pixels among the planes.  What it computes
// is also CHECKED.
// Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/render_mi355x_upscale.h"

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static float rnd() {                                       // splitmix64 -> [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (float)((z ^ (z >> 31)) >> 40) * (1.0f / 16777216.0f);
}

// exactly sized heap blocks: malloc for the planes, posix_memalign for `work`
static float *floats(size_t n, float fill) {
    float *p = (float *)malloc(n * sizeof(float) + (n == 0));
    if (!p) exit(2);
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

// planes of a wall z = 100 (normal +z) split into a left and a right albedo, with a few zero-coverage and partly covered pixels
static float *wall(uint32_t w, uint32_t h) {
    const size_t n = (size_t)w * h;
    float *f = floats(8 * n, 0.0f);
    for (uint32_t x = 0; x < w; ++x)
        for (uint32_t y = 0; y < h; ++y) {
            const size_t i = (size_t)x * h + y;
            const float cov = i % 7 == 3 ? 0.0f : (i % 5 == 1 ? 0.5f + 0.5f * rnd() : 1.0f);
            const float a = 2 * x < w ? 0.25f : 0.75f;
            f[i] = cov; f[n + i] = 100.0f * cov; f[4 * n + i] = cov;
            for (int k = 5; k < 8; ++k) f[k * n + i] = a * cov;
        }
    return f;
}

int main() {
    const uint32_t sizes[][4] = {{1, 1, 1, 1}, {1, 1, 3, 2}, {1, 4, 1, 7}, {4, 1, 7, 1}, {3, 2, 5, 3}, {4, 4, 8, 8}, {7, 5, 33, 17},
                                 {5, 3, 5, 3}, {24, 16, 48, 32}};
    apt_film_upscale rec;
    CHECK(apt_film_upscale_default_host(&rec) == APT_OK && rec.struct_size == sizeof rec && rec.sigma_n == 32.0f && rec.min_weight == 0.015625f, "defaults");
    CHECK(apt_film_upscale_default_host(nullptr) == APT_ERR_ARG, "null record");
    for (const auto &s : sizes) {
        const uint32_t lw = s[0], lh = s[1], w = s[2], h = s[3];
        const size_t nl = (size_t)lw * lh, n = (size_t)w * h;
        CHECK(apt_film_upscale_work_floats(lw, lh) == 12 * nl, "work floats");
        for (int which = 0; which < 3; ++which) {                           // clean; NaN in the planes and the radiance; min_weight 1
            float *lf = wall(lw, lh), *hf = wall(w, h);
            if (nl == n) memcpy(hf, lf, 8 * n * sizeof(float));            // equal sizes: equal features (the random coverages differ)
            float *lo = floats(3 * nl, 0.0f), *out = floats(3 * n, NAN);
            uint32_t *res = (uint32_t *)malloc(n * sizeof(uint32_t));
            void *wk = nullptr;
            if (!res || posix_memalign(&wk, 16, 12 * nl * sizeof(float))) exit(2);
            float *work = (float *)wk;
            for (size_t i = 0; i < n; ++i) res[i] = 7u;
            for (size_t i = 0; i < 12 * nl; ++i) work[i] = -3.5f;
            const float c = 0.5f;                                           // lo = A_q * c: out = A_p * c everywhere (closed form (a))
            for (size_t i = 0; i < nl; ++i)
                for (int k = 0; k < 3; ++k) {
                    const float a = lf[(5 + k) * nl + i] + (1.0f - lf[i]);
                    lo[k * nl + i] = (a > 0.03125f ? a : 0.03125f) * c;
                }
            apt_film_upscale r = rec;
            if (which == 1 && nl > 4) { lf[nl + 2] = NAN; lo[1] = NAN; hf[4 * n + n / 2] = NAN; }
            if (which == 2) r.min_weight = 1.0f;
            CHECK(apt_film_upscale_host(&r, lo, lf, lw, lh, hf, w, h, work, out, res) == APT_OK, "upscale %ux%u -> %ux%u/%d: %s", lw, lh, w, h, which,
                  apt_film_upscale_last_error());
            size_t unresolved = 0;
            for (size_t i = 0; i < n; ++i) {
                CHECK(res[i] <= 1u, "resolved[%zu] = %u", i, res[i]);
                unresolved += res[i] == 0;
                if (which != 1)
                    for (int k = 0; k < 3; ++k) {
                        const float a = hf[(5 + k) * n + i] + (1.0f - hf[i]);
                        const double want = (double)(a > 0.03125f ? a : 0.03125f) * c;
                        CHECK(fabs(out[k * n + i] - want) <= 12 * 5.96e-8 * want, "pixel %zu channel %d: %g, expected %g", i, k, out[k * n + i], want);
                    }
            }
            for (size_t i = 0; i < nl; ++i) {
                CHECK(work[4 * (2 * nl + i) + 3] == 0.0f, "the third record's last word of low pixel %zu", i);
                CHECK(work[4 * i + 3] == lf[i] || isnan(lf[i]), "the first record's coverage of low pixel %zu", i);
            }
            if (which == 0 && lw == w && lh == h) CHECK(unresolved == 0, "equal sizes and features resolve every pixel: %zu", unresolved);

            // the patch over the unresolved pixels and two entries beyond the image, on exactly sized blocks
            const size_t count = unresolved + 2;
            uint32_t *list = (uint32_t *)malloc(count * sizeof(uint32_t));
            if (!list) exit(2);
            float *sums = floats(3 * count, 0.0f);
            size_t k = 0;
            list[k++] = (uint32_t)n;
            for (size_t i = 0; i < n; ++i)
                if (res[i] == 0) list[k++] = (uint32_t)i;
            list[k++] = 0xFFFFFFFFu;
            CHECK(k == count, "the list's length");
            for (size_t i = 0; i < 3 * count; ++i) sums[i] = 4.0f * (float)(i + 1);
            float *before = floats(3 * n, 0.0f);
            memcpy(before, out, 3 * n * sizeof(float));
            CHECK(apt_film_upscale_patch_host(sums, list, count, 4, n, out) == APT_OK, "patch");
            for (size_t i = 0, j = 1; i < n; ++i) {
                if (res[i] == 0) { CHECK(out[n + i] == (float)(count + j + 1), "patched pixel %zu", i); ++j; }
                else CHECK(out[n + i] == before[n + i] || isnan(before[n + i]), "pixel %zu is not listed", i);
            }
            CHECK(apt_film_upscale_patch_host(sums, list, 0, 4, n, out) == APT_OK, "an empty list");
            CHECK(apt_film_upscale_patch_host(sums, list, count, 0, n, out) == APT_ERR_ARG, "passes 0");
            CHECK(apt_film_upscale_patch_host(nullptr, list, count, 1, n, out) == APT_ERR_ARG, "null sums");

            // refusals: nothing written
            float *keep = floats(3 * n, -7.0f);
            apt_film_upscale bad = rec;
            bad.min_weight = 0.0f;
            CHECK(apt_film_upscale_host(&bad, lo, lf, lw, lh, hf, w, h, work, keep, res) == APT_ERR_ARG, "min_weight 0");
            bad = rec; bad.struct_size = 28;
            CHECK(apt_film_upscale_host(&bad, lo, lf, lw, lh, hf, w, h, work, keep, res) == APT_ERR_STRUCT, "struct_size");
            bad = rec; bad.sigma_z = -1.0f;
            CHECK(apt_film_upscale_host(&bad, lo, lf, lw, lh, hf, w, h, work, keep, res) == APT_ERR_ARG, "a negative sigma");
            CHECK(apt_film_upscale_host(&rec, lo, lf, w + 1, lh, hf, w, h, work, keep, res) == APT_ERR_ARG, "a low width above the full one");
            CHECK(apt_film_upscale_host(&rec, lo, lf, lw, lh, hf, w, 0, work, keep, res) == APT_ERR_ARG, "zero height");
            CHECK(apt_film_upscale_host(&rec, lo, lf, lw, lh, hf, w, h, work + 1, keep, res) == APT_ERR_ARG, "work not aligned");
            CHECK(apt_film_upscale_host(&rec, lo, lf, lw, lh, hf, w, h, work, lo, res) == APT_ERR_ARG, "out is an input");
            CHECK(apt_film_upscale_host(&rec, lo, lf, lw, lh, hf, w, h, work, work, res) == APT_ERR_ARG, "out is work");
            CHECK(apt_film_upscale_last_error()[0] != 0, "the refusal has a text");
            for (size_t i = 0; i < 3 * n; ++i) CHECK(keep[i] == -7.0f, "a refusal writes nothing");
            free(keep); free(before); free(sums); free(list); free(work); free(res); free(out); free(lo); free(hf); free(lf);
        }
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
