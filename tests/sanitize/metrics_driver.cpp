// metrics_driver.cpp -- CPU sanitizer driver for the host code of the film comparison metrics (include/render_mi355x_metrics.h;
// tests/test_film_stage_sanitizers.py builds it with -fsanitize=address,undefined together with csrc/metrics_host.cpp and csrc/film_stage_host.cpp; no GPU, no HIP):
// apt_film_compare_host and apt_film_ssim_host on the sizes of the CPU test, every buffer an exactly sized heap block (a stray access
// is ASan's to see), with NaN, infinite and huge pixels in the films.  What it computes is also CHECKED.
// Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/render_mi355x_metrics.h"

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static float rnd() {                                       // splitmix64 -> [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (float)((z ^ (z >> 31)) >> 40) * (1.0f / 16777216.0f);
}
static double as_double(uint64_t w) {
    double d;
    memcpy(&d, &w, sizeof d);
    return d;
}

static void compare_checks() {
    const uint64_t sizes[] = {1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097};
    apt_film_compare rec;
    CHECK(apt_film_compare_default_host(&rec, 3, 2) == APT_OK && rec.struct_size == sizeof rec && rec.passes_a == 3 && rec.passes_b == 2 &&
          rec.exposure == 1.0f && rec.eps == 1e-2f, "defaults");
    CHECK(apt_film_compare_default_host(nullptr, 3, 2) == APT_ERR_ARG && apt_film_compare_default_host(&rec, 0, 1) == APT_ERR_ARG, "refused defaults");
    CHECK(apt_film_compare_default_host(&rec, 3, 2) == APT_OK, "defaults again");
    const float specials[] = {NAN, INFINITY, -INFINITY, 1.152921504606846976e18f * 3.0f, -4e18f};
    for (uint64_t n : sizes) {
        std::vector<float> a(3 * n), b(3 * n), map(n, NAN);
        for (uint64_t i = 0; i < 3 * n; ++i) {
            const float s = exp2f(40.0f * rnd() - 20.0f);
            b[i] = 2.0f * s;
            a[i] = 3.0f * s * (0.5f + rnd());
        }
        // every 7th pixel from the third is bad, through a or through b
        uint64_t chosen = 0;
        for (uint64_t i = 2; i < n; i += 7, ++chosen) (i % 2 ? a : b)[(i % 3) * n + i] = specials[(i / 7) % 5];
        std::vector<uint64_t> res(APT_COMPARE_WORDS, 0xDEADBEEFull);
        CHECK(apt_film_compare_host(&rec, a.data(), b.data(), n, res.data(), map.data()) == APT_OK, "compare of %llu", (unsigned long long)n);
        CHECK(res[5] == chosen && res[6] == n && res[7] == 0, "bad %llu of %llu, chosen %llu", (unsigned long long)res[5], (unsigned long long)n, (unsigned long long)chosen);
        double se = 0.0;
        for (uint64_t i = 0; i < n; ++i) {
            CHECK(map[i] >= 0.0f && isfinite(map[i]), "map[%llu] = %g", (unsigned long long)i, map[i]);
            se += map[i];
        }
        for (int k = 0; k < 4; ++k) CHECK(as_double(res[k]) >= 0.0 && isfinite(as_double(res[k])), "sum %d = %g", k, as_double(res[k]));
        CHECK(fabs(as_double(res[0]) - se) <= 1e-9 * se, "the tree sum %g against a sequential one %g", as_double(res[0]), se);
        if (chosen < n) CHECK(res[4] != 0 && 0xFFFFFFFFull - (res[4] & 0xFFFFFFFFull) < n, "the key's index");
        else CHECK(res[4] == 0, "no good pixel: key 0");
        // without a map, and a film against itself
        std::vector<uint64_t> res2(APT_COMPARE_WORDS);
        CHECK(apt_film_compare_host(&rec, a.data(), b.data(), n, res2.data(), nullptr) == APT_OK && res2 == res, "without a map");
        apt_film_compare same = rec;
        same.passes_b = same.passes_a;
        CHECK(apt_film_compare_host(&same, a.data(), a.data(), n, res2.data(), nullptr) == APT_OK, "a against a");
        for (int k = 0; k < 4; ++k) CHECK(res2[k] == 0, "a against a: sum %d", k);
        // refusals: nothing written
        std::vector<uint64_t> keep(APT_COMPARE_WORDS, 7u);
        std::vector<float> kmap(n, -7.0f);
        apt_film_compare bad = rec;
        bad.exposure = 0.0f;
        CHECK(apt_film_compare_host(&bad, a.data(), b.data(), n, keep.data(), kmap.data()) == APT_ERR_ARG, "exposure 0");
        bad = rec; bad.eps = NAN;
        CHECK(apt_film_compare_host(&bad, a.data(), b.data(), n, keep.data(), kmap.data()) == APT_ERR_ARG, "eps NaN");
        bad = rec; bad.struct_size = 20;
        CHECK(apt_film_compare_host(&bad, a.data(), b.data(), n, keep.data(), kmap.data()) == APT_ERR_STRUCT, "struct_size");
        bad = rec; bad.passes_b = 0;
        CHECK(apt_film_compare_host(&bad, a.data(), b.data(), n, keep.data(), kmap.data()) == APT_ERR_ARG, "passes_b 0");
        CHECK(apt_film_compare_host(&rec, a.data(), b.data(), 0, keep.data(), kmap.data()) == APT_ERR_ARG, "no pixels");
        CHECK(apt_film_compare_host(&rec, a.data(), b.data(), (1ull << 28) + 1, keep.data(), kmap.data()) == APT_ERR_ARG, "too many pixels");
        CHECK(apt_film_compare_host(&rec, a.data(), nullptr, n, keep.data(), kmap.data()) == APT_ERR_ARG, "null b");
        CHECK(apt_film_compare_host(&rec, a.data(), b.data(), n, nullptr, kmap.data()) == APT_ERR_ARG, "null result");
        CHECK(apt_film_compare_host(&rec, a.data(), b.data(), n, keep.data(), a.data()) == APT_ERR_ARG, "err_map == a");
        CHECK(apt_film_metrics_last_error()[0] != 0, "the refusal has a text");
        for (uint64_t w : keep) CHECK(w == 7u, "a refusal writes nothing");
        for (float v : kmap) CHECK(v == -7.0f, "a refusal leaves the map alone");
    }
    CHECK(apt_film_compare_work_doubles(0) == 0 && apt_film_compare_work_doubles(1025) == 12 && apt_film_compare_work_doubles((1ull << 22) + 1) == 6 * 4099 &&
          apt_film_compare_work_doubles((1ull << 28) + 1) == 0, "work doubles");
}

static void ssim_checks() {
    const uint32_t sizes[][2] = {{11, 11}, {11, 12}, {12, 11}, {16, 16}, {43, 27}, {75, 70}};
    apt_film_compare rec;
    CHECK(apt_film_compare_default_host(&rec, 2, 1) == APT_OK, "defaults");
    std::vector<float> w(APT_SSIM_TAPS, NAN);
    CHECK(apt_film_ssim_weights_host(w.data()) == APT_OK && apt_film_ssim_weights_host(nullptr) == APT_ERR_ARG, "weights");
    float wsum = 0.0f;
    for (int k = 0; k < APT_SSIM_TAPS; ++k) { CHECK(w[k] > 0.0f && w[k] == w[APT_SSIM_TAPS - 1 - k], "weight %d", k); wsum += w[k]; }
    CHECK(fabsf(wsum - 1.0f) < 1e-6f, "the weights sum to %g", wsum);
    for (const auto &wh : sizes) {
        const uint32_t W = wh[0], H = wh[1];
        const size_t n = (size_t)W * H, windows = (size_t)(W - 10) * (H - 10);
        std::vector<float> a(3 * n), b(3 * n), map(windows, NAN);
        for (size_t i = 0; i < 3 * n; ++i) { b[i] = 1.2f * rnd(); a[i] = 2.0f * (b[i] + 0.2f * (rnd() - 0.5f)); }
        if (n > 200) { a[7] = NAN; b[n + 9] = INFINITY; a[2 * n + 11] = -INFINITY; a[n - 1] = 4e18f; }   // clip01 takes them all: s stays finite
        std::vector<uint64_t> res(APT_SSIM_WORDS, 0xDEADBEEFull);
        CHECK(apt_film_ssim_host(&rec, a.data(), b.data(), W, H, res.data(), map.data()) == APT_OK, "ssim %ux%u", W, H);
        CHECK(res[1] == windows, "windows");
        double sum = 0.0;
        for (size_t j = 0; j < windows; ++j) { CHECK(map[j] > -1.0f && map[j] <= 1.0f, "map[%zu] = %g", j, map[j]); sum += map[j]; }
        CHECK(fabs(as_double(res[0]) - sum) <= 1e-9 * windows, "the tree sum %g against a sequential one %g", as_double(res[0]), sum);
        std::vector<uint64_t> res2(APT_SSIM_WORDS);
        CHECK(apt_film_ssim_host(&rec, a.data(), b.data(), W, H, res2.data(), nullptr) == APT_OK && res2 == res, "without a map");
        // an image against itself: 1 in every window
        apt_film_compare same = rec;
        same.passes_b = same.passes_a;
        std::vector<float> c(b);
        CHECK(apt_film_ssim_host(&same, b.data(), c.data(), W, H, res2.data(), map.data()) == APT_OK, "b against b");
        for (size_t j = 0; j < windows; ++j) CHECK(map[j] == 1.0f, "identical images: map[%zu] = %g", j, map[j]);
        CHECK(as_double(res2[0]) == (double)windows, "identical images: the sum");
        // refusals: nothing written
        std::vector<uint64_t> keep(APT_SSIM_WORDS, 7u);
        std::vector<float> kmap(windows, -7.0f);
        CHECK(apt_film_ssim_host(&rec, a.data(), b.data(), 10, H, keep.data(), kmap.data()) == APT_ERR_ARG, "width 10");
        CHECK(apt_film_ssim_host(&rec, a.data(), b.data(), W, 10, keep.data(), kmap.data()) == APT_ERR_ARG, "height 10");
        apt_film_compare bad = rec;
        bad.exposure = INFINITY;
        CHECK(apt_film_ssim_host(&bad, a.data(), b.data(), W, H, keep.data(), kmap.data()) == APT_ERR_ARG, "exposure inf");
        bad = rec; bad.struct_size = 28;
        CHECK(apt_film_ssim_host(&bad, a.data(), b.data(), W, H, keep.data(), kmap.data()) == APT_ERR_STRUCT, "struct_size");
        CHECK(apt_film_ssim_host(&rec, nullptr, b.data(), W, H, keep.data(), kmap.data()) == APT_ERR_ARG, "null a");
        CHECK(apt_film_ssim_host(&rec, a.data(), b.data(), W, H, keep.data(), b.data()) == APT_ERR_ARG, "ssim_map == b");
        CHECK(apt_film_metrics_last_error()[0] != 0, "the refusal has a text");
        for (uint64_t v : keep) CHECK(v == 7u, "a refusal writes nothing");
        for (float v : kmap) CHECK(v == -7.0f, "a refusal leaves the map alone");
    }
    CHECK(apt_film_ssim_work_bytes(10, 11) == 0 && apt_film_ssim_work_bytes(11, 11) == 32 && apt_film_ssim_work_bytes(75, 70) == 32 + 4 * 3900, "work bytes");
}

int main() {
    compare_checks();
    ssim_checks();
    printf("ok %ld\n", g_checks);
    return 0;
}
