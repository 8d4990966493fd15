// denoise_driver.cpp -- CPU sanitizer driver for the host code of the film's moments and its filter (include/render_mi355x_denoise.h;
// tests/test_film_stage_sanitizers.py builds it with -fsanitize=address,undefined together with csrc/denoise_host.cpp and csrc/film_stage_host.cpp; no GPU, no HIP):
// apt_film_accumulate_host and apt_film_denoise_host on the small shapes of the CPU test, every buffer an exactly sized heap block
// (a stray access is ASan's to see) and guard floats round `work` and `out` inside theirs.  What it computes is also CHECKED.
// Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/render_mi355x_denoise.h"

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static float rnd() {                                       // splitmix64 -> [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (float)((z ^ (z >> 31)) >> 40) * (1.0f / 16777216.0f);
}

int main() {
    const uint32_t shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 3}, {33, 17}, {40, 70}};
    const size_t G = 8;                                    // guard floats: work stays 16-byte aligned behind them
    for (const auto &sh : shapes) {
        const uint32_t W = sh[0], H = sh[1], K = 3;
        const size_t n = (size_t)W * H;
        std::vector<float> film(3 * n, NAN), mom(2 * n, NAN), feat(8 * n), pass(3 * n), sum(3 * n, 0.0f);
        for (size_t i = 0; i < n; ++i) {
            const float cov = i % 3 == 0 ? 1.0f : (i % 3 == 1 ? rnd() : 0.0f);
            feat[i] = cov;
            feat[n + i] = cov * (50.0f + 100.0f * rnd());
            for (size_t c = 0; c < 3; ++c) feat[(2 + c) * n + i] = cov * (rnd() - 0.5f);
            for (size_t c = 0; c < 3; ++c) feat[(5 + c) * n + i] = i % 5 == 2 ? 0.0f : cov * rnd();      // some albedo-0 pixels
        }
        for (uint32_t k = 0; k < K; ++k) {
            for (size_t i = 0; i < 3 * n; ++i) { pass[i] = 2.0f * rnd(); sum[i] = k ? sum[i] + pass[i] : pass[i]; }
            CHECK(apt_film_accumulate_host(pass.data(), n, film.data(), mom.data(), k) == APT_OK, "accumulate %ux%u pass %u", W, H, k);
        }
        for (size_t i = 0; i < 3 * n; ++i) CHECK(film[i] == sum[i], "the film is the sequential sum");
        for (size_t i = 0; i < n; ++i) CHECK(mom[i] > 0.0f && mom[n + i] > 0.0f && K * mom[n + i] >= mom[i] * mom[i] * 0.999f, "moments of pixel %zu", i);
        CHECK(apt_film_accumulate_host(pass.data(), 0, film.data(), mom.data(), 1) == APT_OK, "empty");
        CHECK(apt_film_accumulate_host(nullptr, n, film.data(), mom.data(), 1) == APT_ERR_ARG, "null pass");

        CHECK(apt_film_denoise_work_floats(W, H) == 16 * n, "work floats");
        float *work_block = static_cast<float *>(aligned_alloc(16, (16 * n + 2 * G) * sizeof(float)));
        std::vector<float> out_block(3 * n + 2 * G, -7.0f);
        for (uint32_t it = 1; it <= 5; ++it) {
            for (size_t i = 0; i < 16 * n + 2 * G; ++i) work_block[i] = -7.0f;
            for (float &v : out_block) v = -7.0f;
            apt_film_denoise d;
            CHECK(apt_film_denoise_default_host(&d, K) == APT_OK && d.iterations == 5 && d.struct_size == sizeof d, "defaults");
            d.iterations = it;
            float *work = work_block + G, *out = out_block.data() + G;
            CHECK(apt_film_denoise_host(&d, film.data(), mom.data(), feat.data(), W, H, work, out) == APT_OK, "denoise %ux%u", W, H);
            for (size_t g = 0; g < G; ++g)
                CHECK(work_block[g] == -7.0f && work_block[G + 16 * n + g] == -7.0f && out_block[g] == -7.0f && out_block[G + 3 * n + g] == -7.0f, "guards");
            // every iteration is a weighted mean of non-negative illumination, and the albedo is at most 1 (a miss): the result is finite,
            // not negative, and no brighter than the brightest illumination in c[0] -- prepare's, the last iteration's input or its
            // result, whichever `it` leaves there -- with room for the roundings
            float top = 0.0f;
            for (size_t i = 0; i < n; ++i) top = fmaxf(top, fmaxf(work[8 * n + 4 * i], fmaxf(work[8 * n + 4 * i + 1], work[8 * n + 4 * i + 2])));
            for (size_t i = 0; i < 3 * n; ++i) CHECK(isfinite(out[i]) && out[i] >= 0.0f && out[i] <= top * 1.001f, "out[%zu] = %g", i, out[i]);
            d.iterations = 6;
            CHECK(apt_film_denoise_host(&d, film.data(), mom.data(), feat.data(), W, H, work, out) == APT_ERR_ARG, "iterations 6");
            d.iterations = it; d.passes = 1;
            CHECK(apt_film_denoise_host(&d, film.data(), mom.data(), feat.data(), W, H, work, out) == APT_ERR_ARG, "passes 1");
            d.passes = K;
            CHECK(apt_film_denoise_host(&d, film.data(), mom.data(), feat.data(), W, H, work + 1, out) == APT_ERR_ARG, "misaligned work");
            CHECK(apt_film_denoise_host(&d, film.data(), mom.data(), feat.data(), W, H, nullptr, out) == APT_ERR_ARG, "null work");
        }
        free(work_block);
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
