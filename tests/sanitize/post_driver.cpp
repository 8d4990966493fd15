// post_driver.cpp -- CPU sanitizer driver for the host code of metering and bloom (include/render_mi355x_post.h;
// tests/test_film_stage_sanitizers.py builds it with -fsanitize=address,undefined together with csrc/post_host.cpp and csrc/film_stage_host.cpp; no GPU, no HIP):
// apt_film_meter_host, apt_film_exposure_host and apt_film_bloom_host on the sizes of the CPU test, every buffer an exactly sized
// heap block (a stray access is ASan's to see), with NaN, infinite, negative and subnormal pixels in the films.  What it computes is
// also CHECKED.
// Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/render_mi355x_post.h"

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static float rnd() {                                       // splitmix64 -> [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (float)((z ^ (z >> 31)) >> 40) * (1.0f / 16777216.0f);
}

// work must be 16-byte aligned AND exactly sized: the block is posix_memalign's, of exactly the bytes asked for
struct Aligned {
    float *p = nullptr;
    explicit Aligned(size_t floats) {
        void *v = nullptr;
        if (posix_memalign(&v, 16, floats * sizeof(float)) != 0) { fprintf(stderr, "posix_memalign failed\n"); exit(1); }
        p = static_cast<float *>(v);
        for (size_t i = 0; i < floats; ++i) p[i] = NAN;
    }
    ~Aligned() { free(p); }
    Aligned(const Aligned &) = delete;
    Aligned &operator=(const Aligned &) = delete;
};

static void meter_checks() {
    const uint64_t sizes[] = {0, 1, 63, 64, 65, 257, 1001};
    apt_film_meter rec;
    CHECK(apt_film_meter_default_host(&rec, 3) == APT_OK && rec.struct_size == sizeof rec && rec.passes == 3 && rec.low_q == 6554, "defaults");
    CHECK(apt_film_meter_default_host(nullptr, 3) == APT_ERR_ARG && apt_film_meter_default_host(&rec, 0) == APT_ERR_ARG, "refused defaults");
    CHECK(apt_film_meter_default_host(&rec, 3) == APT_OK, "defaults again");
    const float specials[] = {NAN, INFINITY, -INFINITY, -2.0f, 0.0f, -0.0f, 1e-40f, 3e38f, 1.52587890625e-05f, 65536.0f};
    for (uint64_t n : sizes) {
        std::vector<float> film(3 * n);
        for (uint64_t i = 0; i < n; ++i) {
            const float s = exp2f(40.0f * rnd() - 20.0f);
            for (int ch = 0; ch < 3; ++ch) film[ch * n + i] = i % 5 == 2 ? specials[(i / 5 + ch * (i % 3 == 0)) % 10] : 3.0f * s * (0.5f + rnd());
        }
        std::vector<uint32_t> hist(APT_METER_WORDS, 0xDEADBEEFu);
        CHECK(apt_film_meter_host(&rec, n ? film.data() : nullptr, n, hist.data()) == APT_OK, "meter of %llu", (unsigned long long)n);
        uint64_t sum = 0;
        for (uint32_t w : hist) sum += w;
        CHECK(sum == n, "the words sum to %llu, not %llu", (unsigned long long)sum, (unsigned long long)n);
        // two bands add to the whole
        if (n > 2) {
            const uint64_t cut = n / 3;
            std::vector<float> a(3 * cut), b(3 * (n - cut));
            for (int ch = 0; ch < 3; ++ch) {
                memcpy(a.data() + ch * cut, film.data() + ch * n, cut * sizeof(float));
                memcpy(b.data() + ch * (n - cut), film.data() + ch * n + cut, (n - cut) * sizeof(float));
            }
            std::vector<uint32_t> ha(APT_METER_WORDS), hb(APT_METER_WORDS);
            CHECK(apt_film_meter_host(&rec, a.data(), cut, ha.data()) == APT_OK && apt_film_meter_host(&rec, b.data(), n - cut, hb.data()) == APT_OK, "bands");
            for (int k = 0; k < APT_METER_WORDS; ++k) CHECK(ha[k] + hb[k] == hist[k], "band sum of word %d", k);
        }
        // the exposure from it, on an exactly sized histogram
        for (float adapt : {1.0f, 0.25f, 0.0f}) {
            apt_film_meter r = rec;
            r.adapt = adapt;
            float e = -7.0f;
            CHECK(apt_film_exposure_host(&r, hist.data(), 2.0f, &e) == APT_OK, "exposure");
            CHECK(e >= (adapt >= 1.0f ? r.min_exposure : 0.0f) && e <= r.max_exposure, "exposure %g in range", e);
            if (adapt == 0.0f || n == 0) CHECK(e == 2.0f, "the exposure stays at prev, got %g", e);
        }
        // refusals: nothing written
        std::vector<uint32_t> keep(APT_METER_WORDS, 7u);
        float e = -7.0f;
        apt_film_meter bad = rec;
        bad.low_q = 0;
        CHECK(apt_film_meter_host(&bad, film.data(), n, keep.data()) == APT_ERR_ARG && apt_film_exposure_host(&bad, hist.data(), 1.0f, &e) == APT_ERR_ARG, "low_q 0");
        bad = rec; bad.struct_size = 28;
        CHECK(apt_film_meter_host(&bad, film.data(), n, keep.data()) == APT_ERR_STRUCT, "struct_size");
        bad = rec; bad.key = NAN;
        CHECK(apt_film_meter_host(&bad, film.data(), n, keep.data()) == APT_ERR_ARG, "key NaN");
        bad = rec; bad.min_exposure = 9.0f; bad.max_exposure = 8.0f;
        CHECK(apt_film_exposure_host(&bad, hist.data(), 1.0f, &e) == APT_ERR_ARG, "min > max");
        CHECK(apt_film_exposure_host(&rec, hist.data(), NAN, &e) == APT_ERR_ARG && apt_film_exposure_host(&rec, hist.data(), -1.0f, &e) == APT_ERR_ARG, "prev");
        CHECK(apt_film_meter_host(&rec, film.data(), (1ull << 28) + 1, keep.data()) == APT_ERR_ARG, "too many pixels");
        CHECK(apt_film_post_last_error()[0] != 0, "the refusal has a text");
        for (uint32_t w : keep) CHECK(w == 7u, "a refusal writes nothing");
        CHECK(e == -7.0f, "a refused exposure writes nothing");
    }
    // a histogram of the largest counts: the selection's 64-bit arithmetic
    std::vector<uint32_t> full(APT_METER_WORDS, 0xFFFFFFFFu);
    float e = 0.0f;
    CHECK(apt_film_exposure_host(&rec, full.data(), 1.0f, &e) == APT_OK && e > 0.0f, "full histogram");
    CHECK(apt_film_meter_work_words(0) == 0 && apt_film_meter_work_words(1025) == 2 * APT_METER_WORDS && apt_film_meter_work_words(1ull << 28) == 512 * APT_METER_WORDS, "work words");
}

static void bloom_checks() {
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 3}, {33, 17}, {64, 48}};
    apt_film_bloom rec;
    CHECK(apt_film_bloom_default_host(&rec, 2) == APT_OK && rec.struct_size == sizeof rec && rec.levels == 5 && rec.passes == 2, "defaults");
    CHECK(apt_film_bloom_default_host(nullptr, 2) == APT_ERR_ARG, "null record");
    for (const auto &wh : sizes) {
        const uint32_t w = wh[0], h = wh[1];
        const size_t n = (size_t)w * h;
        for (uint32_t levels : {1u, 2u, 6u}) {
            rec.levels = levels;
            std::vector<float> film(3 * n), out(3 * n, NAN);
            for (float &v : film) v = rnd() < 0.15f ? 80.0f * rnd() : 1.8f * rnd();
            if (n > 4) { film[1] = NAN; film[n + 2] = INFINITY; film[2 * n + 3] = -5.0f; film[n - 1] = INFINITY; film[2 * n - 1] = NAN; }
            const uint64_t floats = apt_film_bloom_work_floats(w, h, levels);
            CHECK(floats >= 4 && floats % 4 == 0, "work floats %llu", (unsigned long long)floats);
            Aligned work(floats);
            CHECK(apt_film_bloom_host(&rec, film.data(), w, h, work.p, out.data()) == APT_OK, "bloom %ux%u/%u", w, h, levels);
            for (uint64_t i = 0; i < floats; ++i) CHECK(work.p[i] >= 0.0f && isfinite(work.p[i]), "work[%llu] = %g", (unsigned long long)i, work.p[i]);
            for (size_t i = 0; i < 3 * n; ++i) {
                const float m = film[i] / 2.0f;
                if (isnan(m)) { CHECK(isnan(out[i]), "a NaN stays in its pixel %zu", i); continue; }
                CHECK(!isnan(out[i]) && out[i] >= m, "out[%zu] = %g below the mean %g", i, out[i], m);
            }
            // below the threshold: the mean itself
            std::vector<float> dark(3 * n), same(3 * n, NAN);
            for (float &v : dark) v = 1.9f * rnd();
            CHECK(apt_film_bloom_host(&rec, dark.data(), w, h, work.p, same.data()) == APT_OK, "dark film");
            for (size_t i = 0; i < 3 * n; ++i) CHECK(same[i] == dark[i] / 2.0f, "dark pixel %zu", i);

            // refusals: nothing written
            std::vector<float> keep(3 * n, -7.0f);
            Aligned kwork(floats);
            apt_film_bloom bad = rec;
            bad.levels = 7;
            CHECK(apt_film_bloom_host(&bad, film.data(), w, h, kwork.p, keep.data()) == APT_ERR_ARG, "levels 7");
            bad = rec; bad.struct_size = 28;
            CHECK(apt_film_bloom_host(&bad, film.data(), w, h, kwork.p, keep.data()) == APT_ERR_STRUCT, "struct_size");
            bad = rec; bad.cap = INFINITY;
            CHECK(apt_film_bloom_host(&bad, film.data(), w, h, kwork.p, keep.data()) == APT_ERR_ARG, "cap inf");
            bad = rec; bad.threshold = -1.0f;
            CHECK(apt_film_bloom_host(&bad, film.data(), w, h, kwork.p, keep.data()) == APT_ERR_ARG, "threshold < 0");
            CHECK(apt_film_bloom_host(&rec, film.data(), 0, h, kwork.p, keep.data()) == APT_ERR_ARG, "zero width");
            CHECK(apt_film_bloom_host(&rec, film.data(), w, h, kwork.p, film.data()) == APT_ERR_ARG, "aliased");
            CHECK(apt_film_bloom_host(&rec, film.data(), w, h, nullptr, keep.data()) == APT_ERR_ARG, "null work");
            CHECK(apt_film_bloom_host(&rec, film.data(), w, h, kwork.p + 1, keep.data()) == APT_ERR_ARG, "misaligned work");
            CHECK(apt_film_post_last_error()[0] != 0, "the refusal has a text");
            for (float v : keep) CHECK(v == -7.0f, "a refusal writes nothing");
            for (uint64_t i = 0; i < floats; ++i) CHECK(isnan(kwork.p[i]), "a refusal leaves work alone");
        }
    }
    CHECK(apt_film_bloom_work_floats(0, 1, 1) == 0 && apt_film_bloom_work_floats(1, 1, 7) == 0 && apt_film_bloom_work_floats(33, 17, 6) == 4 * 222, "work floats");
}

int main() {
    meter_checks();
    bloom_checks();
    printf("ok %ld\n", g_checks);
    return 0;
}
