// adaptive_driver.cpp -- CPU sanitizer driver for the host code of adaptive sampling (include/render_mi355x_adaptive.h;
// tests/test_film_stage_sanitizers.py builds it with -fsanitize=address,undefined together with csrc/adaptive_host.cpp and csrc/film_stage_host.cpp; no GPU, no HIP):
// apt_film_select_host, apt_film_accumulate_list_host and apt_film_mean_host on the sizes of the CPU test, every buffer an exactly sized
// heap block (a stray access is ASan's to see).  What it computes is also CHECKED.
// Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../include/render_mi355x_adaptive.h"

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
    const size_t sizes[] = {1, 63, 64, 65, 255, 256, 257, 1001, 65537};
    for (const size_t n : sizes) {
        const uint32_t base = 3;
        apt_film_select s;
        CHECK(apt_film_select_default_host(&s, base) == APT_OK && s.struct_size == sizeof s && s.base_passes == base, "defaults");
        s.min_passes = 4; s.max_passes = 9; s.threshold = 0.125f; s.floor = 0.25f;
        std::vector<float> film(3 * n), mom(2 * n);
        std::vector<uint32_t> extra(n), list(n, 0xDEADBEEFu), work(apt_film_select_work_words(n), 0xDEADBEEFu);
        CHECK(work.size() == (n + 255) / 256, "work words");
        for (size_t i = 0; i < n; ++i) {
            extra[i] = (uint32_t)(i % 8);                                  // n_u = 3 .. 10: below min_passes, inside, at and above max_passes
            const float nu = (float)(base + extra[i]), lm = 0.5f + rnd();
            mom[i] = lm * nu;
            mom[n + i] = lm * lm * nu * (i % 3 == 0 ? 3.0f : 0.5f);        // loud or quiet
            if (i % 11 == 5) mom[i] = NAN;
            for (size_t c = 0; c < 3; ++c) film[c * n + i] = 4.0f * rnd();
        }
        uint32_t *count = new uint32_t(0xDEADBEEFu);
        CHECK(apt_film_select_host(&s, mom.data(), extra.data(), n, work.data(), list.data(), count) == APT_OK, "select %zu", n);
        const uint32_t k = *count;
        CHECK(k <= n, "count");
        size_t expect = 0;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t nu = base + extra[i];
            const bool must = nu < 4 || (nu < 9 && i % 3 == 0 && i % 11 != 5), never = nu >= 9 || (nu >= 4 && (i % 11 == 5 || i % 3 != 0));
            const bool in = expect < k && list[expect] == i;
            CHECK(!(must && !in) && !(never && in), "pixel %zu of %zu", i, n);
            if (in) ++expect;
        }
        CHECK(expect == k, "the list is ascending and holds nothing else");
        for (size_t i = k; i < n; ++i) CHECK(list[i] == 0xDEADBEEFu, "list words from count on are not written");
        for (uint32_t w : work) CHECK(w == 0xDEADBEEFu, "the twin does not touch work");

        // a list pass on exactly sized planes, with entries beyond the image in it
        std::vector<uint32_t> lst(list.begin(), list.begin() + k);
        if (k >= 2) { lst[k / 2] = (uint32_t)n; lst[k - 1] = 0xFFFFFFFFu; }
        std::vector<float> planes(3 * (size_t)k), film0 = film, mom0 = mom;
        std::vector<uint32_t> extra0 = extra;
        for (float &v : planes) v = 2.0f * rnd();
        CHECK(apt_film_accumulate_list_host(planes.data(), lst.data(), k, n, film.data(), mom.data(), extra.data()) == APT_OK, "accumulate");
        size_t added = 0;
        for (size_t i = 0; i < k; ++i) {
            const size_t p = lst[i];
            if (p >= n) continue;
            ++added;
            CHECK(extra[p] == extra0[p] + 1 && film[p] == film0[p] + planes[i] && film[2 * n + p] == film0[2 * n + p] + planes[2 * (size_t)k + i], "entry %zu", i);
        }
        size_t changed = 0;
        for (size_t i = 0; i < n; ++i) changed += extra[i] != extra0[i];
        CHECK(changed == added, "only the listed pixels inside the image change");
        CHECK(apt_film_accumulate_list_host(planes.data(), lst.data(), n + 1, n, film.data(), mom.data(), extra.data()) == APT_ERR_ARG, "list_count > N");
        CHECK(apt_film_accumulate_list_host(nullptr, lst.data(), k, n, film.data(), mom.data(), extra.data()) == APT_ERR_ARG, "null planes");
        CHECK(apt_film_accumulate_list_host(planes.data(), lst.data(), 0, n, film.data(), mom.data(), extra.data()) == APT_OK, "empty list");

        std::vector<float> out(3 * n, -7.0f);
        CHECK(apt_film_mean_host(film.data(), extra.data(), base, n, out.data()) == APT_OK, "mean");
        for (size_t i = 0; i < n; ++i) CHECK(out[n + i] == film[n + i] / (float)(base + extra[i]), "mean of pixel %zu", i);
        CHECK(apt_film_mean_host(film.data(), nullptr, base, n, out.data()) == APT_OK && out[0] == film[0] / 3.0f, "mean without extra");
        CHECK(apt_film_mean_host(film.data(), nullptr, 1, n, out.data()) == APT_ERR_ARG, "base 1");

        s.min_passes = 1;
        CHECK(apt_film_select_host(&s, mom.data(), extra.data(), n, work.data(), list.data(), count) == APT_ERR_ARG && *count == k, "min_passes 1");
        s.min_passes = 4; s.struct_size = 20;
        CHECK(apt_film_select_host(&s, mom.data(), extra.data(), n, work.data(), list.data(), count) == APT_ERR_STRUCT, "struct_size");
        CHECK(apt_film_adaptive_last_error()[0] != 0, "the refusal has a text");
        delete count;
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
