// history_driver.cpp -- CPU sanitizer driver for the host code of temporal accumulation (include/render_mi355x_history.h;
// tests/test_film_stage_sanitizers.py builds it with -fsanitize=address,undefined together with csrc/history_host.cpp and csrc/film_stage_host.cpp; no GPU, no HIP):
// apt_film_history_host and apt_film_history_export_host on the sizes of the CPU test, every buffer an exactly sized heap block (a
// stray access is ASan's to see), with cameras that send taps outside the previous image, behind it and onto NaN and zero-coverage
// pixels.  What it computes is also CHECKED.
// Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/render_mi355x_history.h"

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static float rnd() {                                       // splitmix64 -> [0, 1)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (float)((z ^ (z >> 31)) >> 40) * (1.0f / 16777216.0f);
}

// a pinhole at `eye` looking along -z with the image plane axes x and y: mutually orthogonal, as the library's builders make them
static apt_camera camera(double ex, double ey, double ez, double yaw) {
    apt_camera c;
    memset(&c, 0, sizeof c);
    c.struct_size = sizeof c;
    c.pos[0] = ex; c.pos[1] = ey; c.pos[2] = ez;
    c.g[0] = sin(yaw); c.g[2] = -cos(yaw);
    c.cx[0] = 1.2 * cos(yaw); c.cx[2] = 1.2 * sin(yaw);
    c.cy[1] = 0.8;
    return c;
}

// the planes of the wall z = 0 (normal +z) seen by camera c: depth = the distance along the pixel centre's ray
static void wall(const apt_camera &c, uint32_t w, uint32_t h, std::vector<float> &f) {
    const size_t n = (size_t)w * h;
    f.assign(8 * n, 0.0f);
    for (uint32_t x = 0; x < w; ++x)
        for (uint32_t y = 0; y < h; ++y) {
            const size_t i = (size_t)x * h + y;
            const double a = (x + 0.5) / w - 0.5, b = (y + 0.5) / h - 0.5;
            double d[3];
            for (int k = 0; k < 3; ++k) d[k] = c.cx[k] * a + c.cy[k] * b + c.g[k];
            const double len = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const double t = -c.pos[2] / (d[2] / len);
            if (!(t > 0)) continue;                                          // looking away: a miss, all planes 0
            const float cov = i % 7 == 3 ? 0.0f : (i % 5 == 1 ? 0.5f + 0.5f * rnd() : 1.0f);
            f[i] = cov; f[n + i] = (float)t * cov; f[4 * n + i] = cov;       // normal (0, 0, 1) * cov
            for (int k = 5; k < 8; ++k) f[k * n + i] = rnd() * cov;
        }
}

int main() {
    const uint32_t sizes[][2] = {{1, 1}, {1, 7}, {7, 1}, {5, 3}, {33, 17}, {48, 32}};
    apt_film_history rec;
    CHECK(apt_film_history_default_host(&rec) == APT_OK && rec.struct_size == sizeof rec && rec.max_history == 32, "defaults");
    CHECK(apt_film_history_default_host(nullptr) == APT_ERR_ARG, "null record");
    for (const auto &wh : sizes) {
        const uint32_t w = wh[0], h = wh[1];
        const size_t n = (size_t)w * h;
        const apt_camera cur = camera(0.0, 0.0, 100.0, 0.0);
        const apt_camera prevs[] = {cur, camera(4.0, -3.0, 95.0, 0.0), camera(0.0, 0.0, 100.0, 0.5), camera(0.0, 0.0, -100.0, 0.0)};
        std::vector<float> cf, pf;
        wall(cur, w, h, cf);
        for (int which = 0; which < 4; ++which) {
            const apt_camera &prev = prevs[which];
            wall(prev, w, h, pf);
            std::vector<float> c3(3 * n), hist(6 * n), out(6 * n, NAN);
            for (float &v : c3) v = 2.0f * rnd();
            for (size_t i = 0; i < n; ++i) {
                for (int k = 0; k < 5; ++k) hist[k * n + i] = 2.0f * rnd();
                hist[5 * n + i] = i % 6 == 2 ? 0.5f : (float)(1 + i % 40);
            }
            if (n > 4) { hist[5 * n + 4] = NAN; pf[n + 3] = NAN; cf[1] = NAN; }
            if (which == 3) {                                               // the previous camera stands behind the wall, looking away from
                for (size_t i = 0; i < n; ++i) { pf[i] = 1.0f; pf[n + i] = 50.0f; pf[4 * n + i] = 1.0f; }   // it: valid planes, but f <= 0
            }
            CHECK(apt_film_history_host(&rec, &cur, &prev, c3.data(), cf.data(), pf.data(), hist.data(), w, h, out.data()) == APT_OK, "history %ux%u/%d", w, h, which);
            size_t valid = 0;
            for (size_t i = 0; i < n; ++i) {
                const float len = out[5 * n + i];
                CHECK(len >= 1.0f && len <= 32.0f, "length of pixel %zu", i);
                if (len == 1.0f) { CHECK(out[i] == c3[i] && out[2 * n + i] == c3[2 * n + i], "a reset pixel holds the current frame"); }
                else ++valid;
                if (cf[i] == 0.0f || which == 3) CHECK(len == 1.0f, "pixel %zu must be a reset", i);
            }
            if (which == 0 && n >= 15) CHECK(valid > n / 3, "the same camera keeps most pixels: %zu of %zu", valid, n);
            if (which == 1 && n >= 500) CHECK(valid > n / 4, "a small move keeps many pixels: %zu of %zu", valid, n);

            // the first frame: nothing of the previous frame is read
            std::vector<float> first(6 * n, NAN);
            CHECK(apt_film_history_host(&rec, &cur, nullptr, c3.data(), cf.data(), nullptr, nullptr, w, h, first.data()) == APT_OK, "first frame");
            for (size_t i = 0; i < n; ++i) CHECK(first[5 * n + i] == 1.0f && first[n + i] == c3[n + i], "first frame pixel %zu", i);

            // the export on exactly sized planes
            std::vector<float> film(3 * n, NAN), mom(2 * n, NAN);
            CHECK(apt_film_history_export_host(out.data(), n, film.data(), mom.data()) == APT_OK, "export");
            for (size_t i = 0; i < n; ++i) {
                CHECK(film[n + i] == out[n + i] + out[n + i] || isnan(out[n + i]), "film of pixel %zu", i);
                CHECK(mom[i] == out[3 * n + i] + out[3 * n + i] || isnan(out[3 * n + i]), "m0 of pixel %zu", i);
            }
            CHECK(apt_film_history_export_host(out.data(), 0, film.data(), mom.data()) == APT_ERR_ARG, "no pixels");
            CHECK(apt_film_history_export_host(nullptr, n, film.data(), mom.data()) == APT_ERR_ARG, "null hist");

            // refusals: nothing written
            std::vector<float> keep(6 * n, -7.0f);
            apt_film_history bad = rec;
            bad.min_weight = 0.0f;
            CHECK(apt_film_history_host(&bad, &cur, &prev, c3.data(), cf.data(), pf.data(), hist.data(), w, h, keep.data()) == APT_ERR_ARG, "min_weight 0");
            bad = rec; bad.struct_size = 20;
            CHECK(apt_film_history_host(&bad, &cur, &prev, c3.data(), cf.data(), pf.data(), hist.data(), w, h, keep.data()) == APT_ERR_STRUCT, "struct_size");
            apt_camera cam = cur;
            cam.struct_size = 8;
            CHECK(apt_film_history_host(&rec, &cam, &prev, c3.data(), cf.data(), pf.data(), hist.data(), w, h, keep.data()) == APT_ERR_STRUCT, "camera size");
            cam = prev; cam.g[0] = cam.g[1] = cam.g[2] = 0.0;
            CHECK(apt_film_history_host(&rec, &cur, &cam, c3.data(), cf.data(), pf.data(), hist.data(), w, h, keep.data()) == APT_ERR_ARG, "zero g");
            CHECK(apt_film_history_host(&rec, &cur, &prev, c3.data(), cf.data(), pf.data(), hist.data(), w, h, hist.data()) == APT_ERR_ARG, "aliased");
            CHECK(apt_film_history_host(&rec, &cur, &prev, c3.data(), cf.data(), pf.data(), hist.data(), 0, h, keep.data()) == APT_ERR_ARG, "zero width");
            CHECK(apt_film_history_last_error()[0] != 0, "the refusal has a text");
            for (float v : keep) CHECK(v == -7.0f, "a refusal writes nothing");
            wall(cur, w, h, cf);                                             // (without the NaN, for the next camera)
        }
    }
    printf("ok %ld\n", g_checks);
    return 0;
}
