// film_driver.cpp -- CPU sanitizer driver for the film's host code (include/render_mi355x.h "film"; tests/test_film_sanitizers.py builds
// it with -fsanitize=address,undefined together with csrc/host_helpers.cpp; no GPU, no HIP): apt_film_curve_host, apt_film_resolve_host on
// ragged sizes with the 8-bit image at every byte offset inside exactly sized heap blocks, and apt_write_pfm.  What it computes is also
// CHECKED.  Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <limits>
#include <vector>

#include "../../include/render_mi355x.h"

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

int main(int argc, char **argv) {
    float table[2][256];
    for (uint32_t curve = 0; curve < 2; ++curve) {
        CHECK(apt_film_curve_host(curve, table[curve]) == APT_OK, "curve %u", curve);
        CHECK(table[curve][0] == 0.0f, "curve %u: table[0]", curve);
        for (int k = 1; k < 256; ++k) CHECK(table[curve][k] > table[curve][k - 1] && table[curve][k] < 1.0f, "curve %u: entry %d", curve, k);
    }
    CHECK(apt_film_curve_host(2, table[0]) == APT_ERR_ARG && apt_film_curve_host(0, nullptr) == APT_ERR_ARG, "curve refusals");
    CHECK(apt_film_curve_host(APT_CURVE_LINEAR, table[0]) == APT_OK, "curve 0 again");

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> pool = {0.0f, -0.0f, -1.0f, nan, inf, -inf, 1e-42f, 1.0f, 0.5f, 3.0f, 1e30f, 3.4e38f};
    for (int k = 0; k < 256; ++k) { pool.push_back(table[1][k]); pool.push_back(nextafterf(table[1][k], 2.0f)); pool.push_back(nextafterf(table[1][k], -1.0f)); }
    const uint64_t counts[] = {1, 2, 3, 5, 64, 257};
    for (uint64_t n : counts)
        for (uint32_t tm = 0; tm < 2; ++tm)
            for (uint32_t off = 0; off < 4; ++off) {
                std::vector<float> film(3 * n), out(3 * n, -7.0f);          // exactly sized: a stray access is ASan's to see
                for (uint64_t i = 0; i < 3 * n; ++i) film[i] = pool[(i * 7 + n + off) % pool.size()];
                std::vector<uint8_t> u8(off + 3 * n, 0xA5);
                apt_film_resolve r = {sizeof(apt_film_resolve), 1, tm, 0, 1.0f, tm ? 0.0625f : 0.0f};
                CHECK(apt_film_resolve_host(&r, film.data(), n, table[tm], out.data(), u8.data() + off) == APT_OK, "resolve n=%llu", (unsigned long long)n);
                for (uint32_t b = 0; b < off; ++b) CHECK(u8[b] == 0xA5, "bytes before the image");
                for (uint64_t i = 0; i < n; ++i)
                    for (uint64_t c = 0; c < 3; ++c) {
                        const float y = out[c * n + i];
                        CHECK(y >= 0.0f && y <= 1.0f, "y in [0, 1]");
                        uint32_t code = 0;
                        for (int k = 1; k < 256; ++k) code += table[tm][k] <= y;
                        CHECK(u8[off + i * 3 + c] == code, "code of %g: %u, want %u", y, u8[off + i * 3 + c], code);
                        if (tm == 0) {
                            const float s = film[c * n + i];
                            CHECK(y == (s > 0.0f ? (s < 1.0f ? s : 1.0f) : 0.0f), "clip of %g", s);
                        }
                    }
                // one output at a time, and the refusals write nothing
                CHECK(apt_film_resolve_host(&r, film.data(), n, table[tm], nullptr, u8.data() + off) == APT_OK, "u8 only");
                CHECK(apt_film_resolve_host(&r, film.data(), n, table[tm], out.data(), nullptr) == APT_OK, "out only");
                CHECK(apt_film_resolve_host(&r, film.data(), n, table[tm], nullptr, nullptr) == APT_ERR_ARG, "no output");
                r.passes = 0;
                CHECK(apt_film_resolve_host(&r, film.data(), n, table[tm], out.data(), nullptr) == APT_ERR_ARG, "passes 0");
            }

    const char *path = argc > 1 ? argv[1] : "film_driver.pfm";
    const float planes[18] = {0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25};   // [3][3 * 2]
    CHECK(apt_write_pfm(path, 3, 2, planes) == APT_OK, "write_pfm");
    FILE *f = fopen(path, "rb");
    CHECK(f != nullptr, "reopen");
    char buf[128];
    const size_t got = fread(buf, 1, sizeof buf, f);
    fclose(f);
    CHECK(got == 12 + 72 && memcmp(buf, "PF\n3 2\n-1.0\n", 12) == 0, "pfm size %zu", got);
    float px[18];
    memcpy(px, buf + 12, 72);
    for (int y = 0; y < 2; ++y)
        for (int x = 0; x < 3; ++x)
            for (int c = 0; c < 3; ++c) CHECK(px[(y * 3 + x) * 3 + c] == planes[c * 6 + x * 2 + y], "pfm pixel");
    CHECK(apt_write_pfm(nullptr, 3, 2, planes) == APT_ERR_ARG && apt_write_pfm(path, 0, 2, planes) == APT_ERR_ARG, "pfm refusals");
    remove(path);
    printf("ok %ld\n", g_checks);
    return 0;
}
