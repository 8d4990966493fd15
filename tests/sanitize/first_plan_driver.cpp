// first_plan_driver.cpp -- CPU sanitizer driver for the CPU twin of the first-bounce plan (csrc/first_plan_host.cpp with the text it shares
// with the kernels, csrc/pt_first_plan.h; tests/test_film_stage_sanitizers.py builds the two together with -fsanitize=address,undefined;
// no GPU, no HIP): apt_first_plan_host, apt_first_plan_camera_host and apt_first_plan_mask_host at the edge shapes (1 x 1, one row, one
// column, 2^24 squared, beyond 2^24, 2^32 - 1 squared), at tables of the test family written out as numbers, at every refusing premise
// and at non-finite entries, every buffer an exactly sized heap block (a stray access is ASan's to see).  What it computes is also
// CHECKED: the record's invariants, the records of the family members (as the product build of the twin gave them), the record of the
// headline frame, and the mask against a statement of the header's table.
// Prints "ok <checks>" and exits 0; a failed check prints what failed and exits 1; a sanitizer report aborts.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

extern "C" {
int apt_first_plan_host(uint32_t width, uint32_t height, const float *spheres, double eps, const double *camera12, int32_t *record16);
int apt_first_plan_camera_host(uint32_t width, uint32_t height, double *camera12);
uint32_t apt_first_plan_mask_host(const int32_t *record16, uint32_t width, uint32_t height, uint32_t col, uint32_t row);
}

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {                          // splitmix64 -> [0, n)
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)(((z ^ (z >> 31)) >> 11) % n);
}

// the reference room: radius, x, y, z of its eight spheres (the table stores r^2, rounded once)
static const double kRoom[8][4] = {{1e5, 1e5 + 1, 40.8, 81.6}, {1e5, -1e5 + 99, 40.8, 81.6}, {1e5, 50, 40.8, 1e5}, {1e5, 50, 40.8, -1e5 + 170},
                                   {1e5, 50, 1e5, 81.6}, {1e5, 50, -1e5 + 81.6, 81.6}, {16.5, 27, 16.5, 47}, {600, 50, 681.6 - .27, 81.6}};

struct Member { uint32_t w, h; double eps; double table[32]; double cam[12]; int32_t record[16]; };
static const Member kMembers[] = {
    // member 0 of the family of seed 7 (tests/first_plan_ref.py)
    {33, 19, 1.0,
     {4.62625434e+09, 5.4779689e+09, 1.43722394e+10, 2.5422999e+09, 1.33860905e+10, 1.29426012e+10, 3274.66577, 8366.51172,
      67980.8203, -73911.0312, 55.0038185, 55.0038185, 55.0038185, 55.0038185, 91.2145844, 55.0038185,
      52.7164154, 52.7164154, 52.7164154, 52.7164154, 115654.844, -113634.922, 72.1987839, 247.84761,
      98.1411438, 98.1411438, 119790.234, -50126.1523, 98.1411438, 98.1411438, 320.113708, 98.1411438},
     {50, 52, 295.60000000000002, 0, -0.042573365542992951, -0.99909334325994914, 0.89186842105263153, 0, 0, 0, 0.51303443176398389, -0.021861423206326877},
     {0, 28, 0, 19, 15, 15, 7, 10, 1, 0, 0, 0, 0, 19, 0, 0}},
    // member 1 of the family of seed 7 (tests/first_plan_ref.py)
    {64, 36, 0.0001,
     {3.94339046e+09, 7.14997197e+09, 8.12490906e+09, 1.67511224e+10, 5.55181466e+09, 5.7863895e+09, 5805.67822, 150357424,
      62756.1758, -84474.6562, 60.8056374, 60.8056374, 60.8056374, 60.8056374, 25.2147198, 60.8056374,
      29.1578178, 29.1578178, 29.1578178, 29.1578178, 74501.3516, -75879.9453, 14.7882309, -12269.2539,
      62.9458656, 62.9458656, 90115.9062, -129180.664, 62.9458656, 62.9458656, 169.275711, 62.9458656},
     {45.224424123676847, 44.836516283125512, 300.69816853224847, 0, -0.042573365542992951, -0.99909334325994914, 1.4392208360533196, 0, 0, 0, 0.36272350816552695, -0.015456374129949432},
     {7, 42, 0, 36, 31, 31, 12, 20, 1, 0, 8, 0, 0, 0, 0, 0}},
    // member 6 of the family of seed 7 (tests/first_plan_ref.py)
    {17, 31, 0.3,
     {2.5e+09, 6.94653542e+09, 1.45692283e+10, 6.46311885e+09, 2.79329587e+09, 3.62583245e+09, 46.7061348, 1155036.75,
      50004.0586, -83226.6016, 49.4026146, 49.4026146, 49.4026146, 49.4026146, 66.0093994, 49.4026146,
      43.6236687, 43.6236687, 43.6236687, 43.6236687, 52797.0586, -60095.4492, 127.718613, -16.3975677,
      102.069733, 102.069733, 120533.719, -80050.6875, 102.069733, 102.069733, -84.0564499, 102.069733},
     {44.416148638167428, 57.725454479778975, 297.14803938792858, 0, -0.042573365542992951, -0.99909334325994914, 0.22609024205745204, 0, 0, 0, 0.38067153181204749, -0.016221175313574965},
     {0, 17, 0, 31, 6, 7, 10, 17, 1, 0, 0, 20, 0, 0, 0, 0}},
    // member 24 of the family of seed 7 (tests/first_plan_ref.py)
    {128, 8, 0.01,
     {9.50916301e+09, 8.72817971e+09, 2.87574093e+09, 1.18055107e+10, 9.17245235e+09, 1.0145662e+10, 257.021637, 388029408,
      97528.7734, -93307.6172, 65.807251, 65.807251, 65.807251, 65.807251, 114.493248, 65.807251,
      47.2643738, 47.2643738, 47.2643738, 47.2643738, 95738.4141, -100603.367, 74.7481003, -19730.9277,
      53.307518, 53.307518, 53427.2852, -108435.148, 53.307518, 53.307518, 246.999268, 53.307518},
     {57.616945255494684, 48.207561883466695, 294.32282157360908, 0, -0.042573365542992951, -0.99909334325994914, 9.6952767501942727, 0, 0, 0, 0.61707281943415282, -0.026294706981728113},
     {61, 68, 0, 8, 63, 63, 2, 3, 1, 23, 5, 5, 0, 0, 0, 0}},
    // member 25 of the family of seed 7 (tests/first_plan_ref.py)
    {8, 128, 1.0,
     {1.58233242e+10, 1.21767004e+10, 6.58972672e+09, 9.99230054e+09, 1.039326e+10, 5.46689434e+09, 3.57757211, 2.32622968e+12,
      125743.68, -110240.758, 35.8611641, 35.8611641, 35.8611641, 35.8611641, 70.1360016, 35.8611641,
      32.6724701, 32.6724701, 32.6724701, 32.6724701, 101941.492, -73744.7344, 131.219833, 156.567139,
      53.7510986, 53.7510986, 81056.625, -99755.9766, 53.7510986, 53.7510986, -5.99629879, 53.7510986},
     {49.844754242572307, 50.907102395041527, 302.77941640635686, 0, -0.042573365542992951, -0.99909334325994914, 0.04055280164441917, 0, 0, 0, 0.54030569496202718, -0.023023506273721898},
     {0, 8, 0, 128, 2, 2, 51, 71, 1, 0, 0, 89, 0, 0, 0, 0}},
};

// exactly sized heap blocks: the table the twin reads is 32 floats (rows r2, x, y, z), the camera 12 doubles, the record 16 words
struct Blocks {
    std::unique_ptr<float[]> sph{new float[32]};
    std::unique_ptr<double[]> cam{new double[12]};
    std::unique_ptr<int32_t[]> rec{new int32_t[16]};
};

static void room(float *sph) {
    for (int k = 0; k < 8; ++k) {
        sph[k] = (float)(kRoom[k][0] * kRoom[k][0]);
        sph[8 + k] = (float)kRoom[k][1]; sph[16 + k] = (float)kRoom[k][2]; sph[24 + k] = (float)kRoom[k][3];
    }
}

static bool all_zero(const int32_t *rec) {
    for (int k = 0; k < 16; ++k) if (rec[k]) return false;
    return true;
}

// the record's invariants; -> whether it is the all-zero record
static bool invariants(const int32_t *rec, uint32_t w, uint32_t h) {
    for (int k = 0; k < 14; ++k) {
        if (k == 8) continue;
        const bool on_col = k == 0 || k == 1 || k == 4 || k == 5 || k == 9 || k == 10;
        CHECK(rec[k] >= 0 && (uint32_t)rec[k] <= (on_col ? w : h), "%u x %u entry %d = %d", w, h, k, rec[k]);
    }
    CHECK((rec[8] == 0 || rec[8] == 1) && rec[14] == 0 && rec[15] == 0, "%u x %u: [8] = %d, [14] = %d, [15] = %d", w, h, rec[8], rec[14], rec[15]);
    if (rec[0] || rec[1] || rec[2] || rec[3])
        CHECK((uint32_t)rec[0] <= w / 2 && w / 2 < (uint32_t)rec[1] && (uint32_t)rec[2] <= h / 2 && h / 2 < (uint32_t)rec[3],
              "%u x %u: wall_cols [%d, %d) wall_rows [%d, %d)", w, h, rec[0], rec[1], rec[2], rec[3]);
    return all_zero(rec);
}

// the header's table of the record, for one pixel
static uint32_t header_mask(const int32_t *r, int64_t w, int64_t h, int64_t c, int64_t j) {
    const bool inside = c >= r[0] && c < r[1] && j >= r[2] && j < r[3];
    uint32_t m = 0;
    if (inside && c >= w - r[4]) m |= 1u;
    if (inside && c < r[5]) m |= 2u;
    if (inside && r[8] != 0) m |= 8u;
    if (inside && j >= h - r[6]) m |= 16u;
    if (inside && j < r[7]) m |= 32u;
    if (c < r[9] || c >= w - r[10] || j < r[11] || j >= h - r[12]) m |= 64u;
    if (j < r[13]) m |= 128u;
    return m;
}

static void masks(const int32_t *rec, uint32_t w, uint32_t h) {
    // the pixels at the frame's corners and centre, on both sides of every boundary of the record, and random ones
    uint32_t cols[40], rows[40];
    int nc = 0, nr = 0;
    auto add = [](uint32_t *v, int &n, int64_t x, uint32_t lim) { if (x >= 0 && x < (int64_t)lim) v[n++] = (uint32_t)x; };
    for (int64_t x : {(int64_t)0, (int64_t)1, (int64_t)w / 2, (int64_t)w - 2, (int64_t)w - 1}) add(cols, nc, x, w);
    for (int64_t x : {(int64_t)0, (int64_t)1, (int64_t)h / 2, (int64_t)h - 2, (int64_t)h - 1}) add(rows, nr, x, h);
    for (int k : {0, 1, 5, 9}) for (int s = -1; s <= 0; ++s) add(cols, nc, (int64_t)rec[k] + s, w);
    for (int k : {4, 10}) for (int s = -1; s <= 0; ++s) add(cols, nc, (int64_t)w - rec[k] + s, w);
    for (int k : {2, 3, 7, 11, 13}) for (int s = -1; s <= 0; ++s) add(rows, nr, (int64_t)rec[k] + s, h);
    for (int k : {6, 12}) for (int s = -1; s <= 0; ++s) add(rows, nr, (int64_t)h - rec[k] + s, h);
    for (int i = 0; i < 4; ++i) { cols[nc++] = rnd(w); rows[nr++] = rnd(h); }
    for (int a = 0; a < nc; ++a)
        for (int b = 0; b < nr; ++b) {
            const uint32_t got = apt_first_plan_mask_host(rec, w, h, cols[a], rows[b]);
            CHECK(got == header_mask(rec, w, h, cols[a], rows[b]) && !(got & 4u), "%u x %u pixel (%u, %u): mask %u", w, h, cols[a], rows[b], got);
        }
}

int main() {
    Blocks b;
    float *sph = b.sph.get();
    double *cam = b.cam.get();
    int32_t *rec = b.rec.get();

    // ---- the edge shapes, the reference room
    const uint32_t shapes[][2] = {{1, 1}, {1, 2}, {2, 1}, {3, 1}, {1, 1080}, {1920, 1}, {1920, 1080}, {1u << 24, 1u << 24}, {(1u << 24) + 1, 5},
                                  {5, (1u << 24) + 1}, {(1u << 24) + 1, 1u << 24}, {1u << 24, (1u << 24) + 1}, {0xFFFFFFFFu, 0xFFFFFFFFu},
                                  {1u << 24, 1}, {1, 1u << 24}, {7, 4096}, {65535, 3}, {64, 36}, {33, 19}};
    room(sph);
    for (const auto &s : shapes)
        for (double eps : {1e-4, 1.0}) {
            memset(rec, 0xA5, 16 * sizeof(int32_t));
            CHECK(apt_first_plan_host(s[0], s[1], sph, eps, nullptr, rec) == 0, "%u x %u", s[0], s[1]);
            const bool zero = invariants(rec, s[0], s[1]);
            if (s[0] > (1u << 24) || s[1] > (1u << 24)) CHECK(zero, "%u x %u: beyond 2^24 and not refused", s[0], s[1]);
            masks(rec, s[0], s[1]);
            CHECK(apt_first_plan_camera_host(s[0], s[1], cam) == 0, "camera of %u x %u", s[0], s[1]);
            int32_t again[16];
            CHECK(apt_first_plan_host(s[0], s[1], sph, eps, cam, again) == 0 && memcmp(again, rec, sizeof again) == 0, "%u x %u: its own camera handed in", s[0], s[1]);
        }
    const int32_t headline[16] = {286, 1634, 0, 1013, 951, 951, 441, 620, 1, 212, 693, 63, 436, 854, 0, 0};   // profiles/first_bounce_plan_counts.json
    CHECK(apt_first_plan_host(1920, 1080, sph, 1e-4, nullptr, rec) == 0 && memcmp(rec, headline, sizeof headline) == 0, "the headline record");
    CHECK(apt_first_plan_host(1u << 24, 1u << 24, sph, 1e-4, nullptr, rec) == 0 && !all_zero(rec), "2^24 squared is accepted");

    // ---- null pointers and empty shapes
    memset(rec, 0xA5, 16 * sizeof(int32_t));
    CHECK(apt_first_plan_host(64, 36, nullptr, 1e-4, nullptr, rec) == 1 && apt_first_plan_host(64, 36, sph, 1e-4, nullptr, nullptr) == 1, "null pointers");
    CHECK(apt_first_plan_host(0, 36, sph, 1e-4, nullptr, rec) == 1 && apt_first_plan_host(64, 0, sph, 1e-4, nullptr, rec) == 1, "empty shapes");
    CHECK(rec[0] == (int32_t)0xA5A5A5A5 && rec[15] == (int32_t)0xA5A5A5A5, "a refused call wrote the record");
    CHECK(apt_first_plan_camera_host(64, 36, nullptr) == 1 && apt_first_plan_camera_host(0, 1, cam) == 1 && apt_first_plan_camera_host(1, 0, cam) == 1, "camera: refusals");
    CHECK(apt_first_plan_mask_host(nullptr, 64, 36, 0, 0) == 0, "mask of a null record");

    // ---- members of the test family, with the records the product build of the twin gave
    for (const Member &m : kMembers) {
        for (int i = 0; i < 32; ++i) sph[i] = (float)m.table[i];
        memcpy(cam, m.cam, 12 * sizeof(double));
        CHECK(apt_first_plan_host(m.w, m.h, sph, m.eps, cam, rec) == 0, "member %u x %u", m.w, m.h);
        CHECK(!invariants(rec, m.w, m.h), "member %u x %u is refused", m.w, m.h);
        CHECK(memcmp(rec, m.record, sizeof m.record) == 0, "member %u x %u: another record than the product build's", m.w, m.h);
        for (uint32_t c = 0; c < m.w; ++c)
            for (uint32_t j = 0; j < m.h; ++j)
                CHECK(apt_first_plan_mask_host(rec, m.w, m.h, c, j) == header_mask(rec, m.w, m.h, c, j), "member %u x %u pixel (%u, %u)", m.w, m.h, c, j);
        // the same tables at edge shapes, with the reference's camera of that shape
        for (const auto &s : shapes) {
            CHECK(apt_first_plan_host(s[0], s[1], sph, m.eps, nullptr, rec) == 0, "member at %u x %u", s[0], s[1]);
            invariants(rec, s[0], s[1]);
            masks(rec, s[0], s[1]);
        }
    }

    // ---- every table entry and every camera entry non-finite, one at a time: refused, nothing else touched
    const uint32_t w = 96, h = 54;
    const float bad_f[] = {NAN, INFINITY, -INFINITY};
    for (float bad : bad_f) {
        for (int i = 0; i < 32; ++i) {
            room(sph);
            sph[i] = bad;
            CHECK(apt_first_plan_host(w, h, sph, 1e-4, nullptr, rec) == 0 && all_zero(rec), "table entry %d = %f is not refused", i, (double)bad);
        }
        room(sph);
        for (int i = 0; i < 12; ++i) {
            CHECK(apt_first_plan_camera_host(w, h, cam) == 0, "camera");
            cam[i] = (double)bad;
            CHECK(apt_first_plan_host(w, h, sph, 1e-4, cam, rec) == 0 && all_zero(rec), "camera entry %d = %f is not refused", i, (double)bad);
        }
        CHECK(apt_first_plan_host(w, h, sph, (double)bad, nullptr, rec) == 0 && all_zero(rec), "eps = %f is not refused", (double)bad);
    }
    // ---- the other refusing premises
    room(sph);
    CHECK(apt_first_plan_host(w, h, sph, 1e-4, nullptr, rec) == 0 && !all_zero(rec), "the reference room at 96 x 54");
    for (double eps : {0.0, -1e-4, 1.0000001, 2.0}) CHECK(apt_first_plan_host(w, h, sph, eps, nullptr, rec) == 0 && all_zero(rec), "eps = %g", eps);
    const struct { int entry; double value; } cams[] = {{7, 1e-6}, {8, -1e-6}, {9, 1e-3}, {3, 1e-9}, {6, 0.0}, {6, -0.9}, {5, 0.5}, {2, 400.0}, {0, 200.0}, {1, -90.0}};
    for (const auto &c : cams) {
        CHECK(apt_first_plan_camera_host(w, h, cam) == 0, "camera");
        cam[c.entry] = c.value;
        CHECK(apt_first_plan_host(w, h, sph, 1e-4, cam, rec) == 0 && all_zero(rec), "camera entry %d = %g is not refused", c.entry, c.value);
    }
    for (int k = 0; k < 6; ++k)
        for (double r : {4.99e4, 1.301e5}) {
            room(sph);
            sph[k] = (float)(r * r);
            CHECK(apt_first_plan_host(w, h, sph, 1e-4, nullptr, rec) == 0 && all_zero(rec), "wall %d with radius %g", k, r);
        }
    const int shared[][2] = {{1, 2}, {1, 3}, {1, 4}, {1, 5}, {1, 7}, {2, 0}, {2, 1}, {2, 2}, {2, 3}, {3, 0}, {3, 1}, {3, 4}, {3, 5}, {3, 7}};
    for (const auto &e : shared) {
        room(sph);
        sph[e[0] * 8 + e[1]] = nextafterf(sph[e[0] * 8 + e[1]], 1e9f);
        CHECK(apt_first_plan_host(w, h, sph, 1e-4, nullptr, rec) == 0 && all_zero(rec), "row %d sphere %d off its plane by one ulp", e[0], e[1]);
    }

    // ---- the mask of arbitrary records: entries anywhere in [0, n], empty ranges included
    for (int t = 0; t < 400; ++t) {
        const uint32_t mw = 1 + rnd(40), mh = 1 + rnd(40);
        for (int k = 0; k < 16; ++k) {
            const bool on_col = k == 0 || k == 1 || k == 4 || k == 5 || k == 9 || k == 10;
            const uint32_t n = on_col ? mw : mh, pick = rnd(3);
            rec[k] = k >= 14 ? 0 : (k == 8 ? (int32_t)rnd(2) : (int32_t)(pick == 0 ? 0 : (pick == 1 ? n : rnd(n + 1))));
        }
        if (t & 1) { rec[0] = 0; rec[1] = (int32_t)mw; rec[2] = 0; rec[3] = (int32_t)mh; }
        for (uint32_t c = 0; c < mw; ++c)
            for (uint32_t j = 0; j < mh; ++j)
                CHECK(apt_first_plan_mask_host(rec, mw, mh, c, j) == header_mask(rec, mw, mh, c, j), "random record %d, %u x %u pixel (%u, %u)", t, mw, mh, c, j);
    }

    printf("ok %ld\n", g_checks);
    return 0;
}
