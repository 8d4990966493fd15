// host_helpers.cpp -- host-side entry points of librender_mi355x.so that need no GPU:
//   apt_gen_rays_host     scripts/gen_data.py:21-75   gen_rays (MT19937 legacy stream, float64 camera)
//   apt_gen_spheres_host  scripts/gen_data.py:92-132  gen_spheres
//   apt_gen_scene_host    build-defined large scene (BASELINE config 4; no reference counterpart)
//   apt_write_ppm         scripts/data_visualization.py:11-17 write_ppm
// Compiled with -ffp-contract=off like the kernels (shared arithmetic: pt_core.h).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include <string>

#include "../../include/render_mi355x.h"
#include "apt_host.h"
#include "film_ops.h"
#include "pt_core.h"
#include "pt_camera.h"
#include "pt_leaf.h"

// ---- error record and contexts (apt_host.h) ---------------------------------------------------------
namespace {
thread_local std::string t_err;
thread_local int t_status = APT_OK;
} // namespace

namespace apt {
void clear_error() { t_err.clear(); t_status = APT_OK; }
int set_error(int code, const char *fmt, const char *detail) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, detail);
    t_err = buf;
    t_status = code;
    return code;
}
apt_context &default_context() {
    static apt_context ctx;
    return ctx;
}
} // namespace apt

// The APT_* measurement knobs of the process environment are read HERE, once per context, and nowhere else: no launch path calls
// getenv() (it races with setenv() in another thread, and a per-context API must not depend on process-global state).
namespace {
double env_number(const char *name) {
    const char *e = getenv(name);
    return e ? atof(e) : 0.0;
}
} // namespace

apt_context::apt_context() {
    apt_default_params(&v_.params);
    v_.trace_counter = nullptr;
    v_.refill_lanes = apt::kDefaultRefillLanes;
    v_.has_camera = false;
    memset(&v_.camera, 0, sizeof v_.camera);
    v_.has_env = false;
    memset(&v_.env, 0, sizeof v_.env);
    struct { const char *env, *key; } knobs[] = {{"APT_QUEUE_PPW", "queue_ppw"}, {"APT_QUEUE_NBUF", "queue_nbuf"}, {"APT_QUEUE_LDS_PAD", "queue_lds_pad"},
                                                 {"APT_GRID_SPHERES_PER_CELL", "grid_spheres_per_cell"}};
    for (const auto &k : knobs) {
        const double v = env_number(k.env);
        if (v != 0.0) (void)set_debug(k.key, v);     // out-of-range values are ignored, as before
    }
    if (const char *e = getenv("APT_GRID_WALK")) if (e[0] == 'i') v_.debug.grid_walk = 1;   // "items"
    apt::clear_error();
}
apt_context::Values apt_context::snapshot() { std::lock_guard<std::mutex> g(m_); return v_; }
void apt_context::set_params(const apt_render_params &p) { std::lock_guard<std::mutex> g(m_); v_.params = p; }
void apt_context::set_trace_counter(unsigned long long *c) { std::lock_guard<std::mutex> g(m_); v_.trace_counter = c; }
void apt_context::set_refill_lanes(uint32_t lanes) { std::lock_guard<std::mutex> g(m_); v_.refill_lanes = lanes; }
void apt_context::set_camera(const apt_camera *cam) {
    std::lock_guard<std::mutex> g(m_);
    v_.has_camera = cam != nullptr;
    if (cam) v_.camera = *cam;
}
void apt_context::set_environment(const apt_environment *env) {
    std::lock_guard<std::mutex> g(m_);
    v_.has_env = env != nullptr;
    if (env) v_.env = *env;
}
int apt_context::set_debug(const char *key, double value) {
    if (!key) return apt::set_error(APT_ERR_ARG, "apt_context_set_debug: key is null%s");
    const std::string k(key);
    const bool whole = value == std::floor(value);
    std::lock_guard<std::mutex> g(m_);
    apt::Debug &d = v_.debug;
    if (k == "queue_ppw") { if (!(whole && value >= 0 && value <= 4096)) goto range; d.queue_ppw = (uint32_t)value; }
    else if (k == "queue_nbuf") { if (!(whole && (value == 0 || (value >= 2 && value <= 16)))) goto range; d.queue_nbuf = (uint32_t)value; }
    else if (k == "queue_lds_pad") { if (!(whole && value >= 0 && value <= 32768)) goto range; d.queue_lds_pad = (uint32_t)value; }
    else if (k == "grid_walk") { if (!(value == 0 || value == 1)) goto range; d.grid_walk = (uint32_t)value; }
    else if (k == "grid_spheres_per_cell") { if (!(value == 0 || (value > 0.01 && value < 1e6))) goto range; d.grid_spheres_per_cell = value; }
    else return apt::set_error(APT_ERR_ARG, "apt_context_set_debug: unknown key '%s'", key);
    return APT_OK;
range:
    return apt::set_error(APT_ERR_ARG, "apt_context_set_debug: value out of range for '%s'", key);
}
int apt_context::get_debug(const char *key, double *value) {
    if (!key) return apt::set_error(APT_ERR_ARG, "apt_context_get_debug: key is null%s");
    const std::string k(key);
    std::lock_guard<std::mutex> g(m_);
    const apt::Debug &d = v_.debug;
    if (k == "queue_ppw") *value = d.queue_ppw;
    else if (k == "queue_nbuf") *value = d.queue_nbuf;
    else if (k == "queue_lds_pad") *value = d.queue_lds_pad;
    else if (k == "grid_walk") *value = d.grid_walk;
    else if (k == "grid_spheres_per_cell") *value = d.grid_spheres_per_cell;
    else return apt::set_error(APT_ERR_ARG, "apt_context_get_debug: unknown key '%s'", key);
    return APT_OK;
}
uint32_t *apt_context::status_lookup(int dev) {
    if (dev < 0 || dev >= apt::kMaxStatusDevices) return nullptr;
    std::lock_guard<std::mutex> g(m_);
    return status_[dev];
}
uint32_t *apt_context::status_adopt(int dev, uint32_t *fresh, uint32_t **spare) {
    *spare = nullptr;
    if (dev < 0 || dev >= apt::kMaxStatusDevices) { *spare = fresh; return nullptr; }
    std::lock_guard<std::mutex> g(m_);
    if (status_[dev]) *spare = fresh;
    else status_[dev] = fresh;
    return status_[dev];
}
void apt_context::status_release(uint32_t *out[apt::kMaxStatusDevices]) {
    std::lock_guard<std::mutex> g(m_);
    for (int i = 0; i < apt::kMaxStatusDevices; ++i) { out[i] = status_[i]; status_[i] = nullptr; }
}

namespace {
using apt::set_error;

// np.random.seed(s); np.random.rand(): MT19937 (init_genrand) and the 53-bit
// random_sample construction ((a >> 5) * 2^26 + (b >> 6)) / 2^53.
class Mt19937 {
  public:
    explicit Mt19937(uint32_t seed) {
        mt_[0] = seed;
        for (int i = 1; i < kN; ++i) mt_[i] = 1812433253u * (mt_[i - 1] ^ (mt_[i - 1] >> 30)) + (uint32_t)i;
        pos_ = kN;
    }
    uint32_t next32() {
        if (pos_ >= kN) refill();
        uint32_t y = mt_[pos_++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    }
    double next_double() {
        const uint32_t a = next32() >> 5, b = next32() >> 6;
        return (a * 67108864.0 + b) / 9007199254740992.0;
    }

  private:
    static constexpr int kN = 624, kM = 397;
    void refill() {
        for (int i = 0; i < kN; ++i) {
            const uint32_t y = (mt_[i] & 0x80000000u) | (mt_[(i + 1) % kN] & 0x7fffffffu);
            mt_[i] = mt_[(i + kM) % kN] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        pos_ = 0;
    }
    uint32_t mt_[kN];
    int pos_;
};

// The reference scene table, (r, x, y, z, em*3, col*3) per sphere: gen_data.py:94-102.
const double kSpheres[8][10] = {
    {1e5, 1e5 + 1, 40.8, 81.6, 0, 0, 0, 0.435, 0.376, 0.667},     // Left
    {1e5, -1e5 + 99, 40.8, 81.6, 0, 0, 0, 0.667, 0.129, 0.086},   // Right
    {1e5, 50, 40.8, 1e5, 0, 0, 0, 0.270, 0.725, 0.486},           // Back
    {1e5, 50, 40.8, -1e5 + 170, 0, 0, 0, 0, 0, 0},                // Front (black)
    {1e5, 50, 1e5, 81.6, 0, 0, 0, 0.5, 0.5, 0.5},                 // Bottom
    {1e5, 50, -1e5 + 81.6, 81.6, 0, 0, 0, 0.141, 0.408, 0.635},   // Top
    {16.5, 27, 16.5, 47, 0, 0, 0, 0.999, 0.999, 0.999},           // Mirror
    {600, 50, 681.6 - 0.27, 81.6, 12, 12, 12, 0, 0, 0}};          // Light

void sphere_record(int k, float rec[10]) {
    for (int m = 0; m < 10; ++m) {
        double v = kSpheres[k][m];
        if (m == 0) v = v * v; // gen_data.py:109: r -> r^2 in float64, float32 only at tofile (:127)
        rec[m] = (float)v;
    }
}

size_t padded_floats(size_t n) { return (n + 127) / 128 * 128; } // gen_data.py:120-127: 512-byte multiple

} // namespace

extern "C" {

const char *apt_last_error(void) { return t_err.c_str(); }
int apt_last_status(void) { return t_status; }

void apt_default_params(apt_render_params *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->struct_size = sizeof *p;
    p->width = 16; p->height = 16; p->samples = 1; // common.h:4-6
    p->depth = 5;                                   // render.cpp:141
    p->num_spheres = 8; p->light_index = 7;         // common.h:10, rt_helper.h:776
    p->eps = 1e-4f; p->gain = 12.0f;                // common.h:9, render.cpp:194
    p->mode = APT_MODE_KERNEL;
}

int apt_gen_rays_host(uint32_t width, uint32_t height, uint32_t samples, uint32_t seed, float *rays) {
    apt::clear_error();
    if (!rays || !width || !height || !samples) return set_error(APT_ERR_ARG, "apt_gen_rays_host: rays must be non-null, width/height/samples non-zero%s");
    Mt19937 rng(seed); // np.random.seed(0): gen_data.py:438
    apt::Camera cam;
    apt::camera_init(cam, width, height);
    const uint64_t n = (uint64_t)width * height * 4u * samples;
    uint64_t p = 0;
    for (uint32_t i = 0; i < width; ++i)               // gen_data.py:32-36 loop nest
        for (uint32_t j = 0; j < height; ++j)
            for (uint32_t sy = 0; sy < 2; ++sy)
                for (uint32_t sx = 0; sx < 2; ++sx)
                    for (uint32_t k = 0; k < samples; ++k, ++p) {
                        const double u1 = rng.next_double(); // r1 before r2: :37,:39
                        const double u2 = rng.next_double();
                        const apt::Ray ray = apt::camera_ray(cam, width, height, i, j, sy, sx, u1, u2);
                        rays[p] = ray.ox; rays[n + p] = ray.oy; rays[2 * n + p] = ray.oz;   // SoA: :65-71
                        rays[3 * n + p] = ray.dx; rays[4 * n + p] = ray.dy; rays[5 * n + p] = ray.dz;
                    }
    return APT_OK;
}

// The fast direction of ray-generate and its accept rule (pt_core.h fast_direction) on the host, with y = (1/sqrt(n2)) * (1 + rsq_rel_error)
// standing in for v_rsq_f64, against the exact form (float)(d_k / sqrt(n2)).
int apt_selftest_direction_host(const double *d3, uint64_t count, double rsq_rel_error, uint64_t *result5, uint8_t *flags) {
    apt::clear_error();
    if (!d3 || !result5 || !(rsq_rel_error >= -0x1p-20 && rsq_rel_error <= 0x1p-20))
        return set_error(APT_ERR_ARG, "apt_selftest_direction_host: d3 and result5 must be non-null, |rsq_rel_error| <= 2^-20%s");
    uint64_t max_cert = result5[4];
    for (uint64_t i = 0; i < count; ++i) {
        const double d0 = d3[3 * i], d1 = d3[3 * i + 1], d2 = d3[3 * i + 2];
        const double n2 = apt::norm3_sq(d0, d1, d2), n = sqrt(n2);
        const double y = (1.0 / n) * (1.0 + rsq_rel_error);
        double cert;
        const uint32_t f = apt::dir_probe(d0, d1, d2, y, (float)(d0 / n), (float)(d1 / n), (float)(d2 / n), cert);
        result5[(f & 71u) == 71u ? 0 : 1] += 1;
        result5[2] += ((f & (f >> 3)) & 1u) + ((f & (f >> 3)) >> 1 & 1u) + ((f & (f >> 3)) >> 2 & 1u);
        result5[3] += (f & 64u) ? 0 : 1;
        if (std::isfinite(cert)) {
            const double ac = fabs(cert);
            uint64_t b;
            memcpy(&b, &ac, sizeof b);
            max_cert = b > max_cert ? b : max_cert;
        }
        if (flags) flags[i] = (uint8_t)f;
    }
    result5[4] = max_cert;
    return APT_OK;
}

// The generator states render_frame's two-paths-per-lane kernel forms by addition (pt_core.h lane_base_state, chain_state_uniform,
// kPairStateStep), for every lane of the pixels [pixel_begin, pixel_begin + pixel_count) and every pair of the frame's plan, against the
// definition: the two outputs of path_uniforms(seed, path) are splitmix64(s) and splitmix64(s + phi), s = splitmix64(seed) + path * kPathStride.
// The leaf and pair loops below MIRROR render_frame_kernel's (pt_kernels.h, TWO): they are not shared with it and have to be kept in step
// by hand; what guards the kernel itself are the frame-parity tests on the GPU.
int apt_selftest_chain_states_host(uint32_t samples, uint64_t seed, uint64_t pixel_begin, uint64_t pixel_count, uint64_t *result3) {
    apt::clear_error();
    apt::LeafProg lp;
    if (!result3 || !samples || !apt::make_leaf_plan(samples, lp))
        return set_error(APT_ERR_ARG, "apt_selftest_chain_states_host: result3 must be non-null, samples non-zero with a pairwise plan%s");
    const uint64_t phi = 0x9E3779B97F4A7C15ull;
    auto differs = [&](uint64_t state, uint64_t path) {
        const uint64_t s = apt::splitmix64(seed) + path * apt::kPathStride;
        return apt::splitmix64(state) != apt::splitmix64(s) || apt::splitmix64(state + phi) != apt::splitmix64(s + phi);
    };
    for (uint64_t q = pixel_begin; q < pixel_begin + pixel_count; ++q)
        for (uint32_t sub = 0; sub < 4; ++sub)
            for (uint32_t j = 0; j < 8; ++j) {                                        // the lane (pt_frame.h frame_lane, GROUP == 8)
                const uint64_t pbase = (q * 4 + sub) * samples;
                const uint64_t lane = apt::lane_base_state(seed, pbase, j);
                uint32_t start = 0;
                for (uint32_t leaf = 0; leaf < lp.nleaves; ++leaf) {                   // pt_kernels.h render_frame_kernel, TWO
                    const uint32_t n = lp.len(leaf), nfull = n & ~7u;
                    uint32_t i8 = 0;
                    if (samples >= 8 && nfull >= 16)
                        for (; i8 + 16 <= nfull; i8 += 16) {
                            const uint64_t a = apt::chain_state_uniform(lane, start + i8);
                            result3[1] += differs(a, pbase + start + i8 + j) ? 1 : 0;
                            result3[1] += differs(a + apt::kPairStateStep, pbase + start + i8 + 8 + j) ? 1 : 0;
                            result3[0] += 2;
                        }
                    result3[2] += (nfull - i8) / 8 + (j < n - nfull ? 1 : 0);          // traced one at a time, from path_uniforms itself
                    start += n;
                }
            }
    return APT_OK;
}

// The tent filter from the generator's bits (pt_core.h tent_e_from_bits, tent_e: what the two-paths-per-lane kernel's ray-generate
// uses) against the form every other caller keeps, tent_t(unit_from_bits(z)), on the 64-bit generator outputs z[0 .. count).
int apt_selftest_tent_bits_host(const uint64_t *z, uint64_t count, uint64_t *result2) {
    apt::clear_error();
    if (!result2 || (!z && count)) return set_error(APT_ERR_ARG, "apt_selftest_tent_bits_host: z and result2 must be non-null%s");
    auto bits = [](double d) { uint64_t b; memcpy(&b, &d, sizeof b); return b; };
    for (uint64_t i = 0; i < count; ++i) {
        double xe, xt;
        const double te = apt::tent_e<false>(apt::tent_e_from_bits(z[i]), xe);
        const double tt = apt::tent_t<false>(apt::unit_from_bits(z[i]), xt);
        result2[0] += bits(xe) != bits(xt) ? 1 : 0;
        result2[1] += (bits(te) != bits(tt) && !(te == 0.0 && tt == 0.0)) ? 1 : 0;
    }
    return APT_OK;
}

// Checkpoints of the MT19937 stream for the device generator (apt_gen_rays_mt_device).  Output
// block b (624 words = the 4 words of 156 consecutive paths) is the tempering of the state after
// b+1 twists; checkpoint i is that raw state for block i*stride.  Sequential by nature; done once
// per (seed, length) and reusable for every shorter length.
int apt_mt19937_checkpoints_window(const uint32_t *state_in, uint32_t seed, uint64_t first_block, uint64_t num_blocks,
                                   uint32_t stride, uint32_t *states, uint32_t *state_out) {
    apt::clear_error();
    if (!states || stride == 0 || num_blocks == 0) return set_error(APT_ERR_ARG, "apt_mt19937_checkpoints_window: states must be non-null, stride and num_blocks non-zero%s");
    uint32_t mt[624];
    auto twist = [&]() { // genrand twist
        for (int i = 0; i < 624; ++i) {
            const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
    };
    if (state_in) memcpy(mt, state_in, sizeof mt);
    else {
        mt[0] = seed;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        for (uint64_t b = 0; b <= first_block; ++b) twist(); // block b is the tempering of the state after b+1 twists
    }
    for (uint64_t k = 0; k < num_blocks; ++k) {               // mt = raw state of block first_block + k
        if (k % stride == 0) memcpy(states + (k / stride) * 624, mt, sizeof mt);
        if (k + 1 < num_blocks || state_out) twist();
    }
    if (state_out) memcpy(state_out, mt, sizeof mt);
    return APT_OK;
}

int apt_mt19937_checkpoints_host(uint32_t seed, uint64_t num_blocks, uint32_t stride, uint32_t *states) {
    return apt_mt19937_checkpoints_window(nullptr, seed, 0, num_blocks, stride, states, nullptr);
}

int apt_gen_spheres_host(float *spheres128) {
    apt::clear_error();
    if (!spheres128) return set_error(APT_ERR_ARG, "apt_gen_spheres_host: spheres128 is null%s");
    memset(spheres128, 0, 128 * sizeof(float));
    for (int k = 0; k < 8; ++k) {
        float rec[10];
        sphere_record(k, rec);
        for (int m = 0; m < 10; ++m) spheres128[m * 8 + k] = rec[m]; // transpose to planes: :113
    }
    return APT_OK;
}

// The demo scene of the material entries: gen_spheres' eight spheres (light still index 7) and, as sphere 8, the glass ball the
// reference's scene list carries commented out (gen_data.py:84, :103): r 16.5 at (73, 16.5, 78), albedo 0.999.  smallpt's materials
// (gen_data.py:77-87): the walls and the light DIFF, the mirror SPEC, the ball REFR.  [10][9] planes in 128 floats, like gen_spheres.
int apt_gen_spheres_materials_host(float *spheres, uint32_t *materials) {
    apt::clear_error();
    if (!spheres || !materials) return set_error(APT_ERR_ARG, "apt_gen_spheres_materials_host: spheres/materials is null%s");
    constexpr int kNs = 9;
    memset(spheres, 0, padded_floats(kNs * 10) * sizeof(float));
    for (int k = 0; k < kNs; ++k) {
        float rec[10];
        if (k < 8) sphere_record(k, rec);
        else {
            const double glass[10] = {16.5, 73, 16.5, 78, 0, 0, 0, 0.999, 0.999, 0.999};
            for (int m = 0; m < 10; ++m) rec[m] = (float)(m == 0 ? glass[m] * glass[m] : glass[m]);
        }
        for (int m = 0; m < 10; ++m) spheres[m * kNs + k] = rec[m];
        materials[k] = k == 6 ? APT_MAT_SPEC : (k == 8 ? APT_MAT_REFR : APT_MAT_DIFF);
    }
    return APT_OK;
}

int apt_gen_scene_host(uint32_t num_spheres, uint64_t seed, float *spheres, size_t *out_floats) {
    apt::clear_error();
    if (num_spheres < 8) return set_error(APT_ERR_SCENE, "apt_gen_scene_host: needs num_spheres >= 8 (six walls, at least one sphere, the light)%s");
    const size_t total = padded_floats((size_t)num_spheres * 10);
    if (out_floats) *out_floats = total;
    if (!spheres) return APT_OK;
    memset(spheres, 0, total * sizeof(float));
    for (uint32_t k = 0; k < num_spheres; ++k) {
        float rec[10];
        if (k < 6) sphere_record((int)k, rec);                 // the six walls
        else if (k == num_spheres - 1) sphere_record(7, rec);  // the light keeps index Ns-1
        else {                                                 // small random spheres inside the room
            uint64_t s = apt::splitmix64(seed ^ apt::splitmix64(0x5CE7E000ull + k));
            if (s == 0) s = 0x9E3779B97F4A7C15ull;
            double u[7];
            for (int m = 0; m < 7; ++m) u[m] = (double)(apt::xorshift64s(s) >> 11) * (1.0 / 9007199254740992.0);
            const double r = 0.5 + 1.5 * u[0];
            rec[0] = (float)(r * r);
            rec[1] = (float)(1.0 + 98.0 * u[1]);
            rec[2] = (float)(81.6 * u[2]);
            rec[3] = (float)(170.0 * u[3]);
            rec[4] = rec[5] = rec[6] = 0.0f;
            rec[7] = (float)(0.1 + 0.899 * u[4]);
            rec[8] = (float)(0.1 + 0.899 * u[5]);
            rec[9] = (float)(0.1 + 0.899 * u[6]);
        }
        for (int m = 0; m < 10; ++m) spheres[(size_t)m * num_spheres + k] = rec[m];
    }
    return APT_OK;
}

// The material codes that go with apt_gen_scene_host's scene of the same (num_spheres, seed): the walls (0..5) and the light (Ns-1) DIFF,
// small sphere i one of the three codes by (splitmix64(seed + i) >> 32) % 3 (uint64 wrap-around).
int apt_gen_scene_materials_host(uint32_t num_spheres, uint64_t seed, uint32_t *materials) {
    apt::clear_error();
    if (num_spheres < 8) return set_error(APT_ERR_SCENE, "apt_gen_scene_materials_host: needs num_spheres >= 8 (six walls, at least one sphere, the light)%s");
    if (!materials) return set_error(APT_ERR_ARG, "apt_gen_scene_materials_host: materials is null%s");
    for (uint32_t i = 0; i < num_spheres; ++i)
        materials[i] = (i < 6 || i == num_spheres - 1) ? (uint32_t)APT_MAT_DIFF : (uint32_t)((apt::splitmix64(seed + i) >> 32) % 3u);
    return APT_OK;
}

// The light table of the *_lights entries (include/render_mi355x.h "several lights" states the construction; pt_core.h the layout).
size_t apt_lights_bytes(uint32_t num_spheres, uint32_t num_lights) { return apt::lights_words(num_spheres, num_lights) * sizeof(uint32_t); }

int apt_build_lights_host(const float *sph, uint32_t ns, const uint32_t *indices, uint32_t num_indices, void *lights, size_t capacity,
                          size_t *out_bytes) {
    apt::clear_error();
    if (!sph || !lights) return set_error(APT_ERR_ARG, "apt_build_lights_host: spheres/lights must be non-null%s");
    if (ns == 0) return set_error(APT_ERR_SCENE, "apt_build_lights_host: num_spheres is 0%s");
    const float *r2 = sph, *ex = sph + 4 * (size_t)ns, *ey = sph + 5 * (size_t)ns, *ez = sph + 6 * (size_t)ns;
    std::vector<uint32_t> g;
    if (indices) {
        g.assign(indices, indices + num_indices);
    } else {
        for (uint32_t k = 0; k < ns; ++k)
            if (ex[k] > 0.0f || ey[k] > 0.0f || ez[k] > 0.0f) g.push_back(k);
    }
    if (g.empty()) return set_error(APT_ERR_SCENE, indices ? "apt_build_lights_host: the index list is empty%s" : "apt_build_lights_host: no sphere of the scene emits%s");
    const size_t n = g.size(), nbits = ((size_t)ns + 31) / 32;
    std::vector<uint32_t> bits(nbits, 0u);
    for (uint32_t k : g) {
        if (k >= ns) return set_error(APT_ERR_SCENE, "apt_build_lights_host: a light index is out of range%s");
        if (bits[k >> 5] & (1u << (k & 31u))) return set_error(APT_ERR_SCENE, "apt_build_lights_host: a sphere is listed twice%s");
        bits[k >> 5] |= 1u << (k & 31u);
    }
    const size_t bytes = apt_lights_bytes(ns, (uint32_t)n);
    // power, half of the selection by it and half uniform (the floor), then the cumulative sums on the 24-bit grid of the draw
    std::vector<double> w(n);
    double W = 0.0;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t k = g[i];
        const double e = ((double)ex[k] + (double)ey[k]) + (double)ez[k];
        const double p = e * (double)r2[k];
        w[i] = (p > 0.0 && p < HUGE_VAL) ? p : 0.0;
        W = W + w[i];
    }
    const bool by_power = W > 0.0 && W < HUGE_VAL;
    const double floor_q = 0.5 / (double)n;
    std::vector<uint64_t> m(n);
    double S = 0.0;
    uint64_t before = 0;
    for (size_t i = 0; i < n; ++i) {
        const double a = by_power ? (0.5 * w[i]) / W : floor_q;
        const double q = a + floor_q;
        S = S + q;
        const double scaled = S * 16777216.0;
        m[i] = i + 1 == n ? (uint64_t)1 << 24 : (uint64_t)std::floor(scaled + 0.5);
        if (m[i] <= before || m[i] > ((uint64_t)1 << 24)) return set_error(APT_ERR_SCENE, "apt_build_lights_host: a light's selection probability would be below 2^-24 (too many lights)%s");
        before = m[i];
    }
    if (out_bytes) *out_bytes = bytes;
    if (capacity < bytes) return set_error(APT_ERR_ARG, "apt_build_lights_host: capacity is smaller than apt_lights_bytes(num_spheres, n)%s");
    std::vector<uint32_t> out(bytes / sizeof(uint32_t), 0u);
    out[0] = apt::kLightsMagic; out[1] = ns; out[2] = (uint32_t)n; out[3] = (uint32_t)out.size(); out[4] = bits[0];
    uint32_t *idx = out.data() + apt::kLightsHead;
    float *cdf = reinterpret_cast<float *>(idx + n), *invp = cdf + n;
    before = 0;
    for (size_t i = 0; i < n; ++i) {
        idx[i] = g[i];
        cdf[i] = (float)m[i] * 0x1p-24f;                          // exact: m <= 2^24
        const float P = (float)(m[i] - before) * 0x1p-24f;        // exact
        invp[i] = 1.0f / P;                                       // RN(1 / P): one IEEE fp32 division
        before = m[i];
    }
    memcpy(invp + n, bits.data(), nbits * sizeof(uint32_t));
    memcpy(lights, out.data(), bytes);
    return APT_OK;
}

uint32_t apt_materials_flags_host(const uint32_t *materials_host, uint32_t num_spheres) {
    if (!materials_host) return 0u;
    for (uint32_t k = 0; k < num_spheres; ++k) {
        const uint32_t w = materials_host[k], q = (w >> 8) & 0xFFFFu;
        if ((w & 0xFFu) == (uint32_t)APT_MAT_GLOSS && q != 0u && (w >> 24) == 0u) return APT_FLAG_GLOSS;
    }
    return 0u;
}

uint32_t apt_grid_flags(const void *grid_head_host, uint32_t num_spheres) {
    apt::clear_error();
    if (!grid_head_host) return 0u;
    apt::GridHeader h;
    memcpy(&h, grid_head_host, sizeof h);
    return (h.magic == apt::kGridMagic && h.num_spheres == num_spheres && h.off_cellslot != 0u) ? (uint32_t)APT_FLAG_GRID_SLOTS : 0u;
}

// Uniform grid for scenes with many spheres (apt_render_params.accel).  Spheres whose radius exceeds 8x the median
// radius, or that are not finite (pt_core.h grid_is_large), are "large" (the walls and the light of the generated scenes, r >= 600):
// they go to an always-tested list; the others are binned by their bounding boxes, inflated by `margin`
// so that any ray the fp32 intersection formula can possibly accept passes through the interior of a
// cell that lists the sphere (the formula's absolute error on disc is ~1e-3 at these coordinates; the
// margin is 0.05 + 1e-4 * coordinate scale).  Cells are sized for kGridSpheresPerCell = 0.5 sphere centres each (apt_set_debug("grid_spheres_per_cell", v) overrides: tuning knob).
int apt_build_grid_host(const float *sph, uint32_t ns, void *grid, size_t *out_bytes) {
    apt::clear_error();
    if (!sph || ns == 0 || !out_bytes) return set_error(APT_ERR_ARG, "apt_build_grid_host: spheres/out_bytes must be non-null, num_spheres non-zero%s");
    const float *r2 = sph, *cx = sph + ns, *cy = sph + 2 * (size_t)ns, *cz = sph + 3 * (size_t)ns;
    std::vector<float> rad(ns);
    for (uint32_t k = 0; k < ns; ++k) rad[k] = apt::grid_radius(r2[k]);
    std::vector<float> sorted(rad);
    std::nth_element(sorted.begin(), sorted.begin() + ns / 2, sorted.end());
    const float median = sorted[ns / 2];
    std::vector<uint32_t> large, small;
    for (uint32_t k = 0; k < ns; ++k)
        (apt::grid_is_large(r2[k], cx[k], cy[k], cz[k], rad[k], median) ? large : small).push_back(k);
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f}, scale = 1.0f;
    for (uint32_t k : small) {
        const float c[3] = {cx[k], cy[k], cz[k]};
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], c[a] - rad[k]); hi[a] = std::max(hi[a], c[a] + rad[k]); scale = std::max(scale, std::fabs(c[a]) + rad[k]); }
    }
    // sphere centres per cell (boxes overlap ~4 cells each).  The nested walk (round 1, 64 spp): 74.4 / 70.7 / 70.3 / 70.8 / 72.2 ms at 2 / 1 / 0.7 /
    // 0.5 / 0.35; the sample-queue kernel's grid form (round 3): 66.8 / 60.1 / 58.8 / 58.4 / 59.0 / 60.5 / 63.6 ms at 2 / 1 / 0.7 / 0.5 / 0.35 / 0.25 /
    // 0.18 -- a cell step is cheaper there than a pair slot, so smaller cells pay a little longer.
    apt::GridHeader h;
    apt::grid_header_from_stats(ns, (uint32_t)small.size(), (uint32_t)large.size(), lo, hi, scale, apt::grid_spheres_per_cell(), h);
    std::vector<uint32_t> count(h.ncells + 1, 0);
    for (uint32_t k : small) {
        uint32_t x0, x1, y0, y1, z0, z1;
        apt::grid_cell_range(h, cx[k], rad[k], 0, x0, x1); apt::grid_cell_range(h, cy[k], rad[k], 1, y0, y1); apt::grid_cell_range(h, cz[k], rad[k], 2, z0, z1);
        for (uint32_t z = z0; z <= z1; ++z) for (uint32_t y = y0; y <= y1; ++y) for (uint32_t x = x0; x <= x1; ++x)
            if (apt::grid_cell_touches(h, cx[k], cy[k], cz[k], rad[k], x, y, z)) ++count[(z * h.n[1] + y) * h.n[0] + x + 1];
    }
    for (uint32_t c = 0; c < h.ncells; ++c) count[c + 1] += count[c];
    const size_t words = apt::grid_header_offsets(h, count[h.ncells]);
    *out_bytes = words * 4;
    if (!grid) return APT_OK;
    uint32_t *w = (uint32_t *)grid;
    memset(w, 0, words * 4);
    memcpy(w, &h, sizeof h);
    for (size_t i = 0; i < large.size(); ++i) w[h.off_large + i] = large[i];
    memcpy(w + h.off_cells, count.data(), (h.ncells + 1) * 4);
    std::vector<uint32_t> cursor(count.begin(), count.end() - 1);
    for (uint32_t k : small) {                                                       // ascending sphere index inside a cell
        uint32_t x0, x1, y0, y1, z0, z1;
        apt::grid_cell_range(h, cx[k], rad[k], 0, x0, x1); apt::grid_cell_range(h, cy[k], rad[k], 1, y0, y1); apt::grid_cell_range(h, cz[k], rad[k], 2, z0, z1);
        for (uint32_t z = z0; z <= z1; ++z) for (uint32_t y = y0; y <= y1; ++y) for (uint32_t x = x0; x <= x1; ++x)
            if (apt::grid_cell_touches(h, cx[k], cy[k], cz[k], rad[k], x, y, z)) w[h.off_items + cursor[(z * h.n[1] + y) * h.n[0] + x]++] = k;
    }
    float *g = (float *)(w + h.off_geom);
    for (uint32_t k = 0; k < ns; ++k) { g[4 * k] = cx[k]; g[4 * k + 1] = cy[k]; g[4 * k + 2] = cz[k]; g[4 * k + 3] = r2[k]; }
    float *ig = (float *)(w + h.off_item_geom);
    for (uint32_t i = 0; i < h.nitems; ++i) memcpy(ig + 4 * (size_t)i, g + 4 * (size_t)w[h.off_items + i], 16);
    if (h.off_cellslot) {                                                                             // pair-slot tables of the flat walk
        for (uint32_t t = 0, nb = apt::grid_bordered_cells(h.n); t <= nb; ++t) apt::grid_fill_cell_slots(w, h, t);
        for (uint32_t k = 0; k < ns; ++k) apt::grid_fill_sphere8(w, h, sph, k);
    }
    return APT_OK;
}

// write_ppm: the reference's loop `for i in range(w): for j in range(h): data[j, i]` over the
// (w,h,3) array returned by decode_color (second index already y-flipped) emits file row i
// = image row y = h-1-i and file column j = x.  It only stays in range for w == h; the
// non-square case is defined here the evident way, h rows of w pixels.
int apt_write_ppm(const char *path, uint32_t width, uint32_t height, const uint8_t *fb_u8) {
    apt::clear_error();
    if (!path || !fb_u8 || !width || !height) return set_error(APT_ERR_ARG, "apt_write_ppm: path/fb_u8 must be non-null, width/height non-zero%s");
    FILE *f = fopen(path, "w");
    if (!f) return set_error(APT_ERR_IO, "apt_write_ppm: cannot open %s", path);
    fprintf(f, "P3\n%u %u\n255\n", width, height);
    for (uint32_t row = 0; row < height; ++row) {
        const uint32_t y = height - 1 - row;
        for (uint32_t x = 0; x < width; ++x) {
            const uint8_t *px = fb_u8 + ((uint64_t)x * height + y) * 3;
            fprintf(f, "%u %u %u ", px[0], px[1], px[2]);
        }
        fprintf(f, "\n");
    }
    return fclose(f) == 0 ? APT_OK : set_error(APT_ERR_IO, "apt_write_ppm: write to %s failed", path);
}

} // extern "C"

// ---- camera (include/render_mi355x.h "camera"): the record's host helpers.  float64, one operation at a time (-ffp-contract=off), in the
// manner of camera_init (pt_core.h); tests/camera_ref.py restates them.
namespace {
using apt::set_error;
bool cam_finite3(const double v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
bool cam_within3(const double v[3], double m) { return fabs(v[0]) <= m && fabs(v[1]) <= m && fabs(v[2]) <= m; }
bool cam_zero3(const double v[3]) { return v[0] == 0 && v[1] == 0 && v[2] == 0; }
void cam_cross(const double p[3], const double q[3], double out[3]) {   // np.cross
    out[0] = p[1] * q[2] - p[2] * q[1];
    out[1] = p[2] * q[0] - p[0] * q[2];
    out[2] = p[0] * q[1] - p[1] * q[0];
}
// The refusals of apt_camera_check_host, struct_size aside.  `what`: the entry's name for the message.
int cam_check_fields(const apt_camera &c, const char *what) {
    if (!(cam_finite3(c.pos) && cam_finite3(c.g) && cam_finite3(c.cx) && cam_finite3(c.cy) && cam_finite3(c.lens_u) && cam_finite3(c.lens_v) &&
          std::isfinite(c.offset) && std::isfinite(c.aperture) && std::isfinite(c.focus) && std::isfinite(c.offset_over_focus)))
        return set_error(APT_ERR_ARG, "%s: camera: a field is not finite", what);
    if (!(cam_within3(c.pos, apt::kCamMaxPos) && cam_within3(c.cx, apt::kCamMaxAxis) && cam_within3(c.cy, apt::kCamMaxAxis) &&
          cam_within3(c.g, apt::kCamMaxUnit) && cam_within3(c.lens_u, apt::kCamMaxUnit) && cam_within3(c.lens_v, apt::kCamMaxUnit) &&
          c.offset <= apt::kCamMaxPos && c.aperture <= apt::kCamMaxAxis && fabs(c.focus) <= apt::kCamMaxPos))
        return set_error(APT_ERR_ARG, "%s: camera: a field is outside the magnitude bound (|pos|, offset, focus <= 2^30; |cx|, |cy|, aperture <= 2^20)", what);
    if (cam_zero3(c.g) || cam_zero3(c.cx) || cam_zero3(c.cy)) return set_error(APT_ERR_ARG, "%s: camera: g, cx and cy must be non-zero", what);
    if (c.offset < 0) return set_error(APT_ERR_ARG, "%s: camera: offset < 0", what);
    if (c.aperture < 0) return set_error(APT_ERR_ARG, "%s: camera: aperture < 0", what);
    if (c.aperture > 0) {
        if (!(c.focus >= apt::kCamMinFocus)) return set_error(APT_ERR_ARG, "%s: camera: a lens (aperture > 0) needs focus >= 2^-20", what);
        if (cam_zero3(c.lens_u) || cam_zero3(c.lens_v)) return set_error(APT_ERR_ARG, "%s: camera: a lens needs non-zero lens_u and lens_v", what);
        if (c.offset_over_focus != c.offset / c.focus) return set_error(APT_ERR_ARG, "%s: camera: offset_over_focus must be offset / focus", what);
    }
    return APT_OK;
}
int cam_check_out(const apt_camera *out, uint32_t width, uint32_t height, const char *what) {
    if (!out) return set_error(APT_ERR_ARG, "%s: camera: out is null", what);
    if (out->struct_size != sizeof(apt_camera)) return set_error(APT_ERR_STRUCT, "%s: apt_camera.struct_size mismatch", what);
    if (!width || !height) return set_error(APT_ERR_ARG, "%s: camera: width/height must be non-zero", what);
    return APT_OK;
}
} // namespace

extern "C" {

int apt_camera_default_host(uint32_t width, uint32_t height, apt_camera *out) {
    apt::clear_error();
    int rc = cam_check_out(out, width, height, "apt_camera_default_host");
    if (rc) return rc;
    apt::Camera c;
    apt::camera_init(c, width, height);
    apt_camera r;
    memset(&r, 0, sizeof r);
    r.struct_size = sizeof r;
    for (int k = 0; k < 3; ++k) { r.pos[k] = c.pos[k]; r.g[k] = c.g[k]; r.cx[k] = c.cx[k]; r.cy[k] = c.cy[k]; }
    double cr[3];
    cam_cross(c.cx, c.g, cr);                                   // camera_init's own cross product, before its * 0.5135
    const double cn = apt::norm3(cr[0], cr[1], cr[2]);
    for (int k = 0; k < 3; ++k) r.lens_v[k] = cr[k] / cn;
    r.lens_u[0] = 1; r.lens_u[1] = 0; r.lens_u[2] = 0;
    r.offset = 140;
    if ((rc = cam_check_fields(r, "apt_camera_default_host"))) return rc;   // (an absurd aspect ratio leaves the bound)
    *out = r;
    return APT_OK;
}

int apt_camera_build_host(const double eye[3], const double dir[3], const double up[3], double scale, double offset, double aperture,
                          double focus, uint32_t width, uint32_t height, apt_camera *out) {
    apt::clear_error();
    const char *what = "apt_camera_build_host";
    if (!eye || !dir || !up) return set_error(APT_ERR_ARG, "%s: eye/dir/up must be non-null", what);
    int rc = cam_check_out(out, width, height, what);
    if (rc) return rc;
    if (!(cam_finite3(eye) && cam_finite3(dir) && cam_finite3(up) && std::isfinite(scale) && std::isfinite(offset) && std::isfinite(aperture) &&
          std::isfinite(focus))) return set_error(APT_ERR_ARG, "%s: an input is not finite", what);
    if (!(cam_within3(eye, apt::kCamMaxPos) && cam_within3(dir, apt::kCamMaxPos) && cam_within3(up, apt::kCamMaxPos)))
        return set_error(APT_ERR_ARG, "%s: |eye|, |dir|, |up| components must be <= 2^30", what);
    if (!(scale >= apt::kCamMinScale && scale <= apt::kCamMaxScale)) return set_error(APT_ERR_ARG, "%s: scale must lie in [2^-20, 2^20]", what);
    if (offset < 0) return set_error(APT_ERR_ARG, "%s: offset < 0", what);
    if (aperture < 0) return set_error(APT_ERR_ARG, "%s: aperture < 0", what);
    if (aperture > 0 && !(focus > 0)) return set_error(APT_ERR_ARG, "%s: a lens (aperture > 0) needs focus > 0", what);
    apt_camera r;
    memset(&r, 0, sizeof r);
    r.struct_size = sizeof r;
    const double gn = apt::norm3(dir[0], dir[1], dir[2]), un2 = apt::norm3_sq(up[0], up[1], up[2]);
    if (!(gn >= apt::kCamMinNorm) || !(un2 >= apt::kCamMinNorm * apt::kCamMinNorm)) return set_error(APT_ERR_ARG, "%s: dir and up must be non-zero (norm >= 2^-30)", what);
    for (int k = 0; k < 3; ++k) r.g[k] = dir[k] / gn;
    double c[3];
    cam_cross(r.g, up, c);
    const double c2 = apt::norm3_sq(c[0], c[1], c[2]);
    if (!(c2 >= apt::kCamMinSin2 * un2)) return set_error(APT_ERR_ARG, "%s: up is parallel to dir", what);
    const double cn = sqrt(c2);
    double right[3];
    for (int k = 0; k < 3; ++k) right[k] = c[k] / cn;
    const double sx = ((double)width * scale) / (double)height;
    for (int k = 0; k < 3; ++k) r.cx[k] = right[k] * sx;
    double e[3];
    cam_cross(r.cx, r.g, e);
    const double en = apt::norm3(e[0], e[1], e[2]);
    for (int k = 0; k < 3; ++k) {
        r.lens_v[k] = e[k] / en;
        r.cy[k] = r.lens_v[k] * scale;
        r.lens_u[k] = right[k];
        r.pos[k] = eye[k];
    }
    r.offset = offset; r.aperture = aperture; r.focus = focus;
    r.offset_over_focus = aperture > 0 ? offset / focus : 0.0;
    if ((rc = cam_check_fields(r, what))) return rc;
    *out = r;
    return APT_OK;
}

int apt_camera_check_host(const apt_camera *cam) {
    apt::clear_error();
    if (!cam) return set_error(APT_ERR_ARG, "%s: camera is null", "apt_camera_check_host");
    if (cam->struct_size != sizeof(apt_camera)) return set_error(APT_ERR_STRUCT, "%s: apt_camera.struct_size mismatch", "apt_camera_check_host");
    return cam_check_fields(*cam, "apt_camera_check_host");
}

int apt_context_set_camera(apt_context *ctx, const apt_camera *cam) {
    apt::clear_error();
    if (!ctx) return set_error(APT_ERR_ARG, "%s: context is null", "apt_context_set_camera");
    if (cam) {
        if (cam->struct_size != sizeof(apt_camera)) return set_error(APT_ERR_STRUCT, "%s: apt_camera.struct_size mismatch", "apt_context_set_camera");
        const int rc = cam_check_fields(*cam, "apt_context_set_camera");
        if (rc) return rc;
    }
    ctx->set_camera(cam);
    return APT_OK;
}

int apt_set_camera(const apt_camera *cam) { return apt_context_set_camera(&apt::default_context(), cam); }

} // extern "C"

// ---- environment (include/render_mi355x.h "environment"): the record's host helpers, in the manner of the camera's.
namespace {
// The refusals of apt_environment_check_host, struct_size aside.
int env_check_fields(const apt_environment &e, const char *what) {
    if (e.flags & ~(uint32_t)APT_ENV_SAMPLE_SUN) return set_error(APT_ERR_ARG, "%s: environment: unknown flag bits", what);
    const float *rad[3] = {e.horizon, e.zenith, e.sun_radiance};
    for (const float *r : rad)
        for (int k = 0; k < 3; ++k)
            if (!(std::isfinite(r[k]) && r[k] >= 0.0f)) return set_error(APT_ERR_ARG, "%s: environment: a radiance is negative or not finite", what);
    if (!(e.sun_omc >= 0.0f && e.sun_omc <= 1.0f)) return set_error(APT_ERR_ARG, "%s: environment: sun_omc must lie in [0, 1]", what);
    if (!(std::isfinite(e.sun_dir[0]) && std::isfinite(e.sun_dir[1]) && std::isfinite(e.sun_dir[2])))
        return set_error(APT_ERR_ARG, "%s: environment: sun_dir is not finite", what);
    if (e.sun_omc > 0.0f) {
        const double x = e.sun_dir[0], y = e.sun_dir[1], z = e.sun_dir[2];
        double l2 = x * x;
        l2 = l2 + y * y;
        l2 = l2 + z * z;
        if (!(fabs(l2 - 1.0) <= 0x1p-20)) return set_error(APT_ERR_ARG, "%s: environment: sun_dir must have unit length (squared length within 2^-20 of 1)", what);
    }
    return APT_OK;
}
} // namespace

extern "C" {

int apt_environment_build_host(const double horizon[3], const double zenith[3], const double sun_dir[3], const double sun_radiance[3],
                               double sun_omc, uint32_t flags, apt_environment *out) {
    apt::clear_error();
    const char *what = "apt_environment_build_host";
    if (!horizon || !zenith || !sun_dir || !sun_radiance || !out) return set_error(APT_ERR_ARG, "%s: horizon/zenith/sun_dir/sun_radiance/out must be non-null", what);
    if (out->struct_size != sizeof(apt_environment)) return set_error(APT_ERR_STRUCT, "%s: apt_environment.struct_size mismatch", what);
    if (!(cam_finite3(horizon) && cam_finite3(zenith) && cam_finite3(sun_dir) && cam_finite3(sun_radiance) && std::isfinite(sun_omc)))
        return set_error(APT_ERR_ARG, "%s: an input is not finite", what);
    apt_environment r;
    memset(&r, 0, sizeof r);
    r.struct_size = sizeof r;
    r.flags = flags;
    double w[3] = {sun_dir[0], sun_dir[1], sun_dir[2]};
    if (sun_omc > 0) {
        const double n = apt::norm3(sun_dir[0], sun_dir[1], sun_dir[2]);
        if (!(n >= apt::kCamMinNorm)) return set_error(APT_ERR_ARG, "%s: sun_dir must be non-zero (norm >= 2^-30) when sun_omc > 0", what);
        for (int k = 0; k < 3; ++k) w[k] = sun_dir[k] / n;
    }
    for (int k = 0; k < 3; ++k) {
        r.horizon[k] = (float)horizon[k]; r.zenith[k] = (float)zenith[k];
        r.sun_dir[k] = (float)w[k]; r.sun_radiance[k] = (float)sun_radiance[k];
    }
    r.sun_omc = (float)sun_omc;
    const int rc = env_check_fields(r, what);
    if (rc) return rc;
    *out = r;
    return APT_OK;
}

int apt_environment_check_host(const apt_environment *env) {
    apt::clear_error();
    if (!env) return set_error(APT_ERR_ARG, "%s: environment is null", "apt_environment_check_host");
    if (env->struct_size != sizeof(apt_environment)) return set_error(APT_ERR_STRUCT, "%s: apt_environment.struct_size mismatch", "apt_environment_check_host");
    return env_check_fields(*env, "apt_environment_check_host");
}

int apt_context_set_environment(apt_context *ctx, const apt_environment *env) {
    apt::clear_error();
    if (!ctx) return set_error(APT_ERR_ARG, "%s: context is null", "apt_context_set_environment");
    if (env) {
        if (env->struct_size != sizeof(apt_environment)) return set_error(APT_ERR_STRUCT, "%s: apt_environment.struct_size mismatch", "apt_context_set_environment");
        const int rc = env_check_fields(*env, "apt_context_set_environment");
        if (rc) return rc;
    }
    ctx->set_environment(env);
    return APT_OK;
}

int apt_set_environment(const apt_environment *env) { return apt_context_set_environment(&apt::default_context(), env); }

} // extern "C"

// ---- film (include/render_mi355x.h "film"): the pass seed, the curve table, the resolve's CPU twin and the PFM writer.
namespace apt {
// What both resolve forms refuse, in the header's order; the pointers are the entry's own.
int film_resolve_check(const apt_film_resolve *r, const void *film, const void *table, const void *out, const void *u8, const char *what) {
    if (!r || !film || !table) return set_error(APT_ERR_ARG, "%s: r/film/table must be non-null", what);
    if (r->struct_size != sizeof(apt_film_resolve)) return set_error(APT_ERR_STRUCT, "%s: apt_film_resolve.struct_size mismatch", what);
    if (!out && !u8) return set_error(APT_ERR_ARG, "%s: out and u8 are both null: nothing to write", what);
    if (r->passes == 0 || r->passes > (1u << 24)) return set_error(APT_ERR_ARG, "%s: passes must lie in [1, 2^24]", what);
    if (r->tonemap > (uint32_t)APT_TONEMAP_REINHARD) return set_error(APT_ERR_ARG, "%s: unknown tone operator", what);
    if (!(std::isfinite(r->exposure) && r->exposure >= 0.0f && std::isfinite(r->inv_white2) && r->inv_white2 >= 0.0f))
        return set_error(APT_ERR_ARG, "%s: exposure / inv_white2 must be finite and not negative", what);
    return APT_OK;
}
} // namespace apt

extern "C" {

uint64_t apt_film_pass_seed(uint64_t seed, uint32_t pass) {
    return pass == 0 ? seed : apt::splitmix64(seed ^ apt::splitmix64((uint64_t)pass ^ APT_FILM_PASS_SALT));
}

int apt_film_curve_host(uint32_t curve, float table[256]) {
    apt::clear_error();
    if (!table) return set_error(APT_ERR_ARG, "%s: table must be non-null", "apt_film_curve_host");
    if (curve > (uint32_t)APT_CURVE_SRGB) return set_error(APT_ERR_ARG, "%s: unknown curve", "apt_film_curve_host");
    table[0] = 0.0f;
    for (int k = 1; k < 256; ++k) {
        const double e = ((double)k - 0.5) / 255.0;
        const double v = curve == (uint32_t)APT_CURVE_LINEAR ? e : (e <= 0.04045 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4));
        table[k] = (float)v;
    }
    return APT_OK;
}

// The resolve kernel's CPU twin: film_ops.h's film_tone and film_code for every value, as film.hip's kernel runs them.
int apt_film_resolve_host(const apt_film_resolve *r, const float *film, uint64_t pixel_count, const float *table, float *out, uint8_t *u8) {
    apt::clear_error();
    const int rc = apt::film_resolve_check(r, film, table, out, u8, "apt_film_resolve_host");
    if (rc) return rc;
    const apt::FilmTone tone = {(float)r->passes, r->exposure, r->inv_white2, r->tonemap == (uint32_t)APT_TONEMAP_REINHARD ? 1u : 0u};
    for (uint64_t c = 0; c < 3; ++c)
        for (uint64_t i = 0; i < pixel_count; ++i) {
            const float y = apt::film_tone(film[c * pixel_count + i], tone);
            if (out) out[c * pixel_count + i] = y;
            if (u8) u8[i * 3 + c] = (uint8_t)apt::film_code(table, y);
        }
    return APT_OK;
}

int apt_write_pfm(const char *path, uint32_t width, uint32_t height, const float *planes) {
    apt::clear_error();
    if (!path || !planes || !width || !height) return set_error(APT_ERR_ARG, "apt_write_pfm: path/planes must be non-null, width/height non-zero%s");
    FILE *f = fopen(path, "wb");
    if (!f) return set_error(APT_ERR_IO, "apt_write_pfm: cannot open %s", path);
    fprintf(f, "PF\n%u %u\n-1.0\n", width, height);
    const uint64_t np = (uint64_t)width * height;
    std::vector<uint8_t> row((size_t)width * 12);
    for (uint32_t y = 0; y < height; ++y) {            // PFM rows run bottom to top, and so does y: no flip
        for (uint32_t x = 0; x < width; ++x)
            for (uint64_t c = 0; c < 3; ++c) {
                uint32_t bits;
                memcpy(&bits, &planes[c * np + (uint64_t)x * height + y], 4);
                uint8_t *o = &row[((size_t)x * 3 + c) * 4];   // little-endian whatever the host is
                o[0] = (uint8_t)bits; o[1] = (uint8_t)(bits >> 8); o[2] = (uint8_t)(bits >> 16); o[3] = (uint8_t)(bits >> 24);
            }
        fwrite(row.data(), 1, row.size(), f);
    }
    return fclose(f) == 0 ? APT_OK : set_error(APT_ERR_IO, "apt_write_pfm: write to %s failed", path);
}

} // extern "C"
