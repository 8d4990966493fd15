// pt_materials.h -- the material kernels (include/render_mi355x.h "per-sphere materials": smallpt's DIFF / SPEC / REFR with emitted
// radiance), included by materials.hip only.  Same scene forms as the mirror kernels -- the 8-sphere scene with its geometry in SGPRs,
// any scene through LDS tiles (tile_scan, pt_trace.h, shared with dyn_segment), any scene behind the uniform grid (mat_hit_grid: a
// per-lane walk of the grid's item ranges, grid_walk_cells of pt_trace.h, shared with grid_segment) -- and render_frame_kernel's frame
// skeleton: the lane mapping, camera and decode come from pt_frame.h, the pairwise-leaf accumulation is written out as in render_frame_kernel (pt_frame.h
// says why); only the body of one sample differs.  Every fp32 operation is the one the header specifies, in its order
// (-ffp-contract=off): tests/materials_ref.py restates it and the GPU tests compare bit for bit.
#pragma once
#include "pt_frame.h"   // FrameArgs, frame_lane, park_camera, frame_decode; pt_trace.h
#include "pt_camera.h"  // CameraEx, camera_ray_ex: a context's camera (kMatCamera)
#include <type_traits>

namespace {

constexpr uint64_t kMatKeySalt = 0x6A09E667F3BCC909ull;
constexpr uint64_t kNeeKeySalt = 0xBB67AE8584CAA73Bull;   // APT_FLAG_NEE's stream: a third one, next to the bounce's and roulette's
constexpr int kMatNee = 4;      // APT_FLAG_NEE in the kernels' scene-form template argument (kScene8 / kSceneTiles / kSceneGrid are 0 / 1 / 2)
static_assert((kMatNee & (kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatNee must be a bit of its own");
constexpr uint64_t kLightKeySalt = 0x3C6EF372FE94F82Bull; // the light table's selection draw: a fourth stream
constexpr uint64_t kSunKeySalt = APT_ENV_SUN_SALT;        // the environment's sun sample: one more
constexpr int kMatLights = 8;   // a light table (the *_lights entries) in the same template argument; never together with kMatNee
static_assert((kMatLights & (kMatNee | kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatLights must be a bit of its own");
// How a kernel samples lights (LM, from the two bits above): not at all, the one sphere light_index, one light of a table per bounce.
constexpr int kLmNone = 0, kLmNee = 1, kLmTable = 2;
constexpr int mat_light_mode(int scn) { return (scn & kMatLights) ? kLmTable : ((scn & kMatNee) ? kLmNee : kLmNone); }
constexpr int kMatCamera = 16;  // a context's camera (apt_context_set_camera) in the same template argument, frame kernels only: ray-generate in its general form
static_assert((kMatCamera & (kMatLights | kMatNee | kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatCamera must be a bit of its own");
constexpr int kMatGloss = 32;   // APT_FLAG_GLOSS in the same template argument: the table may hold APT_MAT_GLOSS words (the caller's statement)
static_assert((kMatGloss & (kMatCamera | kMatLights | kMatNee | kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatGloss must be a bit of its own");
constexpr int kMatEnv = 64;     // a context's environment (apt_context_set_environment) in the same template argument: only then is the kernels' MatEnv read
static_assert((kMatEnv & (kMatGloss | kMatCamera | kMatLights | kMatNee | kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatEnv must be a bit of its own");
constexpr int kMatFilm = 128;   // the film entries (include/render_mi355x.h "film") in the same template argument, frame kernels with kMatEnv only: the tail is frame_film
static_assert((kMatFilm & (kMatEnv | kMatGloss | kMatCamera | kMatLights | kMatNee | kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatFilm must be a bit of its own");
constexpr int kMatMis = 256;    // APT_FLAG_MIS in the same template argument (mis.hip: with kMatEnv, kMatGloss and a light mode): GLOSS hits sample the lights too
static_assert((kMatMis & (kMatFilm | kMatEnv | kMatGloss | kMatCamera | kMatLights | kMatNee | kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatMis must be a bit of its own");
constexpr int kMatList = 512;   // APT_FLAG_PIXEL_LIST in the same template argument (film_list.hip: with kMatFilm): the lane's pixel comes from a list, FrameArgs::fb_u8 its address
static_assert((kMatList & (kMatMis | kMatFilm | kMatEnv | kMatGloss | kMatCamera | kMatLights | kMatNee | kScene8 | kSceneTiles | kSceneGrid)) == 0, "kMatList must be a bit of its own");
constexpr uint32_t kMatEnvFilmAdd = 2u;   // MatEnv::gloss of a kMatFilm launch, next to bit 0: pass > 0, the tail adds to the film instead of storing
constexpr int mat_scene_of(int scn) { return scn & ~(kMatNee | kMatLights | kMatCamera | kMatGloss | kMatEnv | kMatFilm | kMatMis | kMatList); }
// The contract's limit (include/render_mi355x.h "camera"): a frame with a camera takes a plan of at most this many leaves.  Nothing in
// the kernels needs it any more; lifting it is a feature with its own tests above 4199 samples, not part of any clean-up.
constexpr uint32_t kCamMaxLeaves = 44;
constexpr int kMatTab = 24;     // 8-sphere LDS table: geometry [0, 8), albedo [8, 16), emission [16, 24)
constexpr int kMatTabGloss = 32; // with kMatGloss: .x of [24, 32) is alpha (0 for a sphere that is not gloss).  Both sizes are one 1280-byte LDS granule
constexpr int mat_tab_entries(int scn) { return (scn & kMatGloss) ? kMatTabGloss : kMatTab; }
// A material word as the kernels read it with APT_FLAG_GLOSS: -> the code (0..2 as they are, 3 for a well-formed gloss word, 15 = bad
// for everything else) and q (bits 8..23; alpha = q * 2^-16, exact).
__device__ __forceinline__ uint32_t mat_gloss_code(uint32_t w, uint32_t &q) {
    q = (w >> 8) & 0xFFFFu;
    const bool gloss = (w & 0xFFu) == (uint32_t)APT_MAT_GLOSS && q != 0u && (w >> 24) == 0u;
    return w <= (uint32_t)APT_MAT_REFR ? w : (gloss ? (uint32_t)APT_MAT_GLOSS : 15u);
}

struct MatPath {
    float ox, oy, oz, dx, dy, dz;
    float tx, ty, tz;           // throughput T
    float lx, ly, lz;           // radiance L gathered so far
    int skip;                   // sphere the next segment does not test, or -1
    bool live;                  // the path has not ended (miss or bad material code)
};

// APT_FLAG_NEE ("direct light sampling" in the header).  The light's record, read once per kernel from wave-uniform addresses
// (scalar loads: it lives in SGPRs), and what a DIFF hit hands to the shadow test that follows the bounce.
struct MatLight {
    float cx, cy, cz, r2;
    float ex, ey, ez;
    int idx;
};
struct MatShadow {
    float dx, dy, dz;           // l, the sampled direction towards the light
    float w;                    // cosl * (2 * omc), times invp[i] with a light table
    bool want;                  // cosl > 0: the shadow segment is traced
    int g;                      // light table: the sphere that was sampled (set with `want`)
};
// The material kernels' own argument: TraceArgs as every helper of pt_trace.h reads it (report_status, count_traced, grid_stats,
// russian_roulette, load_grid_header take `ta`), and next to it what only these kernels read.
struct MatKernelArgs {
    TraceArgs ta;               // refill_lanes, emission, gain, grid_walk: 0, not read here
    const uint32_t *lights;     // the light table of the *_lights entries (device), or null
};
static_assert(std::is_trivially_copyable<MatKernelArgs>::value && std::is_trivially_copyable<CameraTail>::value, "kernel arguments are copied as bytes");
static_assert(offsetof(MatKernelArgs, ta) == 0, "the helpers that take TraceArgs see the layout they always saw");
// The environment ("environment" in the header) as the kMatEnv kernels read it: a kernel argument of its own, so wave-uniform and
// fetched by scalar loads where it is used.  gloss: the launch carries APT_FLAG_GLOSS -- the environment kernels are always the gloss
// instantiations, and without the flag a well-formed gloss word is the bad code it is in the kernels without kMatGloss.
struct MatEnv {
    float horizon[3], zenith[3];
    float sun[3], sun_rad[3];   // sun_dir, sun_radiance
    float omc;                  // sun_omc; 0: no sun
    uint32_t sample;            // APT_ENV_SAMPLE_SUN and omc > 0: DIFF hits sample the sun
    uint32_t gloss;
};
struct MatNoEnv {};             // what the kernels without kMatEnv take in its place: nothing
template <int SCN> using MatEnvArg = std::conditional_t<(SCN & kMatEnv) != 0, MatEnv, MatNoEnv>;
static_assert(std::is_trivially_copyable<MatEnv>::value, "kernel arguments are copied as bytes");
// The sun's part of a bounce's state (kMatEnv only): the stream key, `sampled_sun`, and what a DIFF hit hands to the sun's shadow test.
struct MatSun {
    uint64_t key;
    bool sampled;
    bool may;                   // this bounce may sample: E samples and d + 1 < depth (wave-uniform)
    MatShadow sh;               // g is not read
};
// APT_FLAG_MIS's part of a path's state (kMatMis only; "Multiple importance sampling" in the header): the last sampling bounce was a
// GLOSS one, and the density p_b under which it drew its direction.  g: G1(l) of the current GLOSS bounce, which multiplies T only after
// the bounce's shadow segment has used T (1 for every other bounce).
struct MatMis {
    float pb;
    bool gl;
    float g;
};
constexpr float kMisPi = 0x1.921fb6p+1f, kMisTwoPi = 0x1.921fb6p+2f;   // RN(pi), RN(2 * pi)
template <int LM>
__device__ __forceinline__ MatLight load_mat_light(const float *__restrict__ sph, const TraceArgs &ta) {
    MatLight lt = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1};
    if (LM == kLmNee) {         // the entry checked 0 <= light < ns
        const size_t ns = ta.ns, g = (size_t)ta.light;
        lt.r2 = sph[g]; lt.cx = sph[ns + g]; lt.cy = sph[2 * ns + g]; lt.cz = sph[3 * ns + g];
        lt.ex = sph[4 * ns + g]; lt.ey = sph[5 * ns + g]; lt.ez = sph[6 * ns + g];
        lt.idx = ta.light;
    }
    return lt;
}

// The light table of the *_lights entries ("several lights" in the header; the layout: pt_core.h kLightsMagic; MatKernelArgs::lights).
// The head is read once per kernel by a scalar load and checked before anything else of the table is (mat_lights_header); what the
// struct keeps is wave-uniform and lives in SGPRs.  cdf / idx / invp are searched and gathered per lane: the lanes of a wave choose
// different lights.
struct MatTable {
    const uint32_t *p;          // the table; its arrays follow the head: idx(), cdf(), invp(), bits()
    uint32_t n, bits0;          // bits0: spheres 0..31 of the bitset (all of it for the 8-sphere form)
    __device__ __forceinline__ const uint32_t *idx() const { return p + kLightsHead; }
    __device__ __forceinline__ const float *cdf() const { return reinterpret_cast<const float *>(p + kLightsHead) + n; }
    __device__ __forceinline__ const float *invp() const { return reinterpret_cast<const float *>(p + kLightsHead) + 2 * (size_t)n; }
    __device__ __forceinline__ const uint32_t *bits() const { return p + kLightsHead + 3 * (size_t)n; }
    const float *sph;           // the sphere planes and, for the 8-sphere form, their LDS copy: where a chosen light's record is gathered
    const float4 *tab8;
    uint32_t ns;
};
// -> false: the table is not one for this scene (magic, num_spheres, 1 <= n <= num_spheres).  It is not read further, the kernel writes
// nothing and says APT_DEV_LIGHTS_MISMATCH.  Uniform over the launch, like mat_grid_header.
template <int LM>
__device__ __forceinline__ bool mat_lights_header(const MatKernelArgs &ka, const float *__restrict__ sph, const float4 *tab8, MatTable &tb) {
    if (LM != kLmTable) return true;
    const TraceArgs &ta = ka.ta;
    const uint32_t *p = ka.lights;
    uint32_t hw[kLightsHead];
#if defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
    u32x16 w;
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(w) : "s"(p) : "memory");
#pragma unroll
    for (int i = 0; i < 16; ++i) hw[i] = w[i];
#else
    __builtin_memcpy(hw, p, sizeof hw);
#endif
    const uint32_t n = hw[2];
    if (hw[0] == kLightsMagic && hw[1] == ta.ns && n >= 1u && n <= ta.ns) {
        tb.p = p; tb.n = n; tb.bits0 = hw[4];
        tb.sph = sph; tb.tab8 = tab8; tb.ns = ta.ns;
        return true;
    }
    report_status(ta, APT_DEV_LIGHTS_MISMATCH);
    return false;
}
// Is sphere k (0 <= k < num_spheres) listed: one load; the 8-sphere form answers from the SGPR.
template <int SC>
__device__ __forceinline__ bool mat_light_listed(const MatTable &tb, int k) {
    const uint32_t w = SC == kScene8 ? tb.bits0 : tb.bits()[(uint32_t)k >> 5];
    return (w >> ((uint32_t)k & 31u)) & 1u;
}
// The first entry with u < cdf[i]: cdf is strictly increasing and ends with 1 > u, so it exists.  A branchless lower bound, one
// dependent load per halving (none for one light); the trip count is wave-uniform, the addresses are the lane's own.
__device__ __forceinline__ uint32_t mat_light_pick(const MatTable &tb, float u) {
    uint32_t base = 0;
    for (uint32_t len = tb.n; len > 1u;) {
        const uint32_t half = len >> 1;
        if (tb.cdf()[base + half - 1u] <= u) base += half;
        len -= half;
    }
    return base;
}
// Centre and r2 of sphere g, per lane (the emission is fetched only once the light turns out visible: mat_light_emission).
template <int SC>
__device__ __forceinline__ void mat_light_geometry(const MatTable &tb, int g, MatLight &lt) {
    if (SC == kScene8) {
        const float4 c = tb.tab8[g];
        lt.cx = c.x; lt.cy = c.y; lt.cz = c.z; lt.r2 = c.w;
    } else {
        const size_t ns = tb.ns, i = (size_t)g;
        lt.r2 = tb.sph[i]; lt.cx = tb.sph[ns + i]; lt.cy = tb.sph[2 * ns + i]; lt.cz = tb.sph[3 * ns + i];
    }
    lt.idx = g;
}
template <int SC>
__device__ __forceinline__ float4 mat_light_emission(const MatTable &tb, int g) {
    if (SC == kScene8) return tb.tab8[16 + g];
    const size_t ns = tb.ns, i = (size_t)g;
    return make_float4(tb.sph[4 * ns + i], tb.sph[5 * ns + i], tb.sph[6 * ns + i], 0.0f);
}

__device__ __forceinline__ uint64_t light_path_key(uint64_t seed, uint64_t path) { return splitmix64(seed ^ splitmix64(path) ^ kLightKeySalt); }
__device__ __forceinline__ uint64_t nee_path_key(uint64_t seed, uint64_t path) { return splitmix64(seed ^ splitmix64(path) ^ kNeeKeySalt); }
__device__ __forceinline__ uint64_t mat_path_key(uint64_t seed, uint64_t path) { return splitmix64(seed ^ splitmix64(path) ^ kMatKeySalt); }
__device__ __forceinline__ uint64_t sun_path_key(uint64_t seed, uint64_t path) { return splitmix64(seed ^ splitmix64(path) ^ kSunKeySalt); }
__device__ __forceinline__ void mat_uniforms(uint64_t mkey, uint32_t d, float &u1, float &u2) {
    const uint64_t h = splitmix64(mkey + 0x9E3779B97F4A7C15ull * (uint64_t)(d + 1u));
    u1 = (float)(uint32_t)(h >> 40) * 0x1p-24f;
    u2 = (float)((uint32_t)(h >> 16) & 0xFFFFFFu) * 0x1p-24f;
}

// (sin, cos) of 2*pi*u1 for u1 = m * 2^-24: quadrant and fraction of u1 * 4, one fixed polynomial pair, swap / negate.
__device__ __forceinline__ void mat_sincos(float u1, float &sn, float &cs) {
    const float x = u1 * 4.0f;
    const int q = (int)x;
    const float f = x - (float)q;
    const float z = f * f;
    float p = APT_MAT_S11;
    p = APT_MAT_S9 + z * p; p = APT_MAT_S7 + z * p; p = APT_MAT_S5 + z * p; p = APT_MAT_S3 + z * p; p = APT_MAT_S1 + z * p;
    const float s = f * p;
    float c = APT_MAT_C12;
    c = APT_MAT_C10 + z * c; c = APT_MAT_C8 + z * c; c = APT_MAT_C6 + z * c; c = APT_MAT_C4 + z * c; c = APT_MAT_C2 + z * c;
    c = 1.0f + z * c;
    const float a = (q & 1) ? c : s, b = (q & 1) ? s : c;
    sn = (q >= 2) ? -a : a;
    cs = (q == 1 || q == 2) ? -b : b;
}

// The thin lens's point in lens coordinates (include/render_mi355x.h "camera"): a uniform point of the disc of radius `aperture`, fp32,
// from the lens's own stream -- one draw per path -- with the DIFF block's sqrt and polynomial.
__device__ __forceinline__ void cam_lens_point(uint64_t seed, uint64_t path, float aperture, float &lx, float &ly) {
    float v1, v2;
    mat_uniforms(splitmix64(seed ^ splitmix64(path) ^ kLensKeySalt), 0u, v1, v2);
    const float r = sqrtf(v1);
    float sn, cs;
    mat_sincos(v2, sn, cs);
    lx = (cs * r) * aperture;
    ly = (sn * r) * aperture;
}
// The extended camera, parked in LDS like the 14 doubles of park_camera: those from FrameArgs, the tail from the kernel's own argument.
__device__ __forceinline__ void park_camera_ex(CameraEx &cam, const FrameArgs &fa, const CameraTail &ct) {
    park_camera(cam.base, fa);
    if (threadIdx.x < kCamTailWords) reinterpret_cast<uint32_t *>(&cam.t)[threadIdx.x] = reinterpret_cast<const uint32_t *>(&ct)[threadIdx.x];
}

// The written-out fp32 forms of the blocks below (-ffp-contract=off: every product and sum rounds on its own): the dot product as
// ((0 + ax*bx) + ay*by) + az*bz, and v / |v| as that dot of v with itself, an IEEE sqrtf and three divides.
__device__ __forceinline__ float mat_dot(float ax, float ay, float az, float bx, float by, float bz) {
    float s = 0.0f + ax * bx;
    s = s + ay * by;
    return s + az * bz;
}
__device__ __forceinline__ void mat_normalise(float x, float y, float z, float &nx, float &ny, float &nz) {
    const float l = sqrtf(mat_dot(x, y, z, x, y, z));
    nx = x / l; ny = y / l; nz = z / l;
}
// Duff et al. 2017: the orthonormal basis (t, b) of the unit vector n, branchless.
__device__ __forceinline__ void mat_basis(float nx, float ny, float nz, float &tx, float &ty, float &tz, float &bx, float &by, float &bz) {
    const float sg = copysignf(1.0f, nz);
    const float a = -1.0f / (sg + nz);
    const float b = (nx * ny) * a;
    tx = 1.0f + ((sg * nx) * nx) * a; ty = sg * b; tz = (-sg) * nx;
    bx = b; by = sg + (ny * ny) * a; bz = -ny;
}

// G1 of the separable Smith term for a frame direction of z component z (a2 = alpha * alpha): the GLOSS block's own operations.
__device__ __forceinline__ float mat_g1(float a2, float z) { return (2.0f * z) / (z + sqrtf(a2 + (1.0f - a2) * (z * z))); }
// The GGX density of the unit half vector m in the frame, without the cancellation of (m.z^2)(a2 - 1) + 1: k = (m.x^2 + m.y^2) + a2 *
// m.z^2 >= ~a2 > 0, D = a2 / ((pi * k) * k) <= ~1 / (pi * a2) <= 2^32 / pi.
__device__ __forceinline__ float mat_ggx_d(float a2, float mx, float my, float mz) {
    const float k = (mx * mx + my * my) + a2 * (mz * mz);
    return a2 / ((kMisPi * k) * k);
}
// The light-sampling density of a sphere of r2 seen from a point at squared distance d2 > r2, chosen with probability P:
// "Direct light sampling"'s x, cmax and omc, then P / (2 * pi * omc).
__device__ __forceinline__ float mat_light_pdf(float r2, float d2, float P) {
    const float x = r2 / d2;
    const float cmax = sqrtf(1.0f - x);
    const float omc = x / (1.0f + cmax);
    return P / (kMisTwoPi * omc);
}
// P of the table entry that lists sphere k: cdf[i] - cdf[i - 1], exact (both are multiples of 2^-24).  The table lists distinct spheres
// in the caller's order, so the entry is found by a scan; only a path that hits a listed light right after a GLOSS sampling bounce asks.
__device__ __forceinline__ float mat_light_prob(const MatTable &tb, int k) {
    float P = 0.0f;
    for (uint32_t i = 0; i < tb.n; ++i)
        if (tb.idx()[i] == (uint32_t)k) P = tb.cdf()[i] - (i ? tb.cdf()[i - 1u] : 0.0f);
    return P;
}

// A path's stream keys, made once per path: the bounce's, APT_FLAG_NEE's direction (LM != kLmNone), the table's selection (kLmTable).
struct MatKeys {
    uint64_t bounce, nee, pick;
};
// "Direct light sampling"'s sample step for a sphere light of r2 at w0 = c - h, d2 = dot(w0, w0) > r2: a direction l of the light's cone
// from the nkey stream, and omc = 1 - cos_max.  The DIFF hits' and, with APT_FLAG_MIS, the GLOSS hits' (one hit per bounce: one draw).
__device__ __forceinline__ void mat_cone_sample(float r2, float wx0, float wy0, float wz0, float d2, uint64_t nkey, uint32_t d, float &lx,
                                                float &ly, float &lz, float &omc) {
    const float x = r2 / d2;
    const float cmax = sqrtf(1.0f - x);
    omc = x / (1.0f + cmax);                                  // 1 - cos_max
    float v1, v2;
    mat_uniforms(nkey, d, v1, v2);
    const float cos_a = 1.0f - v1 * omc;
    const float sin_a = sqrtf(1.0f - cos_a * cos_a);
    float sp, cp;
    mat_sincos(v2, sp, cp);
    const float dl = sqrtf(d2);
    const float wx = wx0 / dl, wy = wy0 / dl, wz = wz0 / dl;
    float ax, ay, az, ex, ey, ez;
    mat_basis(wx, wy, wz, ax, ay, az, ex, ey, ez);
    const float ca = cp * sin_a, sa = sp * sin_a;
    const float qx = (ax * ca + ex * sa) + wx * cos_a, qy = (ay * ca + ey * sa) + wy * cos_a, qz = (az * ca + ez * sa) + wz * cos_a;
    mat_normalise(qx, qy, qz, lx, ly, lz);
}
template <int LM>
__device__ __forceinline__ MatKeys mat_path_keys(uint64_t seed, uint64_t path) {
    return MatKeys{mat_path_key(seed, path), LM ? nee_path_key(seed, path) : 0, LM == kLmTable ? light_path_key(seed, path) : 0};
}
// What a segment found: the nearest root and its sphere (k < 0: none; the record is then sphere 0's and is not shaded), that sphere's
// record, its material code (with GL: mat_gloss_code's) and, for a gloss sphere, its roughness.  The colours are three floats: a float4
// member makes the 8-sphere form read the unused fourth word of its LDS entries.
struct MatRgb {
    float x, y, z;
};
__device__ __forceinline__ MatRgb mat_rgb(float4 v) { return MatRgb{v.x, v.y, v.z}; }
struct MatHit {
    float t;
    int k;
    float4 geo;                 // geo.w: r2 in the 8-sphere form only
    MatRgb alb, em;
    uint32_t code;
    float alpha;                // GL only
};
// The bounce after the hit `h` (h.code is APT_MAT_SPEC / DIFF / REFR, with GL also GLOSS: checked by the caller): the light step, the
// throughput, the new direction and origin, the skip sphere.  The DIFF, GLOSS and REFR blocks are per-lane branches: exec-masked, skipped
// by a wave with none of its lanes in them.  They stay in this one function, and the light state stays two variables: as functions of
// their own the blocks cost four instantiations a wave of occupancy (profiles/mat_record_isa.txt), as one variable the state made the
// 8-sphere APT_FLAG_NEE frame slower than the parent's by more than the parent's spread (profiles/mat_record_ab_state_merged.json).
// A bounce samples a light only at a DIFF hit that may (`may`: a light mode and not the last bounce; wave-uniform); it then draws the
// direction and weight of its shadow segment -> sh.  The light step leaves out the emission of a light the previous bounce sampled: that
// bounce's shadow segment has counted it.
//   kLmNee    the one light lt.  `sampled`: the previous bounce drew a direction towards it (h was strictly outside it).
//   kLmTable  the hit first picks ONE listed light per lane (key.pick) and samples that one if the predicate S holds for it -- it is not
//             the sphere we stand on and h is strictly outside it --; the bounce counts as sampling either way and remembers its sphere
//             (kprev; -1: the previous bounce did not sample).  The light step leaves out a LISTED sphere for which S held at the
//             previous bounce: the same fp32 chain on the same values (s.o is that bounce's h, h.geo the record the sample gathered).
// With LM == kLmNone lt, tb, sampled, kprev and sh are not read and nothing of this remains in the code.
// GLOSS: a rough conductor of roughness h.alpha (the header's GLOSS block: visible normals of the GGX distribution in their
// spherical-cap form, weight G1(l)).  A direction drawn below the horizon ends the path (s.live).  It does not sample, like SPEC.
// EV (kMatEnv): every hit clears su.sampled, and a DIFF hit that may (su.may) draws the sun's shadow segment -> su.sh, "Direct light
// sampling"'s arithmetic with w = sun_dir and omc = sun_omc; without EV env and su are not read.
// MI (kMatMis; "Multiple importance sampling" in the header): a GLOSS hit that may is a sampling bounce too: it picks and samples a
// light as a DIFF hit does -> sh, with the balance-heuristic weight, and leaves its own density in mi; the light step weights the
// emission of a light that such a bounce could have sampled instead of leaving it out.  Without MI mi is not read.
template <int LM, int SC, bool GL, bool EV = false, bool MI = false, class ENV = MatNoEnv>
__device__ __forceinline__ void mat_shade(MatPath &s, const MatHit &h, MatKeys key, uint32_t d, const MatLight &lt, bool may, bool &sampled,
                                          MatShadow &sh, const MatTable &tb, int &kprev, const ENV &env, MatSun &su, MatMis &mi) {
    const int k = h.k;
    float hx = s.dx * h.t, hy = s.dy * h.t, hz = s.dz * h.t;
    hx = s.ox + hx; hy = s.oy + hy; hz = s.oz + hz;
    float nx, ny, nz;
    mat_normalise(hx - h.geo.x, hy - h.geo.y, hz - h.geo.z, nx, ny, nz);
    bool counted = LM == kLmNee && sampled && k == lt.idx;
    if (LM == kLmTable && kprev >= 0) {                       // the previous bounce was a sampling bounce (that IS `sampled` here)
        if (k != kprev && mat_light_listed<SC>(tb, k)) {
            const float r2k = SC == kScene8 ? h.geo.w : tb.sph[(size_t)k];
            const float wx0 = h.geo.x - s.ox, wy0 = h.geo.y - s.oy, wz0 = h.geo.z - s.oz;
            counted = mat_dot(wx0, wy0, wz0, wx0, wy0, wz0) > r2k;
        }
    }
    if (!counted) { s.lx = s.lx + s.tx * h.em.x; s.ly = s.ly + s.ty * h.em.y; s.lz = s.lz + s.tz * h.em.z; }
    if constexpr (MI) {
        if (counted && mi.gl) {                               // the light a GLOSS bounce could have sampled: the BSDF strategy's share
            const float wx0 = h.geo.x - s.ox, wy0 = h.geo.y - s.oy, wz0 = h.geo.z - s.oz;   // (that bounce's w0, d2 and omc, bit for bit)
            const float r2k = LM == kLmNee ? lt.r2 : (SC == kScene8 ? h.geo.w : tb.sph[(size_t)k]);
            const float pl = mat_light_pdf(r2k, mat_dot(wx0, wy0, wz0, wx0, wy0, wz0), LM == kLmTable ? mat_light_prob(tb, k) : 1.0f);
            const float sum = mi.pb + pl;
            const float wb = (sum > 0.0f && sum < __builtin_inff()) ? mi.pb / sum : 1.0f;   // no finite positive sum: in full
            s.lx = s.lx + (s.tx * h.em.x) * wb; s.ly = s.ly + (s.ty * h.em.y) * wb; s.lz = s.lz + (s.tz * h.em.z) * wb;
        }
        mi.gl = false;
        mi.g = 1.0f;
    }
    if (LM == kLmNee) sampled = false;
    if (LM == kLmTable) kprev = -1;
    if constexpr (EV) su.sampled = false;
    s.tx = s.tx * h.alb.x; s.ty = s.ty * h.alb.y; s.tz = s.tz * h.alb.z;
    const float ddn = mat_dot(s.dx, s.dy, s.dz, nx, ny, nz);
    const bool into = ddn < 0.0f;
    bool outward = into;
    float ndx, ndy, ndz;
    if (h.code == APT_MAT_DIFF) {
        const float nlx = into ? nx : -nx, nly = into ? ny : -ny, nlz = into ? nz : -nz;
        float u1, u2;
        mat_uniforms(key.bounce, d, u1, u2);
        float sn, cs;
        mat_sincos(u1, sn, cs);
        const float r = sqrtf(u2);
        float tx, ty, tz, bx, by, bz;
        mat_basis(nlx, nly, nlz, tx, ty, tz, bx, by, bz);
        const float cr = cs * r, sr = sn * r, w = sqrtf(1.0f - u2);
        const float vx = (tx * cr + bx * sr) + nlx * w, vy = (ty * cr + by * sr) + nly * w, vz = (tz * cr + bz * sr) + nlz * w;
        mat_normalise(vx, vy, vz, ndx, ndy, ndz);
        MatLight chosen;                                      // kLmTable: the lane's light; kLmNee: lt itself
        const MatLight &cur = LM == kLmTable ? chosen : lt;
        float invp = 1.0f;
        if (LM == kLmTable && may) {
            float u, unused;
            mat_uniforms(key.pick, d, u, unused);
            const uint32_t i = mat_light_pick(tb, u);
            invp = tb.invp()[i];
            mat_light_geometry<SC>(tb, (int)min(tb.idx()[i], tb.ns - 1u), chosen);   // (the clamp: a table is trusted, an address is not)
            kprev = k;                                        // sampled, whatever follows
        }
        if (LM && may && k != cur.idx) {
            const float wx0 = cur.cx - hx, wy0 = cur.cy - hy, wz0 = cur.cz - hz;
            const float d2 = mat_dot(wx0, wy0, wz0, wx0, wy0, wz0);
            if (d2 > cur.r2) {                                // h strictly outside the light (false for NaN)
                float omc;
                mat_cone_sample(cur.r2, wx0, wy0, wz0, d2, key.nee, d, sh.dx, sh.dy, sh.dz, omc);
                const float cosl = mat_dot(sh.dx, sh.dy, sh.dz, nlx, nly, nlz);
                sh.w = cosl * (2.0f * omc);
                if (LM == kLmTable) { sh.w = sh.w * invp; sh.g = cur.idx; }
                sh.want = cosl > 0.0f;
                if (LM == kLmNee) sampled = true;
            }
        }
        if constexpr (EV) {
            if (su.may) {
                const float omc = env.omc, wx = env.sun[0], wy = env.sun[1], wz = env.sun[2];
                float v1, v2;
                mat_uniforms(su.key, d, v1, v2);
                const float cos_a = 1.0f - v1 * omc;
                const float sin_a = sqrtf(1.0f - cos_a * cos_a);
                float sp, cp;
                mat_sincos(v2, sp, cp);
                float ax, ay, az, ex, ey, ez;
                mat_basis(wx, wy, wz, ax, ay, az, ex, ey, ez);
                const float ca = cp * sin_a, sa = sp * sin_a;
                const float qx = (ax * ca + ex * sa) + wx * cos_a, qy = (ay * ca + ey * sa) + wy * cos_a, qz = (az * ca + ez * sa) + wz * cos_a;
                mat_normalise(qx, qy, qz, su.sh.dx, su.sh.dy, su.sh.dz);
                const float cosl = mat_dot(su.sh.dx, su.sh.dy, su.sh.dz, nlx, nly, nlz);
                su.sh.w = cosl * (2.0f * omc);
                su.sh.want = cosl > 0.0f;
                su.sampled = true;                            // whatever follows
            }
        }
    } else if (GL && h.code == (uint32_t)APT_MAT_GLOSS) {
        const float nlx = into ? nx : -nx, nly = into ? ny : -ny, nlz = into ? nz : -nz;
        float tx, ty, tz, bx, by, bz;
        mat_basis(nlx, nly, nlz, tx, ty, tz, bx, by, bz);
        const float wx = -s.dx, wy = -s.dy, wz = -s.dz;       // v = -d, in the frame (t, bt, nl)
        const float vx = mat_dot(wx, wy, wz, tx, ty, tz), vy = mat_dot(wx, wy, wz, bx, by, bz), vz = mat_dot(wx, wy, wz, nlx, nly, nlz);
        float sx, sy, sz;
        mat_normalise(h.alpha * vx, h.alpha * vy, vz, sx, sy, sz);   // the view direction of the stretched (alpha = 1) configuration
        float u1, u2;
        mat_uniforms(key.bounce, d, u1, u2);
        float sn, cs;
        mat_sincos(u1, sn, cs);
        const float z = (1.0f - u2) * (1.0f + sz) - sz;       // a uniform point of the spherical cap z > -s.z
        const float r2 = 1.0f - z * z;
        const float r = sqrtf(r2 > 0.0f ? r2 : 0.0f);
        float mx, my, mz;
        mat_normalise(h.alpha * (r * cs + sx), h.alpha * (r * sn + sy), z + sz, mx, my, mz);   // the half vector, stretched back
        const float vm2 = 2.0f * mat_dot(vx, vy, vz, mx, my, mz);
        const float lx = mx * vm2 - vx, ly = my * vm2 - vy, lz = mz * vm2 - vz;
        if (!(lz > 0.0f)) s.live = false;                     // below the horizon: the path ends here, L keeps its value
        const float a2 = h.alpha * h.alpha;
        const float g = (2.0f * lz) / (lz + sqrtf(a2 + (1.0f - a2) * (lz * lz)));   // G1(l), separable Smith
        if constexpr (MI) {
            mi.g = g;                                         // T *= g after the shadow segment (trace_mat)
            if (may) {                                        // a sampling bounce, also when the path ends here (l below the horizon): the
                                                              // light strategy's share must not depend on what the other strategy drew
                const float g1v = mat_g1(a2, vz);
                mi.pb = (g1v * mat_ggx_d(a2, mx, my, mz)) / (4.0f * vz);
                mi.gl = true;
                MatLight chosen;                              // as the DIFF block: the lane's light, or lt itself
                const MatLight &cur = LM == kLmTable ? chosen : lt;
                float P = 1.0f;
                if (LM == kLmTable) {
                    float u, unused;
                    mat_uniforms(key.pick, d, u, unused);
                    const uint32_t i = mat_light_pick(tb, u);
                    P = tb.cdf()[i] - (i ? tb.cdf()[i - 1u] : 0.0f);
                    mat_light_geometry<SC>(tb, (int)min(tb.idx()[i], tb.ns - 1u), chosen);
                    kprev = k;                                // sampled, whatever follows
                }
                if (k != cur.idx) {
                    const float wx0 = cur.cx - hx, wy0 = cur.cy - hy, wz0 = cur.cz - hz;
                    const float d2 = mat_dot(wx0, wy0, wz0, wx0, wy0, wz0);
                    if (d2 > cur.r2) {
                        float cx, cy, cz, omc;
                        mat_cone_sample(cur.r2, wx0, wy0, wz0, d2, key.nee, d, cx, cy, cz, omc);
                        if (LM == kLmNee) sampled = true;
                        const float wlx = mat_dot(cx, cy, cz, tx, ty, tz), wly = mat_dot(cx, cy, cz, bx, by, bz), wlz = mat_dot(cx, cy, cz, nlx, nly, nlz);
                        if (wlz > 0.0f) {
                            float hmx, hmy, hmz;
                            mat_normalise(vx + wlx, vy + wly, vz + wlz, hmx, hmy, hmz);
                            const float pb = (g1v * mat_ggx_d(a2, hmx, hmy, hmz)) / (4.0f * vz);
                            const float pl = P / (kMisTwoPi * omc);
                            const float sum = pb + pl;
                            sh.dx = cx; sh.dy = cy; sh.dz = cz;
                            sh.w = mat_g1(a2, wlz) * (pb / sum);
                            sh.g = cur.idx;
                            sh.want = sum > 0.0f && sum < __builtin_inff();   // false for NaN: a vanishing v.z
                        }
                    }
                }
            }
        } else {
            s.tx = s.tx * g; s.ty = s.ty * g; s.tz = s.tz * g;
        }
        const float qx = (tx * lx + bx * ly) + nlx * lz, qy = (ty * lx + by * ly) + nly * lz, qz = (tz * lx + bz * ly) + nlz * lz;
        mat_normalise(qx, qy, qz, ndx, ndy, ndz);
    } else {
        const float k2 = ddn * 2.0f;                          // SPEC, and the reflection of REFR
        ndx = s.dx - nx * k2; ndy = s.dy - ny * k2; ndz = s.dz - nz * k2;
        if (h.code == APT_MAT_REFR) {
            const float dn = into ? ddn : -ddn;
            const float nnt = into ? APT_MAT_NNT_IN : 1.5f;
            const float cos2t = 1.0f - (nnt * nnt) * (1.0f - dn * dn);
            if (!(cos2t < 0.0f)) {                            // otherwise total internal reflection: the reflection, weight 1
                float g = dn * nnt + sqrtf(cos2t);
                g = into ? g : -g;
                const float vx = s.dx * nnt - nx * g, vy = s.dy * nnt - ny * g, vz = s.dz * nnt - nz * g;
                float tdx, tdy, tdz;
                mat_normalise(vx, vy, vz, tdx, tdy, tdz);
                const float dt = mat_dot(tdx, tdy, tdz, nx, ny, nz);
                const float c = 1.0f - (into ? -ddn : dt);
                const float c5 = (((c * c) * c) * c) * c;
                const float re = APT_MAT_R0 + APT_MAT_1MR0 * c5;
                const float tr = 1.0f - re;
                const float P = 0.25f + 0.5f * re;
                float u1, u2;
                mat_uniforms(key.bounce, d, u1, u2);
                float wt;
                if (u1 < P) {
                    wt = re / P;
                } else {
                    wt = tr / (1.0f - P);
                    ndx = tdx; ndy = tdy; ndz = tdz;
                    outward = !into;
                }
                s.tx = s.tx * wt; s.ty = s.ty * wt; s.tz = s.tz * wt;
            }
        }
    }
    s.dx = ndx; s.dy = ndy; s.dz = ndz;
    s.ox = hx; s.oy = hy; s.oz = hz;
    s.skip = outward ? k : -1;
}

// ---- intersection with the skip rule ------------------------------------------------------------------------------------------
// The 8-sphere scene: sphere pairs from SGPRs through the packed discriminant of the mirror kernels (each half rounds like the
// scalar form), then render_do_ex's K-mode root selection with IEEE sqrtf() and the strict '<' arg-min.  SKIP: the path's skip
// sphere is not a candidate (false for camera rays, which have none).
template <bool SKIP>
__device__ __forceinline__ void mat_hit8(const Scene8 &sc, const MatPath &s, float eps, float &tmin, int &idx) {
    tmin = kMissT;
    idx = -1;
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const HitPre2 h = intersect_pre2(f2{sc.cx[k], sc.cx[k + 1]}, f2{sc.cy[k], sc.cy[k + 1]}, f2{sc.cz[k], sc.cz[k + 1]},
                                         f2{sc.r2[k], sc.r2[k + 1]}, s.ox, s.oy, s.oz, s.dx, s.dy, s.dz);
        const float t0 = intersect_post(HitPre{h.b.x, h.disc.x}, eps), t1 = intersect_post(HitPre{h.b.y, h.disc.y}, eps);
        if (t0 < tmin && (!SKIP || s.skip != k)) { tmin = t0; idx = k; }
        if (t1 < tmin && (!SKIP || s.skip != k + 1)) { tmin = t1; idx = k + 1; }
    }
}

// Any scene: tile_scan (pt_trace.h), as dyn_segment, with the strict '<' arg-min.  Every thread of the workgroup calls this together
// (barriers).  A lane skips nothing but its own skip sphere; the candidates come in ascending order, so ties keep the lowest index.
__device__ __forceinline__ void mat_hit_tiles(const float *__restrict__ sph, float4 *tile, const MatPath &s, uint32_t ns, float eps,
                                              float &tmin, int &idx) {
    tmin = kMissT;
    idx = -1;
    tile_scan(sph, tile, ns, eps, s.ox, s.oy, s.oz, s.dx, s.dy, s.dz, [&](float t, uint32_t sphere) __attribute__((always_inline)) {
        if (t < tmin && (int)sphere != s.skip) { tmin = t; idx = (int)sphere; }
    });
}

// Any scene behind the uniform grid (apt_render_params.accel with APT_FLAG_GRID_SLOTS): the always-tested list, then a per-lane 3D-DDA over
// the cells' item ranges (cells / items / item_geom: the nested walk's tables, pt_core.h GridHeader), with THIS renderer's root selection
// -- intersect_pre / intersect_post, IEEE sqrtf(), no root keys -- so every candidate's t is the tile form's, bit for bit.  The walk is
// grid_segment's own (grid_walk_cells, pt_trace.h: both call it with their candidate test) with its exactness argument and safety rules:
// a sphere's box was inflated by `margin` when it was binned, the walk ends only once tmin lies clearly before the exit of the current
// cell (or the ray leaves the grid), and lanes whose |d|^2 is not within 1e-3 of 1, or not finite, test every sphere from the grid's
// geom table.  It only drops spheres that cannot be hit, so the hit -- and the image -- is the tile form's.  Two things differ from the
// mirror kernels' candidates:
//   arg-min  candidates do not come in ascending sphere order: t < tmin || (t == tmin && k < idx), which equals the tile form's strict
//            '<' over ascending indices; idx starts at -1 (no hit: the path ends).
//   skip     the sphere whose INDEX is the path's skip sphere is no candidate, in the list and in the cells alike (never decided by
//            geometry: two spheres may share a record).  A cell candidate's index is one more dependent load, so it is fetched only when
//            its root could win or tie (t <= tmin); the always-tested list carries its indices with the geometry.
// No barriers: every lane walks on its own, lanes whose path has ended only take part in the wave-uniform list.  The header is the
// caller's (load_grid_header: scalar loads, once per kernel); the caller has checked that the grid is this scene's.
__device__ __forceinline__ void mat_hit_grid(const GridHeader &h, const uint32_t *__restrict__ grid, const MatPath &s, float eps,
                                             float &tmin, int &idx, uint32_t &n_cells, uint32_t &n_tests) {
    const uint32_t *large = grid + h.off_large, *cells = grid + h.off_cells, *items = grid + h.off_items;
    const float4 *geom = reinterpret_cast<const float4 *>(grid + h.off_geom);
    const float4 *item_geom = reinterpret_cast<const float4 *>(grid + h.off_item_geom);
    float best = kMissT;
    int bi = -1;
    // a sphere of known index: the always-tested list (walls: hit by every ray, so no `disc >= 0` skip) and the every-sphere fallback
    auto test = [&](const float4 g, uint32_t k) __attribute__((always_inline)) {
        ++n_tests;
        const float t = intersect_post(intersect_pre(g.x, g.y, g.z, g.w, s.ox, s.oy, s.oz, s.dx, s.dy, s.dz), eps);
        if ((int)k != s.skip && (t < best || (t == best && (int)k < bi))) { best = t; bi = (int)k; }
    };
    // a candidate of the walk, identified by its position in the item list
    auto test_item = [&](const float4 g, uint32_t i) __attribute__((always_inline)) {
        const HitPre hp = intersect_pre(g.x, g.y, g.z, g.w, s.ox, s.oy, s.oz, s.dx, s.dy, s.dz);
        if (hp.disc >= 0.0f) {                       // a negative or NaN discriminant gives kMissT, which never wins
            const float t = intersect_post(hp, eps);
            if (t <= best) {
                const int k = (int)items[i];
                if (k != s.skip && (t < best || k < bi)) { best = t; bi = k; }
            }
        }
    };
#if defined(__HIP_DEVICE_COMPILE__)
    if (h.off_cellslot) {
        // The list from its pair slots by explicit SCALAR loads, as grid_segment reads it (wave-uniform data the compiler would fetch
        // with vector loads and a wait each): two spheres and their indices per pair of loads; an odd list ends with a pad.
        typedef float f32x8 __attribute__((ext_vector_type(8)));
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const float *sg = reinterpret_cast<const float *>(grid + h.off_slots);
        const uint32_t *si = grid + h.off_slot_ids;
        for (uint32_t j = 0; j < h.slot_base; ++j) {
            f32x8 g8;
            u32x2 id2;
            asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(g8), "=&s"(id2) : "s"(sg + 8 * j), "s"(si + 2 * j) : "memory");
            test(make_float4(g8[0], g8[2], g8[4], g8[6]), id2[0]);
            if (id2[1] != kGridNoSphere) test(make_float4(g8[1], g8[3], g8[5], g8[7]), id2[1]);
        }
    } else
#endif
        for (uint32_t i = 0; i < h.nlarge; ++i) { const uint32_t k = large[i]; test(geom[k], k); }   // wave-uniform
    float dd = s.dx * s.dx;
    dd = dd + s.dy * s.dy;
    dd = dd + s.dz * s.dz;
    const bool unit = fabsf(dd - 1.0f) <= 1e-3f;     // false for NaN / inf
    if (s.live && !unit) {
        for (uint32_t k = 0; k < h.num_spheres; ++k) test(geom[k], k);   // every sphere (the list's again: same t, no change)
    } else if (s.live) {
        grid_walk_cells(h, cells, item_geom, s.ox, s.oy, s.oz, s.dx, s.dy, s.dz, n_cells, n_tests, test_item, [&]() { return best; });
    }
    tmin = best;
    idx = bi;
}

// What the 8-sphere form keeps per workgroup: geometry in SGPRs (Scene8), geometry / albedo / emission in LDS, and the 8 material codes
// in ONE SGPR word (4 bits each, saturated at 15: every code above 2 is bad).
struct MatScene8 {
    Scene8 sc;
    const float4 *tab;
    uint32_t codes;
};
// GL: the codes are mat_gloss_code's (3 = gloss, still 4 bits each), and alpha goes into the table's fourth block.
template <bool GL>
__device__ __forceinline__ MatScene8 load_mat_scene8(const float *__restrict__ sph, const uint32_t *__restrict__ mat, float4 *tab) {
    MatScene8 m;
    if (threadIdx.x < 8) {
        const int k = threadIdx.x;
        tab[16 + k] = make_float4(sph[32 + k], sph[40 + k], sph[48 + k], 0.0f);
        if (GL) {
            uint32_t q;
            const bool gloss = mat_gloss_code(mat[k], q) == (uint32_t)APT_MAT_GLOSS;
            tab[24 + k] = make_float4(gloss ? (float)q * 0x1p-16f : 0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    (void)load_scene8<false>(sph, m.sc, tab);   // geometry and albedo entries; its barrier covers the emission entries too
    m.tab = tab;
    uint32_t codes = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint32_t q;
        codes |= (GL ? mat_gloss_code(mat[k], q) : min(mat[k], 15u)) << (4 * k);
    }
    m.codes = codes;
    return m;
}

// One path, `depth` segments (fewer when every path of the wave -- of the workgroup for the tile form -- has ended).  -> segments traced.
// gh: the grid's header (kSceneGrid only; not read by the other forms).  lt: the light (kLmNee only).  tb: the light table (kLmTable).
// LM != kLmNone: after a bounce that drew a shadow segment, that segment goes through the form's own hit routine -- so it sees the scene the bounce
// ray will see -- whenever some lane of the wave (of the workgroup for the tile form, whose scan has barriers) has one; the light is
// visible iff the arg-min is the light (the lane's own chosen light with a table).  A traced shadow segment counts as a traced segment.
// EV (kMatEnv; env: the environment, else not read): a live path that finds no sphere gathers the sky and -- unless the bounce before
// sampled it -- the sun before it ends, and after a DIFF bounce that drew one (mat_shade) the sun's shadow segment goes through the
// same hit routine under the same vote, after the light's: the sun is visible iff it finds no sphere.
// MI (kMatMis): a GLOSS bounce may draw a shadow segment as well (mat_shade), which goes the same way; its G1(l) multiplies T after it.
template <int SC, int LM, bool GL, bool EV = false, bool MI = false, class ENV = MatNoEnv>
__device__ __forceinline__ uint32_t trace_mat(const float *__restrict__ sph, const uint32_t *__restrict__ mat, const MatScene8 &m8,
                                              const GridHeader &gh, const MatLight &lt, const MatTable &tb, float4 *tile, MatPath &s,
                                              const TraceArgs &ta, uint64_t path, const ENV &env = ENV()) {
    const MatKeys key = mat_path_keys<LM>(ta.seed, path);
    MatSun su;
    su.sampled = false;
    if constexpr (EV) su.key = env.sample ? sun_path_key(ta.seed, path) : 0;
    const uint64_t rr_key = ta.rr_start ? rr_path_key(ta.seed, path) : 0;
    uint32_t traced = 0, n_cells = 0, n_tests = 0;           // the last two: walk statistics of the grid form
    bool sampled = false;                                    // kLmNee: the previous bounce sampled the light
    int kprev = -1;                                          // kLmTable: the sphere of the previous bounce if it was a sampling bounce, else -1
    MatMis mi = {0.0f, false, 1.0f};
    for (uint32_t d = 0; d < ta.depth; ++d) {
        MatHit h;
        h.alpha = 0.0f;
        if (SC == kScene8) {
            if (__all(!s.live)) break;
            if (d == 0) mat_hit8<false>(m8.sc, s, ta.eps, h.t, h.k);
            else mat_hit8<true>(m8.sc, s, ta.eps, h.t, h.k);
            const int g = h.k < 0 ? 0 : h.k;
            h.geo = m8.tab[g]; h.alb = mat_rgb(m8.tab[8 + g]); h.em = mat_rgb(m8.tab[16 + g]);
            h.code = (m8.codes >> (4 * g)) & 15u;
            if (GL) h.alpha = m8.tab[24 + g].x;
        } else {
            if (SC == kSceneGrid) {
                if (__all(!s.live)) break;
                mat_hit_grid(gh, ta.grid, s, ta.eps, h.t, h.k, n_cells, n_tests);
            } else {
                if (__syncthreads_and(!s.live)) break;
                mat_hit_tiles(sph, tile, s, ta.ns, ta.eps, h.t, h.k);
            }
            const size_t ns = ta.ns, g = h.k < 0 ? 0 : (size_t)h.k;
            h.geo = make_float4(sph[ns + g], sph[2 * ns + g], sph[3 * ns + g], 0.0f);
            h.alb = MatRgb{sph[7 * ns + g], sph[8 * ns + g], sph[9 * ns + g]};
            h.em = MatRgb{sph[4 * ns + g], sph[5 * ns + g], sph[6 * ns + g]};
            h.code = mat[g];
            if (GL) {
                uint32_t q;
                h.code = mat_gloss_code(h.code, q);
                h.alpha = (float)q * 0x1p-16f;
            }
        }
        if constexpr (EV) {
            if (GL && !env.gloss && h.code == (uint32_t)APT_MAT_GLOSS) h.code = 15u;   // no APT_FLAG_GLOSS: a gloss word is a bad code
            if (s.live && h.k < 0) {                          // miss: the sky, and the sun unless the bounce before sampled it
                float t = s.dy * 0.5f + 0.5f;
                t = t > 0.0f ? t : 0.0f;
                t = t < 1.0f ? t : 1.0f;
                const float kx = env.horizon[0] + (env.zenith[0] - env.horizon[0]) * t;
                const float ky = env.horizon[1] + (env.zenith[1] - env.horizon[1]) * t;
                const float kz = env.horizon[2] + (env.zenith[2] - env.horizon[2]) * t;
                s.lx = s.lx + s.tx * kx; s.ly = s.ly + s.ty * ky; s.lz = s.lz + s.tz * kz;
                if (env.omc > 0.0f && mat_dot(s.dx, s.dy, s.dz, env.sun[0], env.sun[1], env.sun[2]) >= 1.0f - env.omc && !su.sampled) {
                    s.lx = s.lx + s.tx * env.sun_rad[0]; s.ly = s.ly + s.ty * env.sun_rad[1]; s.lz = s.lz + s.tz * env.sun_rad[2];
                }
            }
        }
        const bool hit = s.live && h.k >= 0;
        const bool bad = hit && h.code > (uint32_t)(GL ? APT_MAT_GLOSS : APT_MAT_REFR);
        if (__any(bad)) report_status(ta, APT_DEV_BAD_MATERIAL);
        s.live = hit && !bad;
        const bool may = LM && d + 1 < ta.depth;              // no sample at the last bounce: the header says why
        MatShadow sh;
        sh.want = false;
        su.sh.want = false;
        su.may = false;
        if constexpr (EV) su.may = env.sample && d + 1 < ta.depth;   // no sample at the last bounce, as for the lights
        if (s.live) {
            mat_shade<LM, SC, GL, EV, MI>(s, h, key, d, lt, may, sampled, sh, tb, kprev, env, su, mi);
            ++traced;
        }
        if (may && (SC == kSceneTiles ? __syncthreads_or(sh.want) : __any(sh.want))) {
            MatPath q;                                        // from h (s.o) along l with this bounce's skip (a DIFF bounce's own)
            q.ox = s.ox; q.oy = s.oy; q.oz = s.oz;
            q.dx = sh.want ? sh.dx : s.dx; q.dy = sh.want ? sh.dy : s.dy; q.dz = sh.want ? sh.dz : s.dz;
            q.skip = s.skip;
            q.live = sh.want;
            float ts;
            int ks;
            if (SC == kScene8) mat_hit8<true>(m8.sc, q, ta.eps, ts, ks);
            else if (SC == kSceneGrid) mat_hit_grid(gh, ta.grid, q, ta.eps, ts, ks, n_cells, n_tests);
            else mat_hit_tiles(sph, tile, q, ta.ns, ta.eps, ts, ks);
            if (sh.want) {
                ++traced;
                if (LM == kLmTable) {
                    if (ks == sh.g) {
                        const float4 e = mat_light_emission<SC>(tb, sh.g);
                        s.lx = s.lx + (s.tx * e.x) * sh.w; s.ly = s.ly + (s.ty * e.y) * sh.w; s.lz = s.lz + (s.tz * e.z) * sh.w;
                    }
                } else if (ks == lt.idx) {
                    s.lx = s.lx + (s.tx * lt.ex) * sh.w; s.ly = s.ly + (s.ty * lt.ey) * sh.w; s.lz = s.lz + (s.tz * lt.ez) * sh.w;
                }
            }
        }
        if constexpr (MI) {
            s.tx = s.tx * mi.g; s.ty = s.ty * mi.g; s.tz = s.tz * mi.g;   // G1(l) of a GLOSS bounce, else 1: the light's segment used T before it
            mi.g = 1.0f;
        }
        if constexpr (EV) {
            if (su.may && (SC == kSceneTiles ? __syncthreads_or(su.sh.want) : __any(su.sh.want))) {
                const bool want = su.sh.want;
                MatPath q;                                    // from h along l with this bounce's skip, as the light's segment
                q.ox = s.ox; q.oy = s.oy; q.oz = s.oz;
                q.dx = want ? su.sh.dx : s.dx; q.dy = want ? su.sh.dy : s.dy; q.dz = want ? su.sh.dz : s.dz;
                q.skip = s.skip;
                q.live = want;
                float ts;
                int ks;
                if (SC == kScene8) mat_hit8<true>(m8.sc, q, ta.eps, ts, ks);
                else if (SC == kSceneGrid) mat_hit_grid(gh, ta.grid, q, ta.eps, ts, ks, n_cells, n_tests);
                else mat_hit_tiles(sph, tile, q, ta.ns, ta.eps, ts, ks);
                if (want) {
                    ++traced;
                    if (ks < 0) {                             // nothing in the way: the sun is visible
                        s.lx = s.lx + (s.tx * env.sun_rad[0]) * su.sh.w; s.ly = s.ly + (s.ty * env.sun_rad[1]) * su.sh.w;
                        s.lz = s.lz + (s.tz * env.sun_rad[2]) * su.sh.w;
                    }
                }
            }
        }
        if (ta.rr_start && d + 1 >= ta.rr_start) {          // wave-uniform; APT_FLAG_RR on T
            PathState t;
            t.rxy = f2{s.tx, s.ty}; t.rz = s.tz; t.alive = s.live ? 1u : 0u;
            russian_roulette(t, rr_key, d);
            s.tx = t.rxy.x; s.ty = t.rxy.y; s.tz = t.rz;
        }
    }
    if (SC == kSceneGrid) grid_stats(ta, n_cells, n_tests);
    return traced;
}

// The grid form's header, once per kernel.  A grid that does not keep the caller's promise (APT_FLAG_GRID_SLOTS: built for this scene)
// is not walked: -> false, the kernel writes nothing and says APT_DEV_GRID_MISMATCH (the mirror kernels' rule, pt_queue.h).  Uniform
// over the whole launch, so every thread of a workgroup returns together.
template <int SC>
__device__ __forceinline__ bool mat_grid_header(const TraceArgs &ta, GridHeader &gh) {
    if (SC != kSceneGrid) return true;
    gh = load_grid_header(ta.grid);
    if (gh.magic == kGridMagic && gh.num_spheres == ta.ns) return true;
    report_status(ta, APT_DEV_GRID_MISMATCH);
    return false;
}

__device__ __forceinline__ void mat_path_init(MatPath &s, float ox, float oy, float oz, float dx, float dy, float dz) {
    s.ox = ox; s.oy = oy; s.oz = oz; s.dx = dx; s.dy = dy; s.dz = dz;
    s.tx = s.ty = s.tz = 1.0f;
    s.lx = s.ly = s.lz = 0.0f;
    s.skip = -1;
    s.live = true;
}

// ---- kernel: rays from a buffer -----------------------------------------------------------------------------------------------
// SCN: the scene form, with kMatNee set for APT_FLAG_NEE or kMatLights for a light table, and kMatGloss.  All travel in the first template argument so
// that the instantiations a launch without them runs keep the symbol names (and, the sampling code being dead there, the instructions)
// they had before these existed.
// ev: the environment with kMatEnv, else an empty argument (which moves the hidden kernel arguments by 8 bytes: the only thing that
// differs in the instructions of the kernels without kMatEnv from what they were before there was an environment).
template <int SCN>
__global__ __launch_bounds__(kBlock) void render_paths_mat_kernel(const float *__restrict__ rays, const float *__restrict__ sph,
                                                                  const uint32_t *__restrict__ mat, float *__restrict__ colors,
                                                                  uint64_t n_total, uint64_t begin, uint64_t count, MatKernelArgs ka,
                                                                  MatEnvArg<SCN> ev) {
    const TraceArgs &ta = ka.ta;
    constexpr int SC = mat_scene_of(SCN);
    constexpr int LM = mat_light_mode(SCN);
    constexpr bool GL = (SCN & kMatGloss) != 0;
    constexpr bool EV = (SCN & kMatEnv) != 0;
    constexpr bool MI = (SCN & kMatMis) != 0;
    static_assert(!MI || (EV && GL && LM != kLmNone), "the kMatMis kernels are gloss, environment kernels with a light mode");
    __shared__ float4 tab[mat_tab_entries(SCN)];
    __shared__ float4 tile[SC == kSceneTiles ? kTile : 1];
    GridHeader gh;
    if (!mat_grid_header<SC>(ta, gh)) return;
    MatTable tb;
    if (!mat_lights_header<LM>(ka, sph, tab, tb)) return;
    MatScene8 m8;
    if (SC == kScene8) m8 = load_mat_scene8<GL>(sph, mat, tab);
    const MatLight lt = load_mat_light<LM>(sph, ta);      // here, not after the ray loads: there it reorders the registers of the flag-off kernels
    const uint64_t local = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = local < count;
    const uint64_t p = begin + (valid ? local : 0);
    MatPath s;
    mat_path_init(s, rays[p], rays[n_total + p], rays[2 * n_total + p], rays[3 * n_total + p], rays[4 * n_total + p], rays[5 * n_total + p]);
    const uint32_t traced = trace_mat<SC, LM, GL, EV, MI>(sph, mat, m8, gh, lt, tb, tile, s, ta, p, ev);
    if (valid) {
        colors[p] = s.lx;
        colors[n_total + p] = s.ly;
        colors[2 * n_total + p] = s.lz;
    }
    count_traced(ta, valid ? traced : 0);
}

// ---- kernel: rays of a camera into a buffer -----------------------------------------------------------------------------------------
// gen_rays_kernel (pt_kernels.h) for a CameraEx: the rays the camera instantiations of the frame kernel trace, bit for bit (the same
// camera_ray_ex on the same uniforms and lens point).
__global__ __launch_bounds__(kBlock) void gen_rays_camera_kernel(CameraEx cam, uint32_t width, uint32_t height, uint32_t samples,
                                                                 uint64_t seed, uint64_t n_total, uint64_t begin, uint64_t count,
                                                                 float *__restrict__ rays) {
    const uint64_t local = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = local < count;                                    // no early return: camera_ray_ex votes over the wave
    const uint64_t p = begin + (valid ? local : 0);
    uint32_t i, j, sy, sx;
    path_coords(p, height, samples, i, j, sy, sx);
    double u1, u2;
    path_uniforms(seed, p, u1, u2);
    float lx = 0.0f, ly = 0.0f;
    if (cam.t.lens) cam_lens_point(seed, p, cam.t.aperture, lx, ly);
    float rox, roy, roz, rdx, rdy, rdz;
    camera_ray_ex(cam, width, height, i, j, sy, sx, u1, u2, lx, ly, rox, roy, roz, rdx, rdy, rdz);
    if (valid) {
        rays[p] = rox; rays[n_total + p] = roy; rays[2 * n_total + p] = roz;
        rays[3 * n_total + p] = rdx; rays[4 * n_total + p] = rdy; rays[5 * n_total + p] = rdz;
    }
}

// The lane mapping of the fused frame kernel: pt_frame.h's, by range or (LIST) by list; a list's entries beyond the image are reported
// once per wave, before the bounce: nothing of it lives across the trace.
template <int GROUP, bool LIST>
__device__ __forceinline__ FrameLane<GROUP> mat_frame_lane(const FrameArgs &fa, const TraceArgs &ta) {
    if constexpr (LIST) {
        bool beyond;
        const FrameLane<GROUP> f = frame_lane_list<GROUP>(fa, beyond);
        if (__any(beyond)) report_status(ta, APT_DEV_LIST_RANGE);
        return f;
    } else {
        return frame_lane<GROUP>(fa);
    }
}

// ---- kernel: fused frame ------------------------------------------------------------------------------------------------------
// render_frame_kernel (pt_kernels.h) without its retirement queue and two-path form: pt_frame.h's lanes per sub-pixel (GROUP),
// camera and decode, the same pairwise leaves and tail; the sample is a material path and its colour is L.
// SCN: the scene form and kMatNee / kMatLights / kMatGloss, as for the buffer kernel, and kMatCamera: only then is `ct` read.
// kMatEnv (both kernels): only then does `ev` hold anything -- the environment.
// kMatFilm (with kMatEnv): fa.fb is a film and the tail is frame_film, not frame_decode; fa.fb_u8 is not read.
// kMatList (with kMatFilm): fa.fb_u8 is the address of a uint32 list of fa.pixel_count image pixels and lane pl traces list[pl]
// (pt_frame.h frame_lane_list); the film, compact, is still indexed by pl.  An entry beyond the image: APT_DEV_LIST_RANGE.
template <int SCN, int GROUP>
__global__ __launch_bounds__(kBlock) void render_frame_mat_kernel(const float *__restrict__ sph, const uint32_t *__restrict__ mat,
                                                                  FrameArgs fa, MatKernelArgs ka, LeafProg lp, CameraTail ct,
                                                                  MatEnvArg<SCN> ev) {
    const TraceArgs &ta = ka.ta;
    constexpr int SC = mat_scene_of(SCN);
    constexpr int LM = mat_light_mode(SCN);
    constexpr bool GL = (SCN & kMatGloss) != 0;
    constexpr bool EV = (SCN & kMatEnv) != 0;
    constexpr bool FILM = (SCN & kMatFilm) != 0;
    constexpr bool MI = (SCN & kMatMis) != 0;
    static_assert(!MI || (EV && GL && LM != kLmNone), "the kMatMis kernels are gloss, environment kernels with a light mode");
    static_assert(!FILM || EV, "the film kernels are environment kernels: store-or-add travels in MatEnv::gloss");
    constexpr bool LIST = (SCN & kMatList) != 0;
    static_assert(!LIST || FILM, "the list kernels are film kernels: a film launch never reads fa.fb_u8, which carries the list");
    bool film_add = false;
    if constexpr (FILM) {   // (launch-uniform) the word's bit 0 is what every other reader of ev.gloss takes it for
        film_add = (ev.gloss & kMatEnvFilmAdd) != 0;
        ev.gloss = ev.gloss & 1u;
    }
    __shared__ float4 tab[mat_tab_entries(SCN)];
    __shared__ float4 tile[SC == kSceneTiles ? kTile : 1];
    extern __shared__ float dyn_lds[];
    float *stack_lds = dyn_lds;                                            // [kMaxStack][3][kStackSlots] when lp.nleaves > 1
    constexpr bool CAM = (SCN & kMatCamera) != 0;                            // a context's camera: CameraEx (its tail from ct), camera_ray_ex
    __shared__ std::conditional_t<CAM, CameraEx, Camera> cam;
    GridHeader gh;
    if (!mat_grid_header<SC>(ta, gh)) return;
    MatTable tb;
    if (!mat_lights_header<LM>(ka, sph, tab, tb)) return;
    if constexpr (CAM) park_camera_ex(cam, fa, ct);
    else park_camera(cam, fa);
    MatScene8 m8;
    if (SC == kScene8) m8 = load_mat_scene8<GL>(sph, mat, tab);
    else __syncthreads();
    const MatLight lt = load_mat_light<LM>(sph, ta);

    const uint32_t lane = threadIdx.x & 63;
    const FrameLane<GROUP> fl = mat_frame_lane<GROUP, LIST>(fa, ta);
    const uint32_t j = fl.j, sub = fl.sub;
    const uint64_t pl = fl.pl;
    const bool valid = fl.valid;
    const uint32_t pi = fl.pi, pj = fl.pj, sy = fl.sy, sx = fl.sx;
    const uint64_t pbase = fl.pbase;
    uint32_t traced = 0;

    struct Col { float r, g, b; };
    auto sample = [&](uint32_t k) __attribute__((always_inline)) -> Col {
        double u1, u2;
        path_uniforms(fa.seed, pbase + k, u1, u2);
        float rox, roy, roz, rdx, rdy, rdz;
        if constexpr (CAM) {
            float lx = 0.0f, ly = 0.0f;
            if (cam.t.lens) cam_lens_point(fa.seed, pbase + k, cam.t.aperture, lx, ly);   // launch-uniform branch
            camera_ray_ex(cam, fa.width, fa.height, pi, pj, sy, sx, u1, u2, lx, ly, rox, roy, roz, rdx, rdy, rdz);
        } else {
            camera_ray(cam, fa.width, fa.height, pi, pj, sy, sx, u1, u2, rox, roy, roz, rdx, rdy, rdz);
        }
        MatPath s;
        mat_path_init(s, rox, roy, roz, rdx, rdy, rdz);
        traced += trace_mat<SC, LM, GL, EV, MI>(sph, mat, m8, gh, lt, tb, tile, s, ta, pbase + k, ev);
        return Col{s.lx, s.ly, s.lz};
    };
    auto add = [](const Col &a, const Col &b) { return Col{a.r + b.r, a.g + b.g, a.b + b.b}; };

    float res[3] = {0.0f, 0.0f, 0.0f};
    uint32_t start = 0;
    int sp = 0;
    for (uint32_t leaf = 0; leaf < lp.nleaves; ++leaf) {
        const uint32_t n = lp.len(leaf);
        float acc[3];
        if (GROUP == 1) { // n < 8: res = 0; res += a[i]
            Col a = {0.0f, 0.0f, 0.0f};
            for (uint32_t k = 0; k < n; ++k) a = add(a, sample(start + k));
            acc[0] = a.r; acc[1] = a.g; acc[2] = a.b;
        } else {          // 8 <= n <= 128: r[j] chains, tree, tail
            const uint32_t nfull = n & ~7u;
            Col a = sample(start + j);
            for (uint32_t i8 = 8; i8 < nfull; i8 += 8) a = add(a, sample(start + i8 + j));
            acc[0] = a.r; acc[1] = a.g; acc[2] = a.b;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { // ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7))
                float v = acc[ch];
                v = v + __shfl_xor(v, 1, 64);
                v = v + __shfl_xor(v, 2, 64);
                v = v + __shfl_xor(v, 4, 64);
                acc[ch] = v;
            }
            const uint32_t nt = n - nfull;
            if (nt) { // res += a[i] for the n % 8 trailing samples, in order
                const uint32_t traced_before = traced;
                const Col c = sample(start + nfull + (j < nt ? j : 0));
                if (j >= nt) traced = traced_before;
                for (uint32_t t = 0; t < nt; ++t) {
                    const int src = (int)((lane & ~7u) + t);
                    acc[0] = acc[0] + __shfl(c.r, src, 64);
                    acc[1] = acc[1] + __shfl(c.g, src, 64);
                    acc[2] = acc[2] + __shfl(c.b, src, 64);
                }
            }
        }
        start += n;
        if (lp.nleaves == 1) {
            res[0] = acc[0]; res[1] = acc[1]; res[2] = acc[2];
        } else { // pairwise(left) + pairwise(right), innermost first
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) stack_lds[(sp * 3 + ch) * kStackSlots + (threadIdx.x >> 3)] = acc[ch];
            ++sp;
            for (uint32_t mm = 0; mm < lp.ncomb(leaf); ++mm) {
                --sp;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float a = stack_lds[((sp - 1) * 3 + ch) * kStackSlots + (threadIdx.x >> 3)];
                    const float b = stack_lds[(sp * 3 + ch) * kStackSlots + (threadIdx.x >> 3)];
                    stack_lds[((sp - 1) * 3 + ch) * kStackSlots + (threadIdx.x >> 3)] = a + b;
                }
            }
        }
    }
    if (lp.nleaves > 1) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) res[ch] = stack_lds[ch * kStackSlots + (threadIdx.x >> 3)];
    }

    if constexpr (LIST) {   // the lane's slot and whether it writes, from the list again: one load here instead of values kept across the trace
        bool beyond;
        const FrameLane<GROUP> tl = frame_lane_list<GROUP>(fa, beyond);
        frame_film<GROUP>(fa, tl.pl, tl.valid, res, film_add);
        count_traced(ta, tl.valid ? traced : 0);
        return;
    } else if constexpr (FILM) {
        frame_film<GROUP>(fa, pl, valid, res, film_add);
    } else {
        __shared__ uint32_t u8pack[frame_u8_words(GROUP)];
        frame_decode<GROUP>(fa, pl, valid, res, u8pack);
    }
    count_traced(ta, valid ? traced : 0);
}

} // namespace
