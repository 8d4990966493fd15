// film.hip -- the film (include/render_mi355x.h "film"): the material frame kernels with a film tail (pt_materials.h kMatFilm,
// pt_frame.h frame_film) and the resolve kernel, with their launches: a fourth material code object (`make asm` writes it to film.s), so
// that render_kernels.hip, materials.hip and environment.hip are built from the instantiations they always held.  As in environment.hip
// the frame kernels are the general-camera, gloss, environment instantiations only: 3 scene forms x 3 light modes x 2 groups.  A launch
// without a camera gets the default record, one without an environment the all-zero record (render_kernels.hip), which
// tests/test_gpu_environment.py shows to be the image without one bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_materials.h"
#include "pt_core.h"
#include "pt_dispatch.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

// environment.hip's record, with "store or add" in bit 1 of the gloss word (kMatEnvFilmAdd): no kernel argument of its own
MatEnv film_env(const apt_environment &e, bool gloss, bool add) {
    MatEnv m;
    for (int k = 0; k < 3; ++k) { m.horizon[k] = e.horizon[k]; m.zenith[k] = e.zenith[k]; m.sun[k] = e.sun_dir[k]; m.sun_rad[k] = e.sun_radiance[k]; }
    m.omc = e.sun_omc;
    m.sample = ((e.flags & APT_ENV_SAMPLE_SUN) && e.sun_omc > 0.0f) ? 1u : 0u;
    m.gloss = (gloss ? 1u : 0u) | (add ? kMatEnvFilmAdd : 0u);
    return m;
}

constexpr int film_scene_form(bool ns8, bool grid, bool nee, bool lights) {
    return mat_scene_form(ns8, grid, nee, lights, true, true) | kMatEnv | kMatFilm;
}

// ---- resolve ----------------------------------------------------------------------------------------------------------------
// One lane = one pixel: three coalesced plane reads, the header's operations one at a time, an 8-step search in the table (LDS), and
// three coalesced plane stores.  The workgroup's 8-bit pixels -- kBlock * 3 consecutive bytes that start wherever u8 + 3 * first pixel
// falls -- are gathered in LDS and leave as whole dwords; the bytes of a dword that the workgroup's range does not cover (its ragged
// head and tail, and all of a short last workgroup's) leave as byte stores.
struct ResolveArgs {
    const float *film, *table;
    float *out;
    uint8_t *u8;
    uint64_t pixel_count;
    float fpasses, exposure, inv_white2;
    uint32_t reinhard;
};

__device__ __forceinline__ float film_tone(float s, const ResolveArgs &a) {
    const float m = s / a.fpasses;
    float x = m * a.exposure;
    x = x > 0.0f ? x : 0.0f;
    float y = x;
    if (a.reinhard) {   // (launch-uniform)
        float t = x * a.inv_white2;
        t = 1.0f + t;
        const float num = x * t;
        const float den = 1.0f + x;
        y = x == __builtin_inff() ? 1.0f : num / den;
    }
    return y < 1.0f ? y : 1.0f;
}

__global__ __launch_bounds__(kBlock) void film_resolve_kernel(ResolveArgs a) {
    __shared__ float table[256];
    __shared__ uint8_t bytes[kBlock * 3];
    static_assert(kBlock == 256, "one table entry per thread");
    table[threadIdx.x] = a.table[threadIdx.x];
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * kBlock;                  // < pixel_count: the grid is ceil(pixel_count / kBlock)
    const uint64_t i = first + threadIdx.x;
    if (i < a.pixel_count) {
#pragma unroll
        for (uint64_t c = 0; c < 3; ++c) {
            const float y = film_tone(a.film[c * a.pixel_count + i], a);
            if (a.out) a.out[c * a.pixel_count + i] = y;
            uint32_t code = 0;
#pragma unroll
            for (uint32_t b = 128; b; b >>= 1) code += table[code + b] <= y ? b : 0u;
            bytes[threadIdx.x * 3 + c] = (uint8_t)code;
        }
    }
    if (!a.u8) return;                                                     // (launch-uniform)
    __syncthreads();
    const uint64_t left = a.pixel_count - first;
    const uint32_t nbytes = (uint32_t)(left < (uint64_t)kBlock ? left : (uint64_t)kBlock) * 3u;
    uint8_t *const dst = a.u8 + first * 3;                                 // bytes[k] -> dst[k], 0 <= k < nbytes
    const uint32_t head = (uint32_t)((uintptr_t)dst & 3u);                 // dword k of the range starts at byte 4k - head
    const int32_t k0 = (int32_t)threadIdx.x * 4 - (int32_t)head;
    if (k0 >= (int32_t)nbytes) return;                                     // (at most kBlock * 3 / 4 + 1 dwords: fewer than kBlock)
    if (k0 >= 0 && k0 + 4 <= (int32_t)nbytes) {
        const uint32_t w = (uint32_t)bytes[k0] | ((uint32_t)bytes[k0 + 1] << 8) | ((uint32_t)bytes[k0 + 2] << 16) | ((uint32_t)bytes[k0 + 3] << 24);
        *reinterpret_cast<uint32_t *>(dst + k0) = w;
    } else {
        for (int32_t k = k0 < 0 ? 0 : k0; k < k0 + 4 && k < (int32_t)nbytes; ++k) dst[k] = bytes[k];
    }
}

} // namespace

namespace apt {

void film_render_frame(const MatFrameCall &c, const apt_environment &env, bool add) {
    FrameArgs fa;
    const CameraEx cx = camera_ex(*c.camera, c.width, c.height);
    fa.cam = cx.base;
    fa.width = c.width; fa.height = c.height; fa.samples = c.samples; fa.seed = c.t.seed;
    fa.pixel_begin = c.pixel_begin; fa.pixel_count = c.pixel_count; fa.fb = c.fb; fa.fb_u8 = nullptr;
    const MatKernelArgs ka = mat_trace_args(c.t);
    const MatEnv ev = film_env(env, c.t.gloss, add);
    LeafProg lp;
    (void)make_leaf_plan(c.samples, lp);                   // the caller checked mat_camera_fits
    const int group = c.samples >= 8 ? 8 : 1;
    const uint64_t blocks = (c.pixel_count * 4u * (uint64_t)group + kBlock - 1) / kBlock;   // <= 2^31 - 1: checked by the caller
    const size_t lds = lp.nleaves > 1 ? (size_t)kMaxStack * 3 * kStackSlots * sizeof(float) : 0;
    hipStream_t st = (hipStream_t)c.stream;
    with_flag(c.t.ns == 8, [&](auto ns8) { with_flag(c.t.grid != nullptr, [&](auto gr) { with_flag(group == 8, [&](auto g8) {
        with_flag(c.t.nee, [&](auto nee) { with_flag(c.t.lights != nullptr, [&](auto lt) {
            hipLaunchKernelGGL((render_frame_mat_kernel<film_scene_form(ns8, gr, nee, lt), g8 ? 8 : 1>), dim3((unsigned)blocks),
                               dim3(kBlock), lds, st, c.spheres, c.materials, fa, ka, lp, cx.t, ev);
        }); });
    }); }); });
}

void film_resolve(const apt_film_resolve &r, void *stream, const float *film, uint64_t pixel_count, const float *table_dev, float *out,
                  uint8_t *u8) {
    ResolveArgs a;
    a.film = film; a.table = table_dev; a.out = out; a.u8 = u8; a.pixel_count = pixel_count;
    a.fpasses = (float)r.passes; a.exposure = r.exposure; a.inv_white2 = r.inv_white2;
    a.reinhard = r.tonemap == (uint32_t)APT_TONEMAP_REINHARD ? 1u : 0u;
    const uint64_t blocks = (pixel_count + kBlock - 1) / kBlock;           // <= 2^31 - 1: checked by the caller
    hipLaunchKernelGGL(film_resolve_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
}

} // namespace apt
