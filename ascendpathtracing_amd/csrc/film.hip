// film.hip -- the film (include/render_mi355x.h "film"): the material frame kernels with a film tail (pt_materials.h kMatFilm,
// pt_frame.h frame_film) and the resolve kernel, with their launches: a fourth material code object (`make asm` writes it to film.s), so
// that render_kernels.hip, materials.hip and environment.hip are built from the instantiations they always held.  As in environment.hip
// the frame kernels are the general-camera, gloss, environment instantiations only: 3 scene forms x 3 light modes x 2 groups.  A launch
// without a camera gets the default record, one without an environment the all-zero record (materials.hip mat_render_frame).  The
// launch itself: pt_mat_launch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_materials.h"
#include "film_ops.h"
#include "pt_core.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

constexpr int kPins = kMatEnv | kMatGloss | kMatCamera | kMatFilm;

// ---- resolve ----------------------------------------------------------------------------------------------------------------
// One lane = one pixel: three coalesced plane reads, the header's operations one at a time and an 8-step search in the table (LDS) --
// film_ops.h's film_tone and film_code, as in the CPU twin --, and three coalesced plane stores.  The workgroup's 8-bit pixels --
// kBlock * 3 consecutive bytes that start wherever u8 + 3 * first pixel falls -- are gathered in LDS and leave as whole dwords; the
// bytes of a dword that the workgroup's range does not cover (its ragged head and tail, and all of a short last workgroup's) leave as
// byte stores.
struct ResolveArgs {
    const float *film, *table;
    float *out;
    uint8_t *u8;
    uint64_t pixel_count;
    apt::FilmTone tone;
};

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
            const float y = apt::film_tone(a.film[c * a.pixel_count + i], a.tone);
            if (a.out) a.out[c * a.pixel_count + i] = y;
            bytes[threadIdx.x * 3 + c] = (uint8_t)apt::film_code(table, y);
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

void film_launch_frame(const MatFrameCall &c) { launch_mat_frame<kPins>(c); }

void film_resolve(const apt_film_resolve &r, void *stream, const float *film, uint64_t pixel_count, const float *table_dev, float *out,
                  uint8_t *u8) {
    ResolveArgs a;
    a.film = film; a.table = table_dev; a.out = out; a.u8 = u8; a.pixel_count = pixel_count;
    a.tone = FilmTone{(float)r.passes, r.exposure, r.inv_white2, r.tonemap == (uint32_t)APT_TONEMAP_REINHARD ? 1u : 0u};
    const uint64_t blocks = (pixel_count + kBlock - 1) / kBlock;           // <= 2^31 - 1: checked by the caller
    hipLaunchKernelGGL(film_resolve_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
}

} // namespace apt
