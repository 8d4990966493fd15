// upscale.hip -- the device side of libupscale_mi355x.so (include/render_mi355x_upscale.h): the prepare, upsample and patch kernels
// with their launches and the device entries of the C-ABI.  A library of its own (`make asm` writes its code object to upscale.s).
// The arithmetic of every step is upscale_ops.h, which upscale_host.cpp's CPU twins call too; the entries' checks are
// upscale_host.cpp's.
//
// The upsample: one lane = one full-size pixel, and the image is x-major, so consecutive lanes take consecutive y of one column (a
// workgroup's 256 lanes run on into the next column): the 8 plane reads, the 3 plane stores and the `resolved` store are coalesced.
// Each of up to four taps is three 16-byte record loads; neighbouring lanes share taps (two full pixels a low pixel along y at a
// ratio of 2), so a wave's gathers fall into a few cache lines of two low columns.  The two float64 coordinate chains are computed
// per lane: a wave may straddle columns, so a column's x0 / fx would need a uniformity test or a table pass for one multiply, one
// divide, a subtract and a floor a lane (DESIGN.md "Upscale").  No LDS, no atomics, no state; the upsample launch follows the
// prepare launch on the same stream, nothing waits for another workgroup.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x_upscale.h"
#include "film_stage_launch.h"
#include "upscale_host.h"
#include "upscale_ops.h"

using apt::blocks_for;
using apt::kUpBlock;
using apt::launched;
using apt::UpArgs;

namespace {

__global__ __launch_bounds__(kUpBlock) void film_upscale_prepare_kernel(UpArgs a) {
    const uint32_t i = blockIdx.x * kUpBlock + threadIdx.x;              // < 2^28 + 256
    const uint32_t nl = a.lw * a.lh;                                     // <= w * h <= 2^28: the entry's check
    if (i >= nl) return;
    apt::up_prepare(a, nl, i);
}

__global__ __launch_bounds__(kUpBlock) void film_upscale_kernel(UpArgs a) {
    const uint32_t i = blockIdx.x * kUpBlock + threadIdx.x;              // < 2^28 + 256
    if (i >= a.w * a.h) return;
    const uint32_t x = i / a.h;
    apt::up_pixel(a, x, i - x * a.h);
}

__global__ __launch_bounds__(kUpBlock) void film_upscale_patch_kernel(const float *sums, const uint32_t *list, uint64_t count, float K,
                                                                      uint64_t n, float *out) {
    const uint64_t i = (uint64_t)blockIdx.x * kUpBlock + threadIdx.x;
    if (i >= count) return;
    apt::up_patch(sums, list, count, K, n, out, i);
}

} // namespace

extern "C" {

int apt_film_upscale_device(const apt_film_upscale *rec, void *stream, const float *lo, const float *lo_features, uint32_t lo_width,
                            uint32_t lo_height, const float *hi_features, uint32_t width, uint32_t height, float *work, float *out,
                            uint32_t *resolved) {
    apt::stage_clear_error();
    UpArgs a;
    const int rc = apt::film_upscale_check(rec, lo, lo_features, lo_width, lo_height, hi_features, width, height, work, out, resolved, &a,
                                           "apt_film_upscale_device");
    if (rc) return rc;
    const unsigned lo_blocks = blocks_for((uint64_t)lo_width * lo_height, kUpBlock);
    const unsigned blocks = blocks_for((uint64_t)width * height, kUpBlock);
    hipLaunchKernelGGL(film_upscale_prepare_kernel, dim3(lo_blocks), dim3(kUpBlock), 0, (hipStream_t)stream, a);
    if (int e = launched()) return e;
    hipLaunchKernelGGL(film_upscale_kernel, dim3(blocks), dim3(kUpBlock), 0, (hipStream_t)stream, a);
    return launched();
}

int apt_film_upscale_patch_device(void *stream, const float *sums, const uint32_t *list, uint64_t list_count, uint32_t passes,
                                  uint64_t pixel_count, float *out) {
    apt::stage_clear_error();
    const int rc = apt::film_upscale_patch_check(sums, list, list_count, passes, pixel_count, out, "apt_film_upscale_patch_device");
    if (rc) return rc;
    if (list_count == 0) return APT_OK;
    const unsigned blocks = blocks_for(list_count, kUpBlock);
    hipLaunchKernelGGL(film_upscale_patch_kernel, dim3(blocks), dim3(kUpBlock), 0, (hipStream_t)stream, sums, list, list_count, (float)passes,
                       pixel_count, out);
    return launched();
}

} // extern "C"
