// history.hip -- the device side of libhistory_mi355x.so (include/render_mi355x_history.h): the reprojection kernel and the export
// kernel with their launches and the device entries of the C-ABI.  A library of its own (`make asm` writes its code object to
// history.s).  The arithmetic of every step is history_ops.h, which history_host.cpp's CPU twins call too; the entries' checks are
// history_host.cpp's.
//
// The reprojection: one lane = one pixel, and the image is x-major, so consecutive lanes take consecutive y of one column (a
// workgroup's 256 lanes run on into the next column): the 3 + 5 reads of the current frame and the 6 stores are coalesced.  The four
// taps of neighbouring lanes are neighbours in the previous frame wherever the reprojection is smooth, so a wave's gathers of one
// plane fall into a few cache lines of two columns.  No LDS, no atomics, no state: the output is a function of the inputs alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x_history.h"
#include "history_host.h"
#include "film_stage_launch.h"
#include "history_ops.h"

using apt::blocks_for;
using apt::HsArgs;
using apt::kHsBlock;
using apt::launched;

namespace {

__global__ __launch_bounds__(kHsBlock) void film_history_kernel(HsArgs a) {
    const uint32_t i = blockIdx.x * kHsBlock + threadIdx.x;              // < 2^28 + 256
    if (i >= a.w * a.h) return;                                          // (w * h <= 2^28: the entry's check)
    const uint32_t x = i / a.h;
    apt::hs_pixel(a, x, i - x * a.h);
}

__global__ __launch_bounds__(kHsBlock) void film_history_export_kernel(const float *hist, float *film, float *mom, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kHsBlock + threadIdx.x;
    if (i >= n) return;
    apt::hs_export(hist, film, mom, n, i);
}

} // namespace

extern "C" {

int apt_film_history_device(const apt_film_history *rec, void *stream, const apt_camera *cur_cam, const apt_camera *prev_cam, const float *cur,
                            const float *cur_features, const float *prev_features, const float *prev_hist, uint32_t width, uint32_t height,
                            float *out_hist) {
    apt::stage_clear_error();
    HsArgs a;
    const int rc = apt::film_history_check(rec, cur_cam, prev_cam, cur, cur_features, prev_features, prev_hist, width, height, out_hist, &a,
                                           "apt_film_history_device");
    if (rc) return rc;
    const unsigned blocks = blocks_for((uint64_t)width * height, kHsBlock);
    hipLaunchKernelGGL(film_history_kernel, dim3(blocks), dim3(kHsBlock), 0, (hipStream_t)stream, a);
    return launched();
}

int apt_film_history_export_device(void *stream, const float *hist, uint64_t pixel_count, float *film, float *moments) {
    apt::stage_clear_error();
    const int rc = apt::film_history_export_check(hist, pixel_count, film, moments, "apt_film_history_export_device");
    if (rc) return rc;
    const unsigned blocks = blocks_for(pixel_count, kHsBlock);
    hipLaunchKernelGGL(film_history_export_kernel, dim3(blocks), dim3(kHsBlock), 0, (hipStream_t)stream, hist, film, moments, pixel_count);
    return launched();
}

} // extern "C"
