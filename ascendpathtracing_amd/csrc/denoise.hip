// denoise.hip -- the device side of libdenoise_mi355x.so (include/render_mi355x_denoise.h): the accumulate kernel, and the prepare,
// iteration and finish kernels of the albedo-demodulated, variance-guided a-trous filter, with their launches and the two device
// entries of the C-ABI.  A library of its own (`make asm` writes its code object to denoise.s): librender_mi355x.so, its code objects
// and its export list are what they were.  A kernel is its lane mapping and one call: the arithmetic of every step, and the layout
// of the work buffer, are denoise_ops.h, which denoise_host.cpp's CPU twins call too; the entries' checks are denoise_host.cpp's.
//
// Pixel (x, y) is at x * height + y, so y is the contiguous direction and consecutive lanes of a wave own consecutive y of one column:
// a tap is that column run shifted, three 16-byte loads per lane and 1 KiB contiguous per wave instruction.  The iteration kernel
// keeps everything in registers: no LDS, no barrier, and a lane outside the image leaves at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x_denoise.h"
#include "denoise_host.h"
#include "denoise_ops.h"
#include "film_stage_launch.h"

using apt::DnRec;
using apt::DnSigma;

namespace {

constexpr int kDnBlock = 256;      // 1-D kernels: one lane = one pixel
constexpr int kDnRun = 64;         // iteration kernel: a wave's run of y ...
constexpr int kDnCols = 4;         // ... and the workgroup's columns, one per wave
static_assert(kDnRun * kDnCols == kDnBlock, "one wave per column");

// ---- moments ----------------------------------------------------------------------------------------------------------------------
struct AccArgs {
    const float *pass;
    float *film, *mom;
    uint64_t n;
    uint32_t first;                // pass == 0: store
};

__global__ __launch_bounds__(kDnBlock) void film_accumulate_kernel(AccArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    apt::dn_accumulate(a.pass, a.film, a.mom, a.n, i, a.first);                 // (first: launch-uniform)
}

// ---- prepare and finish ----------------------------------------------------------------------------------------------------------------
struct PrepArgs {
    const float *film, *mom, *feat;
    DnRec *g0, *g1, *c0;
    uint32_t n;
    float K, K1, floor_;
};

__global__ __launch_bounds__(kDnBlock) void denoise_prepare_kernel(PrepArgs a) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    apt::dn_prepare(a.film, a.mom, a.feat, a.g0, a.g1, a.c0, a.n, i, a.K, a.K1, a.floor_);
}

struct FinishArgs {
    const DnRec *g1, *c;
    float *out;
    uint32_t n;
};

__global__ __launch_bounds__(kDnBlock) void denoise_finish_kernel(FinishArgs a) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    apt::dn_finish(a.g1, a.c, a.out, a.n, i);
}

// ---- one iteration -------------------------------------------------------------------------------------------------------------------------
struct IterArgs {
    const DnRec *g0, *g1, *in;
    DnRec *out;
    int32_t W, H, s;
    uint32_t runs;                 // workgroups along y: ceil(H / kDnRun)
    DnSigma sg;
};

__global__ __launch_bounds__(kDnBlock) void denoise_iterate_kernel(IterArgs a) {
    const uint32_t bx = blockIdx.x / a.runs, by = blockIdx.x - bx * a.runs;
    const int32_t x = (int32_t)(bx * kDnCols + (threadIdx.x >> 6));
    const int32_t y = (int32_t)(by * kDnRun + (threadIdx.x & 63u));
    if (x >= a.W || y >= a.H) return;
    apt::dn_iterate(a.g0, a.g1, a.in, a.out, a.W, a.H, a.s, a.sg, x, y);
}

} // namespace

namespace {

void film_accumulate(void *stream, const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass) {
    AccArgs a;
    a.pass = pass_planes; a.film = film; a.mom = moments; a.n = pixel_count; a.first = pass == 0 ? 1u : 0u;
    const unsigned blocks = apt::blocks_for(pixel_count, kDnBlock);        // <= 2^31 - 1: checked by the caller
    hipLaunchKernelGGL(film_accumulate_kernel, dim3(blocks), dim3(kDnBlock), 0, (hipStream_t)stream, a);
}

void film_denoise(const apt_film_denoise &d, void *stream, const float *film, const float *moments, const float *features, uint32_t width,
                  uint32_t height, float *work, float *out) {
    const uint32_t n = width * height;                                     // <= 2^28: checked by the caller
    DnRec *const g0 = reinterpret_cast<DnRec *>(work), *const g1 = g0 + n, *const c[2] = {g1 + n, g1 + 2 * (size_t)n};
    const unsigned blocks = apt::blocks_for(n, kDnBlock);
    PrepArgs p;
    p.film = film; p.mom = moments; p.feat = features; p.g0 = g0; p.g1 = g1; p.c0 = c[0]; p.n = n;
    p.K = (float)d.passes; p.K1 = (float)(d.passes - 1); p.floor_ = d.albedo_floor;
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3(blocks), dim3(kDnBlock), 0, (hipStream_t)stream, p);
    IterArgs it;
    it.g0 = g0; it.g1 = g1; it.W = (int32_t)width; it.H = (int32_t)height;
    it.runs = (height + kDnRun - 1) / kDnRun;
    it.sg = DnSigma{d.sigma_n, d.sigma_z, d.sigma_c, d.sigma_a, d.sigma_l};
    const unsigned tiles = it.runs * ((width + kDnCols - 1) / kDnCols);   // <= n
    for (uint32_t j = 0; j < d.iterations; ++j) {
        it.in = c[j & 1]; it.out = c[(j + 1) & 1]; it.s = 1 << j;
        hipLaunchKernelGGL(denoise_iterate_kernel, dim3(tiles), dim3(kDnBlock), 0, (hipStream_t)stream, it);
    }
    FinishArgs f;
    f.g1 = g1; f.c = c[d.iterations & 1]; f.out = out; f.n = n;
    hipLaunchKernelGGL(denoise_finish_kernel, dim3(blocks), dim3(kDnBlock), 0, (hipStream_t)stream, f);
}

} // namespace

extern "C" {

int apt_film_accumulate_device(void *stream, const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass) {
    apt::stage_clear_error();
    const int rc = apt::film_accumulate_check(pass_planes, pixel_count, film, moments, "apt_film_accumulate_device");
    if (rc || pixel_count == 0) return rc;
    film_accumulate(stream, pass_planes, pixel_count, film, moments, pass);
    return apt::launched();
}

int apt_film_denoise_device(const apt_film_denoise *d, void *stream, const float *film, const float *moments, const float *features,
                            uint32_t width, uint32_t height, float *work, float *out) {
    apt::stage_clear_error();
    const int rc = apt::film_denoise_check(d, film, moments, features, width, height, work, out, "apt_film_denoise_device");
    if (rc) return rc;
    film_denoise(*d, stream, film, moments, features, width, height, work, out);
    return apt::launched();
}

} // extern "C"
