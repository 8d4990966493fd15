// adaptive.hip -- the device side of libadaptive_mi355x.so (include/render_mi355x_adaptive.h): the three kernels of the select's
// ordered stream compaction, the list accumulate and the mean, with their launches and the device entries of the C-ABI.  A library of
// its own (`make asm` writes its code object to adaptive.s).  The arithmetic of every step is adaptive_ops.h, which
// adaptive_host.cpp's CPU twins call too; the entries' checks are adaptive_host.cpp's.
//
// The select: one lane = one pixel, kAdBlock = 256 pixels = four waves per workgroup.  A wave's 64 predicates are one 64-bit ballot;
// its popcount is the wave's count, the popcount of the bits below a lane that lane's rank.  Launch 1 leaves each workgroup's count in
// work[]; launch 2 -- ONE workgroup -- turns work[] into exclusive prefix sums, 256 counts a turn with the running total carried in a
// register, and stores the total as *count; launch 3 computes the predicates again and stores pixel p at
// work[workgroup] + (counts of the waves before) + rank.  The launches are ordered by the stream: no workgroup waits for another and
// no atomic decides a position, so the list is the ascending one whatever the hardware schedules first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x_adaptive.h"
#include "adaptive_host.h"
#include "adaptive_ops.h"
#include "film_stage_launch.h"

using apt::AdSelect;
using apt::blocks_for;
using apt::kAdBlock;
using apt::launched;

namespace {

constexpr uint32_t kAdWaves = kAdBlock / 64;
static_assert(kAdBlock == 256, "four waves per workgroup");

struct SelArgs {
    const float *mom;
    const uint32_t *extra;
    uint32_t *work, *list;
    uint32_t n;                    // <= 2^28
    AdSelect s;
};

__device__ __forceinline__ bool select_lane(const SelArgs &a, uint32_t p) {
    bool sel = false;
    if (p < a.n) sel = apt::ad_selected(a.mom[p], a.mom[a.n + p], a.extra[p], a.s);
    return sel;
}

__global__ __launch_bounds__(kAdBlock) void film_select_count_kernel(SelArgs a) {
    __shared__ uint32_t wsum[kAdWaves];
    const uint32_t p = blockIdx.x * kAdBlock + threadIdx.x;
    const unsigned long long b = __ballot(select_lane(a, p));
    if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) a.work[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ONE workgroup: work[0 .. nblocks) -> its exclusive prefix sums, *count = the total (<= n <= 2^28: no overflow)
__global__ __launch_bounds__(kAdBlock) void film_select_scan_kernel(uint32_t *work, uint32_t nblocks, uint32_t *count) {
    __shared__ uint32_t wtot[kAdWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t first = 0; first < nblocks; first += kAdBlock) {           // (uniform: every thread reaches the barriers)
        const uint32_t i = first + threadIdx.x;
        const uint32_t v = i < nblocks ? work[i] : 0u;
        uint32_t inc = v;                                                    // inclusive scan over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t t = __shfl_up(inc, d, 64);
            if (lane >= d) inc += t;
        }
        if (lane == 63u) wtot[wave] = inc;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kAdWaves; ++w) {
            const uint32_t t = wtot[w];
            if (w < wave) before += t;
            total += t;
        }
        if (i < nblocks) work[i] = carry + before + (inc - v);
        carry += total;
        __syncthreads();                                                     // wtot is written again in the next turn
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(kAdBlock) void film_select_scatter_kernel(SelArgs a) {
    __shared__ uint32_t wsum[kAdWaves];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t p = blockIdx.x * kAdBlock + threadIdx.x;
    const bool sel = select_lane(a, p);
    const unsigned long long b = __ballot(sel);
    if (lane == 0u) wsum[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < kAdWaves; ++w)
        if (w < wave) before += wsum[w];
    const uint32_t rank = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    const uint32_t at = a.work[blockIdx.x] + before + rank;
    if (sel && at < a.n) a.list[at] = p;        // at < count <= n for unchanged moments; the compare keeps a store inside the list regardless
}

// ---- accumulate a list pass, and the mean: one lane = one entry / one pixel ----------------------------------------------------------------
struct AccListArgs {
    const float *pass;
    const uint32_t *list;
    float *film, *mom;
    uint32_t *extra;
    uint64_t count, n;
};

__global__ __launch_bounds__(kAdBlock) void film_accumulate_list_kernel(AccListArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kAdBlock + threadIdx.x;
    if (i >= a.count) return;
    apt::ad_accumulate(a.pass, a.list, a.count, a.film, a.mom, a.extra, a.n, i);
}

struct MeanArgs {
    const float *film;
    const uint32_t *extra;
    float *out;
    uint64_t n;
    uint32_t base;
};

__global__ __launch_bounds__(kAdBlock) void film_mean_kernel(MeanArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kAdBlock + threadIdx.x;
    if (i >= a.n) return;
    apt::ad_mean(a.film, a.extra, a.base, a.out, a.n, i);                     // (extra null or not: launch-uniform)
}

} // namespace

extern "C" {

int apt_film_select_device(const apt_film_select *s, void *stream, const float *moments, const uint32_t *extra, uint64_t pixel_count,
                           uint32_t *work, uint32_t *list, uint32_t *count) {
    apt::stage_clear_error();
    const int rc = apt::film_select_check(s, moments, extra, pixel_count, work, list, count, "apt_film_select_device");
    if (rc) return rc;
    SelArgs a;
    a.mom = moments; a.extra = extra; a.work = work; a.list = list; a.n = (uint32_t)pixel_count;   // <= 2^28: the check above
    a.s = AdSelect{s->base_passes, s->min_passes, s->max_passes, s->threshold, s->floor};
    const unsigned blocks = (unsigned)apt_film_select_work_words(pixel_count);                      // = blocks_for(pixel_count, kAdBlock)
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(film_select_count_kernel, dim3(blocks), dim3(kAdBlock), 0, st, a);
    hipLaunchKernelGGL(film_select_scan_kernel, dim3(1), dim3(kAdBlock), 0, st, work, (uint32_t)blocks, count);
    hipLaunchKernelGGL(film_select_scatter_kernel, dim3(blocks), dim3(kAdBlock), 0, st, a);
    return launched();
}

int apt_film_accumulate_list_device(void *stream, const float *pass_planes, const uint32_t *list, uint64_t list_count, uint64_t pixel_count,
                                    float *film, float *moments, uint32_t *extra) {
    apt::stage_clear_error();
    const int rc = apt::film_accumulate_list_check(pass_planes, list, list_count, pixel_count, film, moments, extra, "apt_film_accumulate_list_device");
    if (rc || list_count == 0) return rc;
    AccListArgs a;
    a.pass = pass_planes; a.list = list; a.film = film; a.mom = moments; a.extra = extra; a.count = list_count; a.n = pixel_count;
    const unsigned blocks = blocks_for(list_count, kAdBlock);
    hipLaunchKernelGGL(film_accumulate_list_kernel, dim3(blocks), dim3(kAdBlock), 0, (hipStream_t)stream, a);
    return launched();
}

int apt_film_mean_device(void *stream, const float *film, const uint32_t *extra, uint32_t base_passes, uint64_t pixel_count, float *out) {
    apt::stage_clear_error();
    const int rc = apt::film_mean_check(film, base_passes, pixel_count, out, "apt_film_mean_device");
    if (rc) return rc;
    MeanArgs a;
    a.film = film; a.extra = extra; a.out = out; a.n = pixel_count; a.base = base_passes;
    const unsigned blocks = blocks_for(pixel_count, kAdBlock);
    hipLaunchKernelGGL(film_mean_kernel, dim3(blocks), dim3(kAdBlock), 0, (hipStream_t)stream, a);
    return launched();
}

} // extern "C"
