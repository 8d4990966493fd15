// post.hip -- the device side of libpost_mi355x.so (include/render_mi355x_post.h): the meter's histogram and fold kernels and the
// bloom's down, combine and composite kernels, with their launches and the device entries of the C-ABI.  A library of its own (`make
// asm` writes its code object to post.s).  The arithmetic of every step is post_ops.h, which post_host.cpp's CPU twins call too; the
// entries' checks are post_host.cpp's.
//
// The meter.  A reduction of N pixels to 257 counters.  A workgroup of four waves strides over the image (16-byte loads of the three
// planes where they are aligned) and counts into LDS, one 257-word sub-histogram per wave (ds_add_u32: integer, so the order of arrival
// is of no account; a wave of its own keeps 64 lanes that hit one bin from meeting the other waves' too).  It then stores the sum of
// its four sub-histograms as ONE row of `work` with plain stores.  A second launch sums the rows, column by column, into hist.  No
// workgroup waits for another, nothing is cleared beforehand, and no global atomic is used: DESIGN.md "Post" says why that form.
// The form it was measured against is kept behind -DAPT_POST_METER_ATOMICS (never the product's build): hist is cleared on the stream
// and every workgroup adds its 257 sums to it with 32-bit integer global atomics; work is then not touched and the fold not launched.
//
// The bloom.  One lane = one destination pixel and the images are x-major, so consecutive lanes take consecutive y of one column (a
// workgroup's 256 lanes run on into the next column): a tap of a level is one 16-byte load per lane, the reads of the film planes and
// the stores of out are coalesced.  No LDS, no atomics; the small levels are a launch each (they are launch-bound; nothing is fused at
// the price of one workgroup waiting for another).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x_post.h"
#include "film_stage_launch.h"
#include "post_host.h"
#include "post_ops.h"

using apt::launched;
using apt::PoBloom;
using apt::PoRec;

namespace {

constexpr int kPoBlock = 256;
constexpr int kPoWaves = kPoBlock / 64;

// ---- meter ---------------------------------------------------------------------------------------------------------------------------------
struct MeterArgs {
    const float *film;
    uint32_t *work;            // [gridDim.x][APT_METER_WORDS]  (APT_POST_METER_ATOMICS: hist itself)
    uint32_t n;                // <= 2^28
    uint32_t quads;            // n / 4 when the planes take 16-byte loads, else 0
    float K;
};

__global__ __launch_bounds__(kPoBlock) void film_meter_kernel(MeterArgs a) {
    __shared__ uint32_t sub[kPoWaves][APT_METER_WORDS];
    uint32_t *const flat = &sub[0][0];
    for (uint32_t k = threadIdx.x; k < kPoWaves * APT_METER_WORDS; k += kPoBlock) flat[k] = 0;
    __syncthreads();
    uint32_t *const mine = sub[threadIdx.x >> 6];
    const uint32_t first = blockIdx.x * kPoBlock + threadIdx.x, stride = gridDim.x * kPoBlock;    // <= 2^17
    if (a.quads) {
        const float4 *const r4 = reinterpret_cast<const float4 *>(a.film), *const g4 = reinterpret_cast<const float4 *>(a.film + a.n),
                     *const b4 = reinterpret_cast<const float4 *>(a.film + 2 * (size_t)a.n);
        for (uint32_t q = first; q < a.quads; q += stride) {                                       // q < 2^26 + 2^17: no overflow
            const float4 r = r4[q], g = g4[q], b = b4[q];
            atomicAdd(&mine[apt::po_meter_bin(r.x, g.x, b.x, a.K)], 1u);
            atomicAdd(&mine[apt::po_meter_bin(r.y, g.y, b.y, a.K)], 1u);
            atomicAdd(&mine[apt::po_meter_bin(r.z, g.z, b.z, a.K)], 1u);
            atomicAdd(&mine[apt::po_meter_bin(r.w, g.w, b.w, a.K)], 1u);
        }
    } else {
        for (uint32_t i = first; i < a.n; i += stride)                                             // i < 2^28 + 2^17: no overflow
            atomicAdd(&mine[apt::po_meter_bin(a.film[i], a.film[a.n + i], a.film[2 * (size_t)a.n + i], a.K)], 1u);
    }
    __syncthreads();
#ifndef APT_POST_METER_ATOMICS
    uint32_t *const row = a.work + (size_t)blockIdx.x * APT_METER_WORDS;
#endif
    for (uint32_t k = threadIdx.x; k < APT_METER_WORDS; k += kPoBlock) {
        uint32_t s = sub[0][k];
        for (int w = 1; w < kPoWaves; ++w) s += sub[w][k];
#ifdef APT_POST_METER_ATOMICS
        if (s) atomicAdd(&a.work[k], s);
#else
        row[k] = s;
#endif
    }
}

// hist[c] = the sum of column c over the rows: 64 columns a workgroup, 16 row groups of 64 lanes each, folded through LDS
constexpr int kFoldCols = 64, kFoldGroups = 16;
__global__ __launch_bounds__(kFoldCols * kFoldGroups) void film_meter_fold_kernel(const uint32_t *work, uint32_t rows, uint32_t *hist) {
    __shared__ uint32_t part[kFoldGroups][kFoldCols];
    const uint32_t c = threadIdx.x & (kFoldCols - 1), g = threadIdx.x / kFoldCols, col = blockIdx.x * kFoldCols + c;
    uint32_t s = 0;
    if (col < APT_METER_WORDS)
        for (uint32_t r = g; r < rows; r += kFoldGroups) s += work[(size_t)r * APT_METER_WORDS + col];
    part[g][c] = s;
    __syncthreads();
    if (g == 0 && col < APT_METER_WORDS) {
        uint32_t t = 0;
        for (int k = 0; k < kFoldGroups; ++k) t += part[k][c];
        hist[col] = t;
    }
}

// ---- bloom ---------------------------------------------------------------------------------------------------------------------------------
struct DownArgs {
    apt::PoFilmSrc film;       // level 0: the bright image of the film ...
    apt::PoRecSrc rec;         // ... the others: the level before
    PoRec *dst;
    int32_t ws, hs, wd, hd;
};

template <bool kFromFilm>
__global__ __launch_bounds__(kPoBlock) void bloom_down_kernel(DownArgs a) {
    const uint32_t i = blockIdx.x * kPoBlock + threadIdx.x;              // < 2^26 + 256
    if (i >= (uint32_t)(a.wd * a.hd)) return;
    const int32_t x = (int32_t)(i / (uint32_t)a.hd), y = (int32_t)i - x * a.hd;
    if (kFromFilm) a.dst[i] = apt::po_down(a.film, a.ws, a.hs, x, y);
    else a.dst[i] = apt::po_down(a.rec, a.ws, a.hs, x, y);
}

struct CombineArgs {
    PoRec *d;                  // D_j in, U_j out
    const PoRec *c;            // U_(j+1)
    int32_t wf, hf, wc, hc;
    float spread;
};

__global__ __launch_bounds__(kPoBlock) void bloom_combine_kernel(CombineArgs a) {
    const uint32_t i = blockIdx.x * kPoBlock + threadIdx.x;
    if (i >= (uint32_t)(a.wf * a.hf)) return;
    const int32_t x = (int32_t)(i / (uint32_t)a.hf), y = (int32_t)i - x * a.hf;
    apt::po_combine(a.d, a.c, a.hf, a.wc, a.hc, a.spread, x, y);
}

struct CompositeArgs {
    const float *film;
    const PoRec *c;            // U_0
    float *out;
    int32_t W, H, wc, hc;
    float K, intensity;
};

__global__ __launch_bounds__(kPoBlock) void bloom_composite_kernel(CompositeArgs a) {
    const uint32_t i = blockIdx.x * kPoBlock + threadIdx.x;              // < 2^28 + 256
    if (i >= (uint32_t)(a.W * a.H)) return;
    const int32_t x = (int32_t)(i / (uint32_t)a.H), y = (int32_t)i - x * a.H;
    apt::po_composite(a.film, a.c, a.out, a.W, a.H, a.wc, a.hc, a.K, a.intensity, x, y);
}

unsigned blocks_of(int32_t w, int32_t h) { return apt::blocks_for((uint32_t)(w * h), kPoBlock); }   // a w x h level: w * h <= 2^28

void film_bloom(const PoBloom &b, hipStream_t stream) {
    const uint32_t n = (uint32_t)(b.W * b.H);
    for (uint32_t j = 0; j < b.levels; ++j) {
        DownArgs d;
        d.film = apt::PoFilmSrc{b.film, n, b.bright};
        d.rec = apt::PoRecSrc{j ? b.level[j - 1] : nullptr};
        d.dst = b.level[j];
        d.ws = j ? b.w[j - 1] : b.W; d.hs = j ? b.h[j - 1] : b.H; d.wd = b.w[j]; d.hd = b.h[j];
        if (j == 0) hipLaunchKernelGGL(bloom_down_kernel<true>, dim3(blocks_of(d.wd, d.hd)), dim3(kPoBlock), 0, stream, d);
        else hipLaunchKernelGGL(bloom_down_kernel<false>, dim3(blocks_of(d.wd, d.hd)), dim3(kPoBlock), 0, stream, d);
    }
    for (int32_t j = (int32_t)b.levels - 2; j >= 0; --j) {
        CombineArgs c;
        c.d = b.level[j]; c.c = b.level[j + 1]; c.wf = b.w[j]; c.hf = b.h[j]; c.wc = b.w[j + 1]; c.hc = b.h[j + 1]; c.spread = b.spread;
        hipLaunchKernelGGL(bloom_combine_kernel, dim3(blocks_of(c.wf, c.hf)), dim3(kPoBlock), 0, stream, c);
    }
    CompositeArgs f;
    f.film = b.film; f.c = b.level[0]; f.out = b.out; f.W = b.W; f.H = b.H; f.wc = b.w[0]; f.hc = b.h[0];
    f.K = b.bright.K; f.intensity = b.intensity;
    hipLaunchKernelGGL(bloom_composite_kernel, dim3(blocks_of(b.W, b.H)), dim3(kPoBlock), 0, stream, f);
}

} // namespace

extern "C" {

int apt_film_meter_device(const apt_film_meter *m, void *stream, const float *film, uint64_t pixel_count, uint32_t *work, uint32_t *hist) {
    apt::stage_clear_error();
    const int rc = apt::film_meter_check(m, film, pixel_count, work, true, hist, "apt_film_meter_device");
    if (rc) return rc;
    const uint32_t rows = apt::po_meter_rows(pixel_count);           // 0 without pixels: the fold then stores zeros and reads nothing
#ifdef APT_POST_METER_ATOMICS
    if (hipMemsetAsync(hist, 0, APT_METER_WORDS * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return launched();
    work = hist;
#endif
    if (rows) {
        MeterArgs a;
        a.film = film; a.work = work; a.n = (uint32_t)pixel_count; a.K = (float)m->passes;
        a.quads = ((uintptr_t)film % 16 == 0 && pixel_count % 4 == 0) ? (uint32_t)(pixel_count / 4) : 0u;
        hipLaunchKernelGGL(film_meter_kernel, dim3(rows), dim3(kPoBlock), 0, (hipStream_t)stream, a);
    }
#ifndef APT_POST_METER_ATOMICS
    hipLaunchKernelGGL(film_meter_fold_kernel, dim3((APT_METER_WORDS + kFoldCols - 1) / kFoldCols), dim3(kFoldCols * kFoldGroups), 0,
                       (hipStream_t)stream, work, rows, hist);
#endif
    return launched();
}

int apt_film_bloom_device(const apt_film_bloom *b, void *stream, const float *film, uint32_t width, uint32_t height, float *work, float *out) {
    apt::stage_clear_error();
    PoBloom a;
    const int rc = apt::film_bloom_check(b, film, width, height, work, out, &a, "apt_film_bloom_device");
    if (rc) return rc;
    film_bloom(a, (hipStream_t)stream);
    return launched();
}

} // extern "C"
