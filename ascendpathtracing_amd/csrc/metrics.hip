// metrics.hip -- the device side of libmetrics_mi355x.so (include/render_mi355x_metrics.h): the compare kernel, the SSIM tile kernel,
// the kernel that sums a map and the fold, with their launches and the device entries of the C-ABI.  A library of its own (`make asm`
// writes its code object to metrics.s).  The arithmetic of every step is metrics_ops.h, which metrics_host.cpp's CPU twins call too;
// the entries' checks are metrics_host.cpp's.
//
// The sums.  The header's tree pairs adjacent terms first, so a reducing workgroup takes an ALIGNED chunk of 2^k terms: a lane holds four
// consecutive terms and adds them (t0 + t1) + (t2 + t3); a wave's 64 lanes then hold 64 consecutive nodes of level 2, and the xor
// butterfly over the strides 1, 2 .. 32 adds node 2i to node 2i + 1 level by level (both lanes of a pair compute the same IEEE sum);
// lane 0 of each wave leaves its node in LDS and the first lanes of wave 0 butterfly over those.  The workgroup stores ONE row of work
// with plain stores, and a second launch folds the rows by the same code.  Lanes past the end hold the padding's +0.0.  The maximum and
// the count ride along as integers.  No workgroup waits for another, no atomic: DESIGN.md "Metrics".
//
// SSIM.  The images are x-major, so consecutive lanes take consecutive y.  A workgroup owns a tile of 16 x 64 windows: it computes the two
// display luminances of its 26 x 74 source pixels into LDS (6 coalesced loads a pixel, each pixel read by at most 4 tiles), runs the x
// pass of the five planes from there into LDS (16 x 74 x 5 floats), the y pass from that, and stores s to the map.  39 KB of LDS: four
// workgroups a CU.  A lane's LDS reads are conflict-free: a wave reads 64 consecutive floats of one row.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x_metrics.h"
#include "film_stage_launch.h"
#include "metrics_host.h"
#include "metrics_ops.h"

using apt::kMxChunk;
using apt::kMxCompareRowWords;
using apt::kMxFoldRows;
using apt::launched;
using apt::MxRec;

namespace {

constexpr int kMxBlock = kMxChunk / 4;         // 256 lanes, four terms each
constexpr int kFoldBlock = kMxFoldRows / 4;    // 1024 lanes, four rows each

__device__ __forceinline__ uint64_t d2u(double d) { return (uint64_t)__double_as_longlong(d); }
__device__ __forceinline__ double u2d(uint64_t u) { return __longlong_as_double((long long)u); }

// One workgroup's nodes -> its root, valid in thread 0.  s: kS tree sums (each lane's node of level 2 on entry); with kCmp also the
// maximum of key and the sum of bad.  lds: kWaves rows of kS + 2 words.
template <int kS, bool kCmp, int kWaves>
__device__ __forceinline__ void block_tree(double s[kS], uint64_t &key, uint32_t &bad, uint64_t (*lds)[kS + 2]) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < kS; ++k) s[k] = s[k] + __shfl_xor(s[k], m);
        if (kCmp) {
            const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)key, m);
            key = other > key ? other : key;
            bad += __shfl_xor(bad, m);
        }
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kS; ++k) lds[wave][k] = d2u(s[k]);
        lds[wave][kS] = key;
        lds[wave][kS + 1] = bad;
    }
    __syncthreads();
    if (wave == 0) {
        const bool in = lane < (uint32_t)kWaves;
        const uint32_t w = in ? lane : 0u;
#pragma unroll
        for (int k = 0; k < kS; ++k) s[k] = in ? u2d(lds[w][k]) : 0.0;
        key = in ? lds[w][kS] : 0ull;
        bad = in ? (uint32_t)lds[w][kS + 1] : 0u;
#pragma unroll
        for (int m = 1; m < kWaves; m <<= 1) {
#pragma unroll
            for (int k = 0; k < kS; ++k) s[k] = s[k] + __shfl_xor(s[k], m);
            if (kCmp) {
                const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)key, m);
                key = other > key ? other : key;
                bad += __shfl_xor(bad, m);
            }
        }
    }
}

// ---- compare -------------------------------------------------------------------------------------------------------------------------------
struct CompareArgs {
    const float *a, *b;
    float *err_map;            // kMap
    uint64_t *work;            // [gridDim.x][kMxCompareRowWords]
    uint32_t n;                // <= 2^28
    MxRec p;
};

template <bool kVec, bool kMap>
__global__ __launch_bounds__(kMxBlock) void film_compare_kernel(CompareArgs g) {
    __shared__ uint64_t lds[kMxBlock / 64][6];
    const uint32_t i0 = blockIdx.x * kMxChunk + threadIdx.x * 4;         // < 2^28 + 1024: no overflow
    const size_t n = g.n;
    float pa[3][4], pb[3][4];
    if (kVec) {                                                            // n is a multiple of 4: a quad is inside or outside
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float4 va = make_float4(0.0f, 0.0f, 0.0f, 0.0f), vb = va;
            if (i0 < g.n) {
                va = *reinterpret_cast<const float4 *>(g.a + ch * n + i0);
                vb = *reinterpret_cast<const float4 *>(g.b + ch * n + i0);
            }
            pa[ch][0] = va.x; pa[ch][1] = va.y; pa[ch][2] = va.z; pa[ch][3] = va.w;
            pb[ch][0] = vb.x; pb[ch][1] = vb.y; pb[ch][2] = vb.z; pb[ch][3] = vb.w;
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool in = i0 + j < g.n;
                pa[ch][j] = in ? g.a[ch * n + i0 + j] : 0.0f;
                pb[ch][j] = in ? g.b[ch * n + i0 + j] : 0.0f;
            }
    }
    double t[4][4];                                                        // [sum][term of the quad]
    float se[4];
    uint64_t key = 0;
    uint32_t bad = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xa[3] = {pa[0][j], pa[1][j], pa[2][j]}, xb[3] = {pb[0][j], pb[1][j], pb[2][j]};
        apt::MxTerms m = apt::mx_pixel(xa, xb, i0 + j, g.p);
        if (!(i0 + j < g.n)) { m.se = 0.0f; m.cse = 0.0f; m.rse = 0.0f; m.ae = 0.0f; m.key = 0; m.bad = 0; }   // the padding
        t[0][j] = (double)m.se; t[1][j] = (double)m.cse; t[2][j] = (double)m.rse; t[3][j] = (double)m.ae;
        se[j] = m.se;
        key = m.key > key ? m.key : key;
        bad += m.bad;
    }
    if (kMap) {
        if (kVec) {
            if (i0 < g.n) *reinterpret_cast<float4 *>(g.err_map + i0) = make_float4(se[0], se[1], se[2], se[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < g.n) g.err_map[i0 + j] = se[j];
        }
    }
    double s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = (t[k][0] + t[k][1]) + (t[k][2] + t[k][3]);
    block_tree<4, true, kMxBlock / 64>(s, key, bad, lds);
    if (threadIdx.x == 0) {
        uint64_t *const row = g.work + (size_t)blockIdx.x * kMxCompareRowWords;
#pragma unroll
        for (int k = 0; k < 4; ++k) row[k] = d2u(s[k]);
        row[4] = key;
        row[5] = bad;
    }
}

// ---- the fold: rows of kS sums (kCmp: and key, bad) -> one row per workgroup, or the entry's result ----------------------------------------
struct FoldArgs {
    const uint64_t *src;
    uint64_t *dst;             // rows, or with `last` the result words
    uint32_t rows;
    uint32_t last;
    uint64_t n;                // `last`: what the result reports beside the sums
};

template <bool kCmp>
__global__ __launch_bounds__(kFoldBlock) void fold_kernel(FoldArgs g) {
    constexpr int kS = kCmp ? 4 : 1, kRow = kCmp ? (int)kMxCompareRowWords : 1;
    __shared__ uint64_t lds[kFoldBlock / 64][kS + 2];
    const uint32_t r0 = blockIdx.x * kMxFoldRows + threadIdx.x * 4;       // rows <= 2^18
    double t[kS][4];
    uint64_t key = 0;
    uint32_t bad = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = r0 + j < g.rows;
        const uint64_t *const row = g.src + (size_t)(in ? r0 + j : 0u) * kRow;
#pragma unroll
        for (int k = 0; k < kS; ++k) t[k][j] = in ? u2d(row[k]) : 0.0;
        if (kCmp) {
            const uint64_t rk = in ? row[4] : 0ull;
            key = rk > key ? rk : key;
            bad += in ? (uint32_t)row[5] : 0u;
        }
    }
    double s[kS];
#pragma unroll
    for (int k = 0; k < kS; ++k) s[k] = (t[k][0] + t[k][1]) + (t[k][2] + t[k][3]);
    block_tree<kS, kCmp, kFoldBlock / 64>(s, key, bad, lds);
    if (threadIdx.x == 0) {
        uint64_t *const out = g.last ? g.dst : g.dst + (size_t)blockIdx.x * kRow;
#pragma unroll
        for (int k = 0; k < kS; ++k) out[k] = d2u(s[k]);
        if (kCmp) {
            out[4] = key;
            out[5] = bad;
            if (g.last) { out[6] = g.n; out[7] = 0; }
        } else if (g.last) {
            out[1] = g.n;
        }
    }
}

// rows [r.r0] at `work` (and room for r.r1 more behind them) -> result
template <bool kCmp>
void fold_rows(uint64_t *work, apt::MxRows r, uint64_t *result, uint64_t n, hipStream_t stream) {
    constexpr int kRow = kCmp ? (int)kMxCompareRowWords : 1;
    FoldArgs f;
    f.src = work; f.rows = r.r0; f.n = n;
    if (r.r1) {
        f.dst = work + (size_t)r.r0 * kRow; f.last = 0;
        hipLaunchKernelGGL(fold_kernel<kCmp>, dim3(r.r1), dim3(kFoldBlock), 0, stream, f);
        f.src = f.dst; f.rows = r.r1;
    }
    f.dst = result; f.last = 1;
    hipLaunchKernelGGL(fold_kernel<kCmp>, dim3(1), dim3(kFoldBlock), 0, stream, f);
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------------------
constexpr int kTX = 16, kTY = 64, kHX = kTX + 10, kHY = kTY + 10;

struct SsimArgs {
    const float *a, *b;
    float *map;                // [(W - 10) * (H - 10)]
    uint32_t W, H, tiles_y;
    MxRec p;
};

__global__ __launch_bounds__(kMxBlock) void film_ssim_kernel(SsimArgs g) {
    __shared__ float ya[kHX][kHY], yb[kHX][kHY];
    __shared__ float hx[5][kTX][kHY];
    const uint32_t x0 = (blockIdx.x / g.tiles_y) * kTX, y0 = (blockIdx.x % g.tiles_y) * kTY;   // the tile's first window = its first source pixel
    const size_t N = (size_t)g.W * g.H;
    for (uint32_t idx = threadIdx.x; idx < kHX * kHY; idx += kMxBlock) {
        const uint32_t ix = idx / kHY, iy = idx - ix * kHY, px = x0 + ix, py = y0 + iy;
        float va = 0.0f, vb = 0.0f;
        if (px < g.W && py < g.H) {
            const size_t i = (size_t)px * g.H + py;
            va = apt::mx_display_lum(g.a[i], g.a[N + i], g.a[2 * N + i], g.p.Ka, g.p.inv_a, g.p.exposure);
            vb = apt::mx_display_lum(g.b[i], g.b[N + i], g.b[2 * N + i], g.p.Kb, g.p.inv_b, g.p.exposure);
        }
        ya[ix][iy] = va;
        yb[ix][iy] = vb;
    }
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < kTX * kHY; idx += kMxBlock) {
        const uint32_t ox = idx / kHY, iy = idx - ox * kHY;
        float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < APT_SSIM_TAPS; ++k) apt::mx_tap_source(acc, apt::mx_weight(k), ya[ox + k][iy], yb[ox + k][iy]);
#pragma unroll
        for (int q = 0; q < 5; ++q) hx[q][ox][iy] = acc[q];
    }
    __syncthreads();
    const uint32_t ww = g.W - 10, wh = g.H - 10;
    for (uint32_t idx = threadIdx.x; idx < kTX * kTY; idx += kMxBlock) {
        const uint32_t ox = idx / kTY, oy = idx - ox * kTY;
        float f[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < APT_SSIM_TAPS; ++k) {
            const float h[5] = {hx[0][ox][oy + k], hx[1][ox][oy + k], hx[2][ox][oy + k], hx[3][ox][oy + k], hx[4][ox][oy + k]};
            apt::mx_tap_planes(f, apt::mx_weight(k), h);
        }
        const float s = apt::mx_ssim(f);
        if (x0 + ox < ww && y0 + oy < wh) g.map[(size_t)(x0 + ox) * wh + (y0 + oy)] = s;
    }
}

// the map's floats as the terms of the tree: one row of one word per workgroup
template <bool kVec>
__global__ __launch_bounds__(kMxBlock) void map_sum_kernel(const float *map, uint32_t n, uint64_t *work) {
    __shared__ uint64_t lds[kMxBlock / 64][3];
    const uint32_t i0 = blockIdx.x * kMxChunk + threadIdx.x * 4;
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (kVec) {
        if (i0 < n) {
            const float4 q = *reinterpret_cast<const float4 *>(map + i0);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < n) v[j] = map[i0 + j];
    }
    double s[1] = {((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3])};
    uint64_t key = 0;
    uint32_t bad = 0;
    block_tree<1, false, kMxBlock / 64>(s, key, bad, lds);
    if (threadIdx.x == 0) work[blockIdx.x] = d2u(s[0]);
}

} // namespace

extern "C" {

int apt_film_compare_device(const apt_film_compare *c, void *stream, const float *a, const float *b, uint64_t pixel_count, double *work,
                            uint64_t *result, float *err_map) {
    apt::stage_clear_error();
    CompareArgs g;
    const int rc = apt::film_compare_check(c, a, b, pixel_count, work, true, result, err_map, &g.p, "apt_film_compare_device");
    if (rc) return rc;
    const apt::MxRows r = apt::mx_rows(pixel_count);
    g.a = a; g.b = b; g.err_map = err_map; g.work = reinterpret_cast<uint64_t *>(work); g.n = (uint32_t)pixel_count;
    const bool vec = (uintptr_t)a % 16 == 0 && (uintptr_t)b % 16 == 0 && pixel_count % 4 == 0 && (uintptr_t)err_map % 16 == 0;
    const dim3 grid(r.r0), block(kMxBlock);
    const hipStream_t s = (hipStream_t)stream;
    if (vec && err_map) hipLaunchKernelGGL((film_compare_kernel<true, true>), grid, block, 0, s, g);
    else if (vec) hipLaunchKernelGGL((film_compare_kernel<true, false>), grid, block, 0, s, g);
    else if (err_map) hipLaunchKernelGGL((film_compare_kernel<false, true>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((film_compare_kernel<false, false>), grid, block, 0, s, g);
    fold_rows<true>(g.work, r, result, pixel_count, s);
    return launched();
}

int apt_film_ssim_device(const apt_film_compare *c, void *stream, const float *a, const float *b, uint32_t width, uint32_t height, void *work,
                         uint64_t *result, float *ssim_map) {
    apt::stage_clear_error();
    SsimArgs g;
    const int rc = apt::film_ssim_check(c, a, b, width, height, work, true, result, ssim_map, &g.p, "apt_film_ssim_device");
    if (rc) return rc;
    const uint32_t ww = width - 10, wh = height - 10, windows = ww * wh;   // <= 2^28
    const apt::MxRows r = apt::mx_rows(windows);
    uint64_t *const rows = reinterpret_cast<uint64_t *>(work);
    const size_t row_words = ((size_t)r.r0 + r.r1 + 1) & ~(size_t)1;       // apt_film_ssim_work_bytes' layout: the map follows the rows
    g.a = a; g.b = b; g.W = width; g.H = height;
    g.map = ssim_map ? ssim_map : reinterpret_cast<float *>(rows + row_words);
    g.tiles_y = (wh + kTY - 1) / kTY;
    const uint32_t tiles_x = (ww + kTX - 1) / kTX;                         // tiles_x * tiles_y < 2^28 / 1024 + 2^24 / 16 + ..: no overflow
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(film_ssim_kernel, dim3(tiles_x * g.tiles_y), dim3(kMxBlock), 0, s, g);
    if ((uintptr_t)g.map % 16 == 0 && windows % 4 == 0)
        hipLaunchKernelGGL(map_sum_kernel<true>, dim3(r.r0), dim3(kMxBlock), 0, s, (const float *)g.map, windows, rows);
    else
        hipLaunchKernelGGL(map_sum_kernel<false>, dim3(r.r0), dim3(kMxBlock), 0, s, (const float *)g.map, windows, rows);
    fold_rows<false>(rows, r, result, windows, s);
    return launched();
}

} // extern "C"
