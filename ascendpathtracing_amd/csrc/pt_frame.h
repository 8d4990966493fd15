// pt_frame.h -- what render_frame_kernel (pt_kernels.h) and render_frame_mat_kernel (pt_materials.h) share around their pairwise
// sums: the frame arguments, the lane mapping, the camera parked in LDS, and the decode (data_visualization.py:36-57) with its packed
// 8-bit store.  The leaf loop itself (chains, butterfly, n % 8 tail, LDS stack) is written out in both kernels: the compiler optimises
// a helper on its own before it inlines it, and every driver form tried (the chain as a callable; the plan, stack and sum by reference,
// as constant / LDS address-space pointers or returned by value) changed the spills, scratch or VGPRs of most frame kernels.
// The kernels keep their __shared__ arrays (the camera, the 8-bit pixels) themselves and hand them in: declared here, they would be laid
// out differently in each kernel's LDS, and the kernels' code would change.  The decode takes FrameArgs by value: through a reference, the
// compiler simplifies it apart from the kernel's kernarg loads and the frame kernels gain SGPR spills.
#pragma once
#include "pt_trace.h"

namespace {

struct FrameArgs {
    Camera cam;
    uint32_t width, height, samples;
    uint64_t seed;
    uint64_t pixel_begin, pixel_count;
    float *fb;       // [3][pixel_count]
    uint8_t *fb_u8;  // [pixel_count][3] or null
};

// The camera frame (14 doubles) is only needed by ray-generate; parked in LDS it does not
// occupy 28 SGPRs across the bounce loop (they spilled to VGPR lanes otherwise).
__device__ __forceinline__ void park_camera(Camera &cam, const FrameArgs &fa) {
    if (threadIdx.x < sizeof(Camera) / sizeof(double)) (&cam.pos[0])[threadIdx.x] = (&fa.cam.pos[0])[threadIdx.x];
}

// The lane -> (pixel, sub-pixel, chain j) mapping.  GROUP lanes share one sub-pixel: lane j of the group owns numpy's pairwise
// accumulator r[j] (samples j, 8+j, 16+j, ...), so the summation order of np.mean is reproduced with a 3-step butterfly and no shared
// memory.  GROUP == 1 serves samples < 8 (numpy sums those sequentially).  The kernels copy the fields into locals and keep
// `lane = threadIdx.x & 63` as their own first line: read through `fl.` inside the kernels' lambdas, or with `lane` computed here,
// the frame kernels' register allocation changes.
template <int GROUP>
struct FrameLane {
    uint32_t j, sub;
    uint64_t pl;        // pixel of the lane, counted from fa.pixel_begin
    bool valid;         // pl < fa.pixel_count
    uint64_t q;         // the pixel (fa.pixel_begin for lanes past the range)
    uint32_t pi, pj, sy, sx;
    uint64_t pbase;     // path index of the sub-pixel's sample 0
};
template <int GROUP>
__device__ __forceinline__ FrameLane<GROUP> frame_lane(const FrameArgs &fa, uint32_t tid = threadIdx.x) {
    FrameLane<GROUP> f;
    const uint64_t L = (uint64_t)xcd_chunked_block<16>(blockIdx.x, gridDim.x) * kBlock + tid;
    f.j = (GROUP == 8) ? (uint32_t)(L & 7) : 0u;
    f.sub = (uint32_t)(L / GROUP) & 3u;
    f.pl = L / (4 * GROUP);
    f.valid = f.pl < fa.pixel_count;
    f.q = fa.pixel_begin + (f.valid ? f.pl : 0);
    f.pi = (uint32_t)(f.q / fa.height); f.pj = (uint32_t)(f.q % fa.height);
    f.sy = f.sub >> 1; f.sx = f.sub & 1;
    f.pbase = (f.q * 4 + f.sub) * fa.samples;
    return f;
}

// The same mapping for a list launch (APT_FLAG_PIXEL_LIST; pt_materials.h kMatList): lane pl's pixel is list[pl], the list's address
// travelling in fa.fb_u8, which a film launch never reads, and fa.pixel_count its length.  The pixel alone decides the camera ray, the
// path indices and so the roulette keys: a listed pixel gets the bits a launch over the whole image gives it.  Lanes past the end
// read list[0], never past it.  An entry beyond the image makes its lanes invalid (`beyond`, for the status word): like the lanes past
// the end they trace entry 0's pixel (pixel 0 when that entry is beyond the image itself) and write nothing.
template <int GROUP>
__device__ __forceinline__ FrameLane<GROUP> frame_lane_list(const FrameArgs &fa, bool &beyond, uint32_t tid = threadIdx.x) {
    FrameLane<GROUP> f;
    const uint32_t *const list = reinterpret_cast<const uint32_t *>(fa.fb_u8);
    const uint64_t npix = (uint64_t)fa.width * fa.height;
    const uint64_t L = (uint64_t)xcd_chunked_block<16>(blockIdx.x, gridDim.x) * kBlock + tid;
    f.j = (GROUP == 8) ? (uint32_t)(L & 7) : 0u;
    f.sub = (uint32_t)(L / GROUP) & 3u;
    f.pl = L / (4 * GROUP);
    const bool listed = f.pl < fa.pixel_count;
    uint64_t q = list[listed ? f.pl : 0];
    beyond = listed && q >= npix;
    f.valid = listed && q < npix;
    if (q >= npix) {
        q = list[0];
        if (q >= npix) q = 0;
    }
    f.q = q;
    const uint32_t q32 = (uint32_t)q;               // < width * height <= 2^32 (the entry's check): a 32-bit division
    f.pi = q32 / fa.height; f.pj = q32 - f.pi * fa.height;
    f.sy = f.sub >> 1; f.sx = f.sub & 1;
    f.pbase = (f.q * 4 + f.sub) * fa.samples;
    return f;
}

// decode_color: data_visualization.py:36-57
// The 8-bit pixels of a workgroup (kBlock / (4 * GROUP) consecutive pixels, 3 bytes each: a whole number of dwords that starts on a
// dword when the image does) leave as DWORD stores assembled in LDS (u8pack, the kernel's) instead of three byte stores per pixel from
// different waves: no partial dwords for the L2 to merge.  (Measured: what brought the frame's write traffic to exactly its size was the
// XCD-aware block mapping, pt_trace.h; this took the launch's fetched bytes from 0.88 to 0.83 MB.  Kept: it costs one barrier per workgroup.)
constexpr uint32_t frame_u8_words(int group) { return kBlock / (4 * group) * 3 / 4; }
// CHANNEL_LANES (GROUP == 8 only): one division and one set of gathers per wave half, see below.  The one-path frame kernels of
// pt_kernels.h keep the per-channel form: with the other one they spill more VGPRs.
template <int GROUP, bool CHANNEL_LANES = (GROUP == 8)>
__device__ __forceinline__ void frame_decode(const FrameArgs fa, uint64_t pl, bool valid, const float (&res)[3],
                                             uint32_t (&u8pack_kernel)[frame_u8_words(GROUP)]) {
    constexpr uint32_t kPixPerBlock = kBlock / (4 * GROUP), kU8Words = frame_u8_words(GROUP);
    // LDS pointers, not generic ones: the compiler would otherwise merge the two byte stores below into one flat store
    typedef __attribute__((address_space(3))) uint8_t lds_uint8;
    typedef __attribute__((address_space(3))) uint32_t lds_uint32;
    lds_uint32 *const u8pack = (lds_uint32 *)u8pack_kernel;
    static_assert(kPixPerBlock * 3 % 4 == 0, "a workgroup's 8-bit pixels are whole dwords");
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t pl0 = pl - (threadIdx.x / (4 * GROUP));                       // first pixel of this workgroup (wave-uniform arithmetic on L)
    const bool pack = fa.fb_u8 && pl0 + kPixPerBlock <= fa.pixel_count && (((uintptr_t)fa.fb_u8 + pl0 * 3) & 3u) == 0;   // workgroup-uniform
    const float fs = (float)fa.samples;
    const int gbase = (int)(lane & ~(uint32_t)(4 * GROUP - 1));
    if (GROUP == 8 && CHANNEL_LANES) {
        // After the butterfly the 8 lanes of a sub-pixel hold the same three sums, so lane c = lane & 7 of every sub-pixel carries channel c
        // (c < 3) through ONE division and one set of gathers -- the source lane gbase + sq * 8 + c has the same c, so it holds the channel
        // its reader wants -- and lanes 0..2 of a pixel finish and store one channel each: the operations of the per-channel form below
        // on the same values, once per wave half instead of three times.
        const uint32_t c = lane & 7u;
        const float sum = c == 0 ? res[0] : (c == 1 ? res[1] : res[2]);
        float mean;                                 // np.mean: float32 sum / count
        if ((fa.samples & (fa.samples - 1)) == 0) { // (wave-uniform) a power of two: 1 / count is exact, and sum * (1 / count) is the correctly rounded
                                                    // quotient just as sum / count is, denormal results included.  Its bits come from the scalar unit.
            const uint32_t inv = (127u - (uint32_t)__builtin_ctz(fa.samples)) << 23;
            mean = sum * __uint_as_float(inv);
        } else {
            mean = sum / fs;
        }
        double acc = 0.0;                           // :38 sum_color = zeros (float64)
#pragma unroll
        for (int sq = 0; sq < 4; ++sq) acc = acc + (double)__shfl(mean, gbase + sq * GROUP + (int)c, 64); // :41-45
        const double v = acc / 4;                   // :46
        const double cl = v < 0 ? 0 : (v > 1 ? 1 : v); // :54
        if (valid && (lane & (4 * GROUP - 1)) < 3) {
            fa.fb[(uint64_t)c * fa.pixel_count + pl] = (float)cl;
            const uint8_t b8 = (uint8_t)(cl * 255);                               // :55-57 truncation
            if (pack) ((lds_uint8 *)u8pack)[(threadIdx.x / (4 * GROUP)) * 3 + c] = b8;
            else if (fa.fb_u8) fa.fb_u8[pl * 3 + c] = b8;
        }
    } else {   // (GROUP == 1 has no other form: the four lanes of a pixel hold different sums, so a source lane cannot pre-select its reader's channel)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float mean = res[ch] / fs;            // np.mean: float32 sum / count
            double acc = 0.0;                           // :38 sum_color = zeros (float64)
#pragma unroll
            for (int sq = 0; sq < 4; ++sq) acc = acc + (double)__shfl(mean, gbase + sq * GROUP, 64); // :41-45
            const double v = acc / 4;                   // :46
            const double cl = v < 0 ? 0 : (v > 1 ? 1 : v); // :54
            if (valid && (lane & (4 * GROUP - 1)) == 0) {
                fa.fb[(uint64_t)ch * fa.pixel_count + pl] = (float)cl;
                const uint8_t b8 = (uint8_t)(cl * 255);                               // :55-57 truncation
                if (pack) ((lds_uint8 *)u8pack)[(threadIdx.x / (4 * GROUP)) * 3 + ch] = b8;
                else if (fa.fb_u8) fa.fb_u8[pl * 3 + ch] = b8;
            }
        }
    }
    if (pack) {                                     // (workgroup-uniform: every thread reaches the barrier)
        __syncthreads();
        if (threadIdx.x < kU8Words) reinterpret_cast<uint32_t *>(fa.fb_u8 + pl0 * 3)[threadIdx.x] = u8pack[threadIdx.x];
    }
}

// The film tail (include/render_mi355x.h "film"): frame_decode's gathers and float64 sum / 4 without :54's clip and without an 8-bit
// image -- so no u8pack and no barrier.  r = (float)v is stored (pass 0: whatever the film held is gone) or added to the film word in
// one fp32 add.  fa.fb is the film, [3][pixel_count]; every word has exactly one owner lane in the launch, hence no atomics.
template <int GROUP>
__device__ __forceinline__ void frame_film(const FrameArgs fa, uint64_t pl, bool valid, const float (&res)[3], bool add) {
    const uint32_t lane = threadIdx.x & 63;
    const float fs = (float)fa.samples;
    const int gbase = (int)(lane & ~(uint32_t)(4 * GROUP - 1));
    if (GROUP == 8) {   // channel c = lane & 7 through one division and one set of gathers per wave half, as in frame_decode
        const uint32_t c = lane & 7u;
        const float sum = c == 0 ? res[0] : (c == 1 ? res[1] : res[2]);
        float mean;                                 // np.mean: float32 sum / count
        if ((fa.samples & (fa.samples - 1)) == 0) { // (wave-uniform) a power of two: sum * (1 / count) is the correctly rounded quotient
            const uint32_t inv = (127u - (uint32_t)__builtin_ctz(fa.samples)) << 23;
            mean = sum * __uint_as_float(inv);
        } else {
            mean = sum / fs;
        }
        double acc = 0.0;                           // :38 sum_color = zeros (float64)
#pragma unroll
        for (int sq = 0; sq < 4; ++sq) acc = acc + (double)__shfl(mean, gbase + sq * GROUP + (int)c, 64); // :41-45
        const float r = (float)(acc / 4);           // :46, `pre` of the oracle's decode_color
        if (valid && (lane & (4 * GROUP - 1)) < 3) {
            float *const w = fa.fb + ((uint64_t)c * fa.pixel_count + pl);
            *w = add ? *w + r : r;
        }
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float mean = res[ch] / fs;            // np.mean: float32 sum / count
            double acc = 0.0;
#pragma unroll
            for (int sq = 0; sq < 4; ++sq) acc = acc + (double)__shfl(mean, gbase + sq * GROUP, 64);
            const float r = (float)(acc / 4);
            if (valid && (lane & (4 * GROUP - 1)) == 0) {
                float *const w = fa.fb + ((uint64_t)ch * fa.pixel_count + pl);
                *w = add ? *w + r : r;
            }
        }
    }
}

} // namespace
