// denoise.hip -- the device side of libdenoise_mi355x.so (include/render_mi355x_denoise.h): the accumulate kernel, and the prepare,
// iteration and finish kernels of the albedo-demodulated, variance-guided a-trous filter, with their launches and the two device
// entries of the C-ABI.  A library of its own (`make asm` writes its code object to denoise.s): librender_mi355x.so, its code objects
// and its export list are what they were.  Every kernel is the header's text, one fp32 operation per line (-ffp-contract=off), and
// denoise_host.cpp's CPU twins are the same text again; the entries' checks are denoise_host.cpp's too.
//
// The work buffer holds per-pixel 16-byte records, pixel (x, y) at x * height + y as in every plane: g0 = (n.xyz, z), g1 = (A.rgb, cov)
// and two images c = (i.rgb, vi) that the iterations ping-pong between; prepare writes c[0], iteration j reads c[j & 1].  y is the
// contiguous direction, so consecutive lanes of a wave own consecutive y of one column: a tap is that column run shifted, three
// 16-byte loads per lane and 1 KiB contiguous per wave instruction.  The iteration kernel keeps everything in registers: no LDS, no
// barrier, and a lane outside the image leaves at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x_denoise.h"
#include "denoise_host.h"

namespace {

constexpr int kDnBlock = 256;      // 1-D kernels: one lane = one pixel
constexpr int kDnRun = 64;         // iteration kernel: a wave's run of y ...
constexpr int kDnCols = 4;         // ... and the workgroup's columns, one per wave
static_assert(kDnRun * kDnCols == kDnBlock, "one wave per column");

__device__ __forceinline__ float dn_lum(float r, float g, float b) {
    float l = 0.2126f * r;
    l = l + 0.7152f * g;
    return l + 0.0722f * b;
}
__device__ __forceinline__ float dn_max(float a, float b) { return a > b ? a : b; }

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
    const float r = a.pass[i], g = a.pass[a.n + i], b = a.pass[2 * a.n + i];
    const float l = dn_lum(r, g, b);
    const float l2 = l * l;
    if (a.first) {                 // (launch-uniform)
        a.film[i] = r; a.film[a.n + i] = g; a.film[2 * a.n + i] = b;
        a.mom[i] = l; a.mom[a.n + i] = l2;
    } else {
        a.film[i] = a.film[i] + r; a.film[a.n + i] = a.film[a.n + i] + g; a.film[2 * a.n + i] = a.film[2 * a.n + i] + b;
        a.mom[i] = a.mom[i] + l; a.mom[a.n + i] = a.mom[a.n + i] + l2;
    }
}

// ---- prepare and finish ----------------------------------------------------------------------------------------------------------------
struct PrepArgs {
    const float *film, *mom, *feat;
    float4 *g0, *g1, *c0;
    uint32_t n;
    float K, K1, floor_;
};

__global__ __launch_bounds__(kDnBlock) void denoise_prepare_kernel(PrepArgs a) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t n = a.n;
    const float cov = a.feat[APT_FEATURE_COVERAGE * n + i];
    const float u = 1.0f - cov;
    float A[3], il[3];
#pragma unroll
    for (uint64_t ch = 0; ch < 3; ++ch) {
        const float cm = a.film[ch * n + i] / a.K;
        A[ch] = dn_max(a.feat[(APT_FEATURE_ALBEDO + ch) * n + i] + u, a.floor_);
        il[ch] = cm / A[ch];
    }
    const float lm = a.mom[i] / a.K, q = a.mom[n + i] / a.K;
    const float v = dn_max(q - lm * lm, 0.0f) / a.K1;
    const float LA = dn_lum(A[0], A[1], A[2]);
    const float vi = v / (LA * LA);
    a.g0[i] = make_float4(a.feat[APT_FEATURE_NORMAL * n + i], a.feat[(APT_FEATURE_NORMAL + 1) * n + i], a.feat[(APT_FEATURE_NORMAL + 2) * n + i],
                          a.feat[APT_FEATURE_DEPTH * n + i]);
    a.g1[i] = make_float4(A[0], A[1], A[2], cov);
    a.c0[i] = make_float4(il[0], il[1], il[2], vi);
}

struct FinishArgs {
    const float4 *g1, *c;
    float *out;
    uint32_t n;
};

__global__ __launch_bounds__(kDnBlock) void denoise_finish_kernel(FinishArgs a) {
    const uint32_t i = blockIdx.x * kDnBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t n = a.n;
    const float4 c = a.c[i], g1 = a.g1[i];
    a.out[i] = c.x * g1.x;
    a.out[n + i] = c.y * g1.y;
    a.out[2 * n + i] = c.z * g1.z;
}

// ---- one iteration -------------------------------------------------------------------------------------------------------------------------
struct IterArgs {
    const float4 *g0, *g1, *in;
    float4 *out;
    int32_t W, H, s;
    uint32_t runs;                 // workgroups along y: ceil(H / kDnRun)
    float sn, sz, sc, sa, sl;
};

__global__ __launch_bounds__(kDnBlock) void denoise_iterate_kernel(IterArgs a) {
    const uint32_t bx = blockIdx.x / a.runs, by = blockIdx.x - bx * a.runs;
    const int32_t x = (int32_t)(bx * kDnCols + (threadIdx.x >> 6));
    const int32_t y = (int32_t)(by * kDnRun + (threadIdx.x & 63u));
    if (x >= a.W || y >= a.H) return;          // every index below is x * H + y of a pixel inside the image: < W * H <= 2^28
    const int32_t ip = x * a.H + y;

    float sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int32_t ex = -1; ex <= 1; ++ex)
#pragma unroll
        for (int32_t ey = -1; ey <= 1; ++ey) {
            const int32_t qx = x + ex, qy = y + ey;
            if ((uint32_t)qx < (uint32_t)a.W && (uint32_t)qy < (uint32_t)a.H) {
                const float b = (ex == 0 ? 2.0f : 1.0f) * (ey == 0 ? 2.0f : 1.0f);
                sv = sv + b * a.in[qx * a.H + qy].w;
                sw = sw + b;
            }
        }
    const float gv = sv / sw;
    float e = sqrtf(gv) * a.sl;
    e = e + 1e-6f;
    const float isd = 1.0f / e;
    const float4 n_p = a.g0[ip], a_p = a.g1[ip], c_p = a.in[ip];
    const float zz = n_p.w + 1e-6f;
    const float iz = 1.0f / zz;
    const float lp = dn_lum(c_p.x, c_p.y, c_p.z);

    float Wt = 0.0f, Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, V = 0.0f;
#pragma unroll
    for (int32_t dx = -2; dx <= 2; ++dx)
#pragma unroll
        for (int32_t dy = -2; dy <= 2; ++dy) {
            const int32_t qx = x + dx * a.s, qy = y + dy * a.s;               // s <= 16: no overflow
            if ((uint32_t)qx < (uint32_t)a.W && (uint32_t)qy < (uint32_t)a.H) {
                const int32_t iq = qx * a.H + qy;
                const float4 n_q = a.g0[iq], a_q = a.g1[iq], c_q = a.in[iq];
                const float cc = a_p.w * a_q.w;
                float dt = 0.0f + n_p.x * n_q.x;
                dt = dt + n_p.y * n_q.y;
                dt = dt + n_p.z * n_q.z;
                const float xn = a.sn * dn_max(cc - dt, 0.0f);
                const float xz = (a.sz * fabsf(n_p.w - n_q.w)) * iz;
                const float xc = a.sc * fabsf(a_p.w - a_q.w);
                float da = fabsf(a_p.x - a_q.x) + fabsf(a_p.y - a_q.y);
                da = da + fabsf(a_p.z - a_q.z);
                const float xa = a.sa * da;
                const float lq = dn_lum(c_q.x, c_q.y, c_q.z);
                const float xl = fabsf(lp - lq) * isd;
                float xs = xn + xz;
                xs = xs + xc;
                xs = xs + xa;
                xs = xs + xl;
                float t = dn_max(1.0f - xs * 0.125f, 0.0f);
                t = t * t;
                t = t * t;
                const float g = dx == 0 && dy == 0 ? 1.0f : t * t;            // the centre tap: x = 0 by definition (compile time)
                const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
                const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
                const float w = (hx * hy) * g;
                Wt = Wt + w;
                Sr = Sr + w * c_q.x;
                Sg = Sg + w * c_q.y;
                Sb = Sb + w * c_q.z;
                V = V + (w * w) * c_q.w;
            }
        }
    a.out[ip] = make_float4(Sr / Wt, Sg / Wt, Sb / Wt, V / (Wt * Wt));
}

} // namespace

namespace {

void film_accumulate(void *stream, const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass) {
    AccArgs a;
    a.pass = pass_planes; a.film = film; a.mom = moments; a.n = pixel_count; a.first = pass == 0 ? 1u : 0u;
    const uint64_t blocks = (pixel_count + kDnBlock - 1) / kDnBlock;      // <= 2^31 - 1: checked by the caller
    hipLaunchKernelGGL(film_accumulate_kernel, dim3((unsigned)blocks), dim3(kDnBlock), 0, (hipStream_t)stream, a);
}

void film_denoise(const apt_film_denoise &d, void *stream, const float *film, const float *moments, const float *features, uint32_t width,
                  uint32_t height, float *work, float *out) {
    const uint32_t n = width * height;                                     // <= 2^28: checked by the caller
    float4 *const g0 = reinterpret_cast<float4 *>(work), *const g1 = g0 + n, *const c[2] = {g1 + n, g1 + 2 * (size_t)n};
    const unsigned blocks = (n + kDnBlock - 1) / kDnBlock;
    PrepArgs p;
    p.film = film; p.mom = moments; p.feat = features; p.g0 = g0; p.g1 = g1; p.c0 = c[0]; p.n = n;
    p.K = (float)d.passes; p.K1 = (float)(d.passes - 1); p.floor_ = d.albedo_floor;
    hipLaunchKernelGGL(denoise_prepare_kernel, dim3(blocks), dim3(kDnBlock), 0, (hipStream_t)stream, p);
    IterArgs it;
    it.g0 = g0; it.g1 = g1; it.W = (int32_t)width; it.H = (int32_t)height;
    it.runs = (height + kDnRun - 1) / kDnRun;
    it.sn = d.sigma_n; it.sz = d.sigma_z; it.sc = d.sigma_c; it.sa = d.sigma_a; it.sl = d.sigma_l;
    const unsigned tiles = it.runs * ((width + kDnCols - 1) / kDnCols);   // <= n
    for (uint32_t j = 0; j < d.iterations; ++j) {
        it.in = c[j & 1]; it.out = c[(j + 1) & 1]; it.s = 1 << j;
        hipLaunchKernelGGL(denoise_iterate_kernel, dim3(tiles), dim3(kDnBlock), 0, (hipStream_t)stream, it);
    }
    FinishArgs f;
    f.g1 = g1; f.c = c[d.iterations & 1]; f.out = out; f.n = n;
    hipLaunchKernelGGL(denoise_finish_kernel, dim3(blocks), dim3(kDnBlock), 0, (hipStream_t)stream, f);
}

// -> APT_OK when the runtime took the launches, APT_ERR_DEVICE with its text otherwise
int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return APT_OK;
    apt::dn_set_error(APT_ERR_DEVICE, "%s", hipGetErrorString(e));
    (void)what;
    return APT_ERR_DEVICE;
}

} // namespace

extern "C" {

int apt_film_accumulate_device(void *stream, const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass) {
    apt::dn_clear_error();
    const int rc = apt::film_accumulate_check(pass_planes, pixel_count, film, moments, "apt_film_accumulate_device");
    if (rc || pixel_count == 0) return rc;
    film_accumulate(stream, pass_planes, pixel_count, film, moments, pass);
    return launched("apt_film_accumulate_device");
}

int apt_film_denoise_device(const apt_film_denoise *d, void *stream, const float *film, const float *moments, const float *features,
                            uint32_t width, uint32_t height, float *work, float *out) {
    apt::dn_clear_error();
    const int rc = apt::film_denoise_check(d, film, moments, features, width, height, work, out, "apt_film_denoise_device");
    if (rc) return rc;
    film_denoise(*d, stream, film, moments, features, width, height, work, out);
    return launched("apt_film_denoise_device");
}

} // extern "C"
