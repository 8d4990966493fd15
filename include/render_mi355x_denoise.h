/* render_mi355x_denoise.h -- C-ABI of libdenoise_mi355x.so: the denoiser of the material renderer's film (render_mi355x.h "film" and
 * "features"): per-pixel luminance moments collected pass by pass, and an albedo-demodulated, variance-guided, edge-avoiding a-trous
 * filter with a CPU twin of every step.  A library and a header of their own: render_mi355x.h and the export list of
 * librender_mi355x.so are what they were, so a caller that does not denoise links and loads nothing new.  The library needs no symbol
 * of librender_mi355x.so: it works on the buffers that library's film and feature entries fill.  Status codes are render_mi355x.h's
 * APT_OK / APT_ERR_*; the error text of a refused call is this library's own, per thread: apt_film_denoise_last_error(). */
#ifndef RENDER_MI355X_DENOISE_H
#define RENDER_MI355X_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#include "render_mi355x.h"   /* APT_OK, APT_ERR_*, APT_FEATURE_* */

#ifdef __cplusplus
extern "C" {
#endif

/* libdenoise_mi355x.so is built with -fvisibility=hidden and librender_mi355x.so's export list (csrc/apt_exports.map): what this
 * header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- denoise (EXTENSION: per-pixel luminance moments of a film, and an albedo-demodulated, variance-guided, edge-avoiding a-trous
 * filter over a film and its feature planes) ------------------------------------------------------------------------------------------
 * A film of a few passes is noisy, and the feature planes say where its edges are.  The moments record how noisy each pixel is; the
 * filter divides the first surface's albedo out, smooths the remaining illumination across pixels whose guides agree, by as much as
 * the pixel's own variance allows, and multiplies the albedo back.  Opt-in: no frame kernel changes, and nothing of render_mi355x.h:
 * APT_ABI_VERSION stays 3 and librender_mi355x.so exports what it exported.  Every step below is one IEEE fp32 operation (no FMA, no transcendental; the divide and
 * the square root are correctly rounded); max(a, b) is the select a > b ? a : b, so a NaN `a` falls to b.
 * lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b.
 *
 * Moments.  apt_film_accumulate_device (DEVICE pointers, asynchronous on `stream`) and apt_film_accumulate_host (HOST pointers, the CPU
 * twin: the same operations, the same bits), elementwise over pixel_count pixels:
 *   - pass_planes is [3][pixel_count] float32 and holds exactly ONE pass: the (float)v a film pass adds.  film is [3][pixel_count],
 *     moments [2][pixel_count] float32, laid out beside the film and band-relative like it: plane 0 is the sum of l, plane 1 the sum
 *     of l * l over the passes, l = lum(r, g, b) of the pass.
 *   - pass == 0: film[c] = r_c, moments = (l, l * l): stores, whatever the buffers held, NaN included, is gone.  pass > 0:
 *     film[c] = film[c] + r_c, m0 = m0 + l, m1 = m1 + l * l, each one fp32 operation.
 *   - A caller gets one pass by itself from apt_render_frame_film with the pass's index into a scratch film, zeroed first when the
 *     index is > 0 (the entry adds then): 0 + r == r bit for bit for every r but -0, and a pass of non-negative radiance holds no
 *     -0.  The film that results is bit for bit the film the direct entry accumulates.
 *   - Refusals, nothing written: APT_ERR_ARG for a NULL pass_planes, film or moments, or a pixel_count beyond one launch's limit
 *     (the resolve's).  pixel_count == 0 is APT_OK.
 *
 * Filter.  apt_film_denoise_device (DEVICE pointers, asynchronous on `stream`) and apt_film_denoise_host (HOST pointers, the CPU twin).
 * Whole images only: film [3][N], moments [2][N], features [APT_FEATURE_PLANES][N] and out [3][N], N = width * height, x-major (pixel
 * (x, y) at x * height + y).  A band has no neighbours to read: there is no band form.  out holds the MEAN radiance, not a sum:
 * apt_film_resolve_* takes it with passes = 1.  work is the caller's buffer of apt_film_denoise_work_floats(width, height) =
 * 16 * N floats, 16-byte aligned.  The entry allocates nothing and keeps no state.  work holds four arrays of N 16-byte per-pixel
 * records, in this order: (n.xyz, z), (A.rgb, cov), and two (i.rgb, vi) images c[0], c[1]; prepare writes c[0] and iteration j
 * reads c[j & 1] and writes the other, so afterwards c[iterations & 1] is the last iteration's result and the other one its input.
 *   Prepare, per pixel, K = (float)passes (exact):
 *       c_ch = film_ch / K
 *       A_ch = max(albedo_ch + (1 - coverage), albedo_floor)    (a miss counts as albedo 1; an emitter of albedo 0 gets the floor)
 *       i_ch = c_ch / A_ch                                       (the demodulated illumination)
 *       lm = m0 / K;  q = m1 / K;  v = max(q - lm * lm, 0) / (float)(passes - 1)     (variance of the pixel's mean luminance)
 *       LA = lum(A);  vi = v / (LA * LA)
 *     The guides of the pixel are n (3), z, A (3) and cov as the feature planes hold them; the mean normal is not renormalised.
 *   Iteration j = 0 .. iterations - 1, step s = 1 << j, reads one (i, vi) image and writes the other, never in place.  At pixel
 *   p = (x, y):
 *       gv  = (sum of b * vi_q) / (sum of b) over ex = -1..1 (outer), ey = -1..1 (inner), q = (x + ex, y + ey) inside the image,
 *             b = B[ex] * B[ey], B = (1, 2, 1); both sums start from 0 and run in that order
 *       isd = 1 / (sqrt(gv) * sigma_l + 1e-6f)
 *       iz  = 1 / (z_p + 1e-6f)
 *       W = S_ch = V = 0;  for dx = -2..2 (outer), dy = -2..2 (inner), q = (x + dx * s, y + dy * s) inside the image:
 *           x_n = sigma_n * max(cov_p * cov_q - dot(n_p, n_q), 0)           (dot as ((0 + x) + y) + z)
 *           x_z = (sigma_z * |z_p - z_q|) * iz
 *           x_c = sigma_c * |cov_p - cov_q|
 *           x_a = sigma_a * ((|A_r,p - A_r,q| + |A_g,p - A_g,q|) + |A_b,p - A_b,q|)
 *           x_l = |lum(i_p) - lum(i_q)| * isd
 *           x   = (((x_n + x_z) + x_c) + x_a) + x_l
 *           t = max(1 - x * 0.125f, 0);  t = t * t;  t = t * t;  g = t * t   ((1 - x / 8)^8: e^-x with compact support)
 *           the centre tap, dx = dy = 0, has x = 0 by definition: g = 1 whatever its guides are (the mean normal of a pixel that
 *           straddles two surfaces is shorter than its coverage, so x_n of a pixel with itself is not 0, and neither is a NaN's x)
 *           w = H[dx][dy] * g              (H[dx][dy] = h[dx] * h[dy], h = (1, 4, 6, 4, 1) / 16: every entry exact in fp32)
 *           W = W + w;  S_ch = S_ch + w * i_q,ch;  V = V + (w * w) * vi_q
 *       i'_ch = S_ch / W;  vi' = V / (W * W)                                  (W >= 9 / 64: the centre tap)
 *   Finish: out_ch = i_ch * A_ch.
 *   apt_film_denoise_default_host fills the record for `passes`: iterations = 5, albedo_floor = 1 / 32, and the sigmas DESIGN.md
 *   "Denoise" records the tuning of.  APT_ERR_ARG for a NULL record (passes is checked by the filter entries).
 *   Refusals of both filter forms, nothing written: APT_ERR_ARG for a NULL d, film, moments, features, work or out, a work that is
 *   not 16-byte aligned, a zero width or height, passes outside 2 .. 2^24, iterations outside 1 .. 5, a sigma that is not finite or
 *   is negative, an albedo_floor that is not finite and > 0, more than 2^28 pixels (one launch's limit: the kernels index pixels in
 *   32 bits); APT_ERR_STRUCT for a wrong struct_size.
 *   Out of scope: bands; ascendpathtracing_amd/dist.py and apt_multi_*; temporal reprojection; a form for the mirror renderer; guides
 *   seen through mirrors or glass -- the FIRST surface is the guide, so a reflection is protected by the luminance term alone. */
typedef struct apt_film_denoise {
    uint32_t struct_size;       /* = sizeof(apt_film_denoise)                                                */
    uint32_t passes;            /* passes in the film and the moments, 2 .. 2^24                             */
    uint32_t iterations;        /* a-trous iterations, 1 .. 5: steps 1, 2, 4, 8, 16                          */
    uint32_t reserved;          /* not read                                                                  */
    float sigma_n, sigma_z, sigma_c, sigma_a, sigma_l;   /* finite, >= 0: normal, depth, coverage, albedo, luminance */
    float albedo_floor;         /* finite, > 0                                                               */
} apt_film_denoise;
int apt_film_accumulate_device(void *stream, const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass);
int apt_film_accumulate_host(const float *pass_planes, uint64_t pixel_count, float *film, float *moments, uint32_t pass);
int apt_film_denoise_default_host(apt_film_denoise *d, uint32_t passes);
uint64_t apt_film_denoise_work_floats(uint32_t width, uint32_t height);
int apt_film_denoise_device(const apt_film_denoise *d, void *stream, const float *film, const float *moments, const float *features,
                            uint32_t width, uint32_t height, float *work, float *out);
int apt_film_denoise_host(const apt_film_denoise *d, const float *film, const float *moments, const float *features, uint32_t width,
                          uint32_t height, float *work, float *out);

/* This thread's last refusal by an entry above ("" after a call that returned APT_OK): every entry clears it on entry. */
const char *apt_film_denoise_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RENDER_MI355X_DENOISE_H */
