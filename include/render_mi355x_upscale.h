/* render_mi355x_upscale.h -- C-ABI of libupscale_mi355x.so: guided upscaling for the material renderer's film (render_mi355x.h "film"
 * and "features"; render_mi355x_denoise.h).  Radiance is what a frame pays for, the feature planes are cheap: a frame may trace its
 * radiance at a lower resolution and its planes at the full one, and the entries here rebuild full-size radiance from the small film
 * under the guidance of the full-size planes -- joint bilateral upsampling of the albedo-demodulated illumination, so albedo edges and
 * silhouettes come back as sharp as the planes hold them.  A library and a header of their own, the seventh: the other six libraries,
 * their headers and export lists and APT_ABI_VERSION are what they were, and the library needs no symbol of theirs.  Status codes are
 * render_mi355x.h's APT_OK / APT_ERR_*; the error text of a refused call is this library's own, per thread:
 * apt_film_upscale_last_error(). */
#ifndef RENDER_MI355X_UPSCALE_H
#define RENDER_MI355X_UPSCALE_H

#include <stddef.h>
#include <stdint.h>

#include "render_mi355x.h"   /* APT_OK, APT_ERR_*, APT_FEATURE_* */

#ifdef __cplusplus
extern "C" {
#endif

/* libupscale_mi355x.so is built with -fvisibility=hidden and librender_mi355x.so's export list (csrc/apt_exports.map): what this
 * header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- guided upscaling (EXTENSION) ---------------------------------------------------------------------------------------------------
 * Conventions: render_mi355x_denoise.h's.  Every `_device` entry takes DEVICE pointers and is asynchronous on `stream`; its `_host`
 * twin takes HOST pointers, runs the same operations and gives the same bits.  The entries allocate nothing and keep no state.
 *
 * Buffers.  Whole images only, x-major (pixel (x, y) at x * height + y).  The low image has Nl = lo_width * lo_height pixels, the full
 * one N = width * height; 1 <= lo_width <= width, 1 <= lo_height <= height, N <= 2^28.  The ratio need not be an integer, and the two
 * axes may have different ratios.
 *   lo            [3][Nl] float32: the MEAN radiance of the low image (a film divided by its passes, a denoiser's output, a history's
 *                 radiance).
 *   lo_features   [APT_FEATURE_PLANES][Nl], hi_features [APT_FEATURE_PLANES][N] float32, as apt_render_frame_features writes them for
 *                 the SAME camera at the two sizes.
 *   out           [3][N] float32: mean radiance; apt_film_resolve_* takes it with passes = 1.  STORED.
 *   resolved      [N] uint32: 1 where the guided sum decided the pixel, 0 where the fallback did.  STORED.
 *   work          the caller's buffer of apt_film_upscale_work_floats(lo_width, lo_height) = 12 * Nl floats, 16-byte aligned: three
 *                 arrays of Nl 16-byte records, in this order: (i.rgb, cov), (n.xyz, z), (A.rgb, 0).  STORED; its contents after a call
 *                 are part of the contract (twin and device agree on every word), so a tap is three 16-byte loads, not eleven gathers.
 *   Whatever out, resolved and work held, NaN included, is gone.  None of them is an input or one another (compared as pointers; an
 *   overlap that is not an equality is the caller's error).
 *
 * Every fp32 step below is one IEEE operation (no FMA; the divides are correctly rounded); max(a, b) is the select a > b ? a : b, so a
 * NaN `a` falls to b.  cov, z, n (3) and albedo (3) are the feature planes' values as they are; the mean normal is not renormalised.
 *
 * Prepare, per low pixel q:
 *       A_q,ch = max(albedo_ch + (1 - cov), albedo_floor)        (the denoiser's rule: a miss counts as albedo 1)
 *       i_q,ch = lo_ch / A_q,ch                                  (the demodulated illumination)
 *   and the three records of q are stored.
 *
 * Coordinates, per full-size pixel p = (x, y): float64, every operation rounded on its own, NO FMA, the divide correctly rounded; the
 * sizes and pixel indices widen exactly.
 *       u = ((x + 0.5) * lo_width) / width - 0.5;    x0 = floor(u);  fx = u - x0
 *       v = ((y + 0.5) * lo_height) / height - 0.5;  y0 = floor(v);  fy = v - y0
 *   The four taps, in TAP ORDER ex = 0, 1 (outer), ey = 0, 1 (inner): q = (x0 + ex, y0 + ey), with the bilinear weight of their corner
 *       b_q = (float)((ex ? fx : 1 - fx) * (ey ? fy : 1 - fy))      (one float64 product, rounded once to fp32)
 *   A tap is INSIDE iff 0 <= x0 + ex <= lo_width - 1 and 0 <= y0 + ey <= lo_height - 1, compared in float64, before any conversion to
 *   an integer; a tap outside is skipped.  u lies in [-0.5, lo_width - 0.5), so along each axis an inside tap with a factor >= 0.5
 *   exists: at least one inside tap has b_q >= 0.25.
 *
 * Guided sum.  The guides of p are n_p, z_p, cov_p as hi_features holds them, A_p by the rule above from p's albedo and coverage, and
 * iz = 1 / (z_p + 1e-6f).  Per inside tap, the denoiser's terms WITHOUT its luminance term and WITHOUT a centre exception (no tap is
 * the pixel itself):
 *       x_n = sigma_n * max(cov_p * cov_q - dot(n_p, n_q), 0)           (dot as ((0 + x) + y) + z)
 *       x_z = (sigma_z * |z_p - z_q|) * iz
 *       x_c = sigma_c * |cov_p - cov_q|
 *       x_a = sigma_a * ((|A_r,p - A_r,q| + |A_g,p - A_g,q|) + |A_b,p - A_b,q|)
 *       x   = ((x_n + x_z) + x_c) + x_a
 *       t = max(1 - x * 0.125f, 0);  t = t * t;  t = t * t;  g = t * t
 *       w = b_q * g
 *   A tap ENTERS the sums only when w > 0 (a branch, not a product with 0: a zero-weight tap never meets a NaN or an infinite
 *   illumination):
 *       Wg = Wg + w;   S_ch = S_ch + w * i_q,ch           (all start from 0 and run in tap order)
 *   A NaN guide gives g = 0 by the max, so the tap does not enter.
 *
 * Decision.  Wg >= min_weight (written so that a NaN fails it):  i_p = S / Wg, resolved[p] = 1.
 *   Otherwise the FALLBACK, resolved[p] = 0: the same sums with g = 1, i.e. w = b_q, over the inside taps with b_q > 0 -- plain bilinear
 *   interpolation of the illumination over the taps the image has, renormalised.  Its weight is >= 0.25 (above), so the divide is safe.
 *   Either way  out_ch = i_p,ch * A_p,ch.
 *   Decisions this header takes where the outline left them open: the fallback's sums are separate accumulators that run over the same
 *   taps in the same order (an implementation may keep them beside the guided ones in one loop); a NaN illumination under a tap that
 *   enters reaches out; x_z may be negative for a negative z_p (planes never hold one), then g > 1 and nothing is clamped.
 *
 * The unresolved pixels need no compaction of their own.  The UNCHANGED apt_film_select_device / _host (render_mi355x_adaptive.h) with
 * a record of base_passes = 2, min_passes = 3, max_passes = 3, `resolved` passed as `extra` and ANY valid [2][N] buffer as `moments`
 * select pixel p exactly when resolved[p] == 0: a pixel with extra = 0 stands at 2 passes, below min_passes, and is selected before a
 * moment is used; one with extra = 1 stands at max_passes and is not, also before a moment is used.  The list comes out strictly
 * ascending.  It is what APT_FLAG_PIXEL_LIST of apt_render_frame_film takes: a list pass at FULL resolution gives each listed pixel,
 * in a compact scratch, the bits a whole pass of the same index gives it.
 *
 * Patch.  apt_film_upscale_patch_device / _host: the listed pixels of `out` [3][pixel_count] replaced by the mean of `passes` list
 * passes.  sums is [3][list_count] float32 (the compact scratch films of the passes, added up by the caller), list [list_count] uint32.
 *       for i < list_count, p = list[i] < pixel_count:   out[c][p] = sums[c][i] / (float)passes          (passes exact: <= 2^24)
 *   An entry with p >= pixel_count is skipped.  A repeated entry is the caller's error: one of its values stays; nothing faults.
 *   list_count == 0 is APT_OK and writes nothing.  Refusals: APT_ERR_ARG for a NULL pointer, passes outside 1 .. 2^24, pixel_count
 *   outside 1 .. 2^28, list_count > 2^28, out == sums.
 *
 * apt_film_upscale_default_host fills the record with the denoiser's values: sigma_n = 32, sigma_z = 10, sigma_c = 8, sigma_a = 8,
 * albedo_floor = 1 / 32, and min_weight = 2^-6.  These values are NOT TUNED for this use: they are the ones the denoiser was tuned
 * with, on another kernel footprint.  APT_ERR_ARG for a NULL record.
 *
 * Refusals of both upscale forms, nothing written: APT_ERR_ARG for a NULL pointer, a zero size, a low size above the full one,
 * N > 2^28, a work that is not 16-byte aligned, out, resolved or work equal to an input or to one another, a sigma that is not finite
 * or is negative, an albedo_floor that is not finite and > 0, a min_weight outside (0, 1] (a NaN is outside); APT_ERR_STRUCT for a
 * wrong struct_size.
 *
 * The kernels compute each lane's two coordinate chains themselves: that a column's x0 and fx are the same for a run of lanes is not
 * used (DESIGN.md "Upscale" says why).
 * Out of scope: bands; ascendpathtracing_amd/dist.py and apt_multi_*; the mirror renderer; a footprint wider than 2 x 2; a variance
 * output for the denoiser; temporal upscaling; tuning of the defaults; any change to the other six libraries. */
typedef struct apt_film_upscale {
    uint32_t struct_size;       /* = sizeof(apt_film_upscale)                                                  */
    uint32_t reserved;          /* not read                                                                    */
    float sigma_n, sigma_z, sigma_c, sigma_a;   /* finite, >= 0: normal, depth, coverage, albedo               */
    float albedo_floor;         /* finite, > 0                                                                 */
    float min_weight;           /* in (0, 1]: the least guided weight of a resolved pixel                      */
} apt_film_upscale;
int apt_film_upscale_default_host(apt_film_upscale *rec);
uint64_t apt_film_upscale_work_floats(uint32_t lo_width, uint32_t lo_height);
int apt_film_upscale_device(const apt_film_upscale *rec, void *stream, const float *lo, const float *lo_features, uint32_t lo_width,
                            uint32_t lo_height, const float *hi_features, uint32_t width, uint32_t height, float *work, float *out,
                            uint32_t *resolved);
int apt_film_upscale_host(const apt_film_upscale *rec, const float *lo, const float *lo_features, uint32_t lo_width, uint32_t lo_height,
                          const float *hi_features, uint32_t width, uint32_t height, float *work, float *out, uint32_t *resolved);
int apt_film_upscale_patch_device(void *stream, const float *sums, const uint32_t *list, uint64_t list_count, uint32_t passes,
                                  uint64_t pixel_count, float *out);
int apt_film_upscale_patch_host(const float *sums, const uint32_t *list, uint64_t list_count, uint32_t passes, uint64_t pixel_count,
                                float *out);

/* This thread's last refusal by an entry above ("" after a call that returned APT_OK): every entry clears it on entry. */
const char *apt_film_upscale_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RENDER_MI355X_UPSCALE_H */
