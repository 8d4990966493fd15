/* render_mi355x_metrics.h -- C-ABI of libmetrics_mi355x.so: how far one film is from another.  COMPARE, the mean-squared-error family
 * (squared, clipped squared, relative squared and absolute error, the largest difference and where it is) of a film against a
 * reference, and SSIM, the structural similarity of their display luminances.  Both read the planes that a film, Film.mean(), the
 * denoiser (render_mi355x_denoise.h), the history (render_mi355x_history.h) or the bloom (render_mi355x_post.h) fill, and write a few
 * 64-bit words: every sum is ONE fixed tree in float64, so a result is the same bits on the device and on the host, whatever the
 * launch geometry.  A library and a header of their own, as the other four film libraries': the other five headers and the export
 * lists of the other five libraries are what they were.  The library needs no symbol of the other five.  Status codes are
 * render_mi355x.h's APT_OK / APT_ERR_*; the error text of a refused call is this library's own, per thread:
 * apt_film_metrics_last_error(). */
#ifndef RENDER_MI355X_METRICS_H
#define RENDER_MI355X_METRICS_H

#include <stddef.h>
#include <stdint.h>

#include "render_mi355x.h"   /* APT_OK, APT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* libmetrics_mi355x.so is built with -fvisibility=hidden and librender_mi355x.so's export list (csrc/apt_exports.map): what this
 * header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- conventions (EXTENSION) -----------------------------------------------------------------------------------------------------------
 * render_mi355x_post.h's.  Every `_device` entry takes DEVICE pointers and is asynchronous on `stream`; its `_host` twin takes HOST
 * pointers, runs the same operations and gives the same bits.  The entries allocate nothing and keep no state.  Every fp32 step below
 * is ONE IEEE fp32 operation, no FMA, no transcendental; the divides are correctly rounded; max(a, b) is the select a > b ? a : b;
 * lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b, the denoiser's; clip01(e): t = e > 0 ? e : 0, then t < 1 ? t : 1.
 * bits(f) is the 32-bit pattern of the float f.  A film is [3][N] float32 SUMS over `passes` frames (K = (float)passes); planes of
 * MEAN radiance go in with passes = 1.  Images are x-major: pixel (x, y) at x * height + y.
 *
 * ---- the sum ----------------------------------------------------------------------------------------------------------------------------
 * Every sum of this library over n terms t_0 .. t_(n-1) (fp32 values) is the same fixed tree in float64:
 *       T(i, 0) = (double)t_i  for i < n,  +0.0 for i >= n
 *       T(i, l + 1) = T(2 i, l) + T(2 i + 1, l)
 *       the sum = T(0, L), L the smallest with 2^L >= n
 *   Adjacent pairs first: the result depends neither on the launch geometry nor on the order of arrival, and a device reduction that
 *   takes aligned chunks of 2^k terms -- four consecutive terms a lane, an xor butterfly over the strides 1, 2, 4 .. 32 of a wave, the
 *   waves of a workgroup in pairs, one row of `work` per workgroup, a second launch that folds the rows by the same tree -- gives
 *   exactly these bits.  No float atomic, no global atomic, no workgroup waits for another.  (A level of padding adds +0.0: it changes
 *   nothing but a -0.0 partial sum, which becomes +0.0.)
 *
 * ---- compare ----------------------------------------------------------------------------------------------------------------------------
 * apt_film_compare_device / _host: a [3][n] with passes_a against the reference b [3][n] with passes_b, 1 <= n <= 2^28, -> result,
 * APT_COMPARE_WORDS uint64 words, STORED.  a == b is allowed.  Per pixel i:
 *       x_ch = a[ch][i] / Ka;   y_ch = b[ch][i] / Kb
 *   The pixel is BAD when any of the six means has a biased exponent field ((bits >> 23) & 255) >= 187: |v| >= 2^60, an infinity or
 *   a NaN; an integer test on the bits.  A bad pixel contributes +0 to every sum, takes no part in the maximum, and is counted.
 *   Otherwise, with d_ch = x_ch - y_ch:
 *       se  = (d_r * d_r + d_g * d_g) + d_b * d_b
 *       ae  = (|d_r| + |d_g|) + |d_b|
 *       r_ch = (d_ch * d_ch) / (y_ch * y_ch + eps);   rse = (r_r + r_g) + r_b
 *       cse = se computed on clip01(x_ch * exposure) and clip01(y_ch * exposure)        (the project's "clipped MSE")
 *       ad  = max(max(|d_r|, |d_g|), |d_b|)
 *   result[0 .. 3] = the bit patterns of the tree sums of se, cse, rse, ae over the pixels
 *   result[4]      = the maximum over the good pixels of the key ((uint64)bits(ad) << 32) | (0xFFFFFFFF - i): the largest absolute
 *                    difference and the lowest pixel index that reaches it, by integer order; 0 when no pixel is good
 *   result[5]      = the number of bad pixels;   result[6] = n;   result[7] = 0
 *   The means of an error are the sums over 3 * (n - bad).
 *   err_map: NULL, or [n] float32 that receives se per pixel (0 for a bad pixel).
 *   Device form: `work` holds apt_film_compare_work_doubles(n) 8-byte words, 8-byte aligned, every one of which a call may write.  A
 *   workgroup takes an aligned chunk of 1024 pixels and stores one row of 6 words; a fold launch reduces up to 4096 rows to one, a
 *   second one follows beyond 4096 rows (n > 2^22).  The loads are 16 bytes a lane when a and b are 16-byte aligned, n is a multiple
 *   of 4 (all six planes are then aligned) and err_map is NULL or 16-byte aligned; 4 bytes a lane otherwise.  No mixed body and tail.
 *
 * apt_film_compare_default_host fills the record for the two pass counts: exposure = 1, eps = 1e-2f.
 * apt_film_compare_work_doubles: a function of n alone; 0 for an n the entries refuse.
 *
 * ---- SSIM -------------------------------------------------------------------------------------------------------------------------------
 * apt_film_ssim_device / _host: whole images a and b, width, height >= 11, width * height <= 2^28, with the same record -> result,
 * APT_SSIM_WORDS uint64 words, STORED.  The display luminance of each image, per pixel:
 *       Y = lum(clip01(m_r * exposure), clip01(m_g * exposure), clip01(m_b * exposure)),   m_ch = film[ch] / K
 *   Five planes: Ya, Yb, Ya * Ya, Yb * Yb, Ya * Yb (each product ONE operation at the source pixel).  Each goes through a separable
 *   11-tap Gaussian, sigma 1.5, weights w[0 .. 10] (apt_film_ssim_weights_host: exp(-(k - 5)^2 / 4.5) normalised in float64 and
 *   rounded once to fp32; symmetric):
 *       first, along x:   acc = 0;  acc = acc + w[k] * P(x - 5 + k, y),  k = 0 .. 10 in that order
 *       then, along y:    the same over the first pass's results
 *   VALID windows only: the centres 5 <= x < W - 5, 5 <= y < H - 5, window j = (x - 5) * (H - 10) + (y - 5).  Per window, from the
 *   filtered planes ma, mb, Eaa, Ebb, Eab, with C1 = 1e-4f, C2 = 9e-4f:
 *       maa = ma * ma;  mbb = mb * mb;  mab = ma * mb;   saa = Eaa - maa;  sbb = Ebb - mbb;  sab = Eab - mab
 *       s = ((2 * mab + C1) * (2 * sab + C2)) / (((maa + mbb) + C1) * ((saa + sbb) + C2))
 *   result[0] = the bits of the tree sum of s over j;   result[1] = the window count (W - 10) * (H - 10).  The mean SSIM is their
 *   quotient.  Identical images give s == 1.0f in every window (2 * (m * m) and m * m + m * m are the same float).
 *   ssim_map: NULL, or [(W - 10) * (H - 10)] float32 that receives s.
 *   Device form: `work` holds apt_film_ssim_work_bytes(W, H) bytes, 16-byte aligned: the rows of the reduction and, for a NULL
 *   ssim_map, the map.  A workgroup filters a tile of 16 x 64 windows from its 26 x 74 luminances in LDS, the x pass's five planes
 *   kept in LDS too, and stores s; the map is then summed as compare's terms are.
 *
 * Refusals, nothing written: APT_ERR_ARG for a NULL pointer (err_map and ssim_map excepted), n = 0 or n > 2^28, a width or height
 * below 11, width * height > 2^28, passes_a or passes_b outside 1 .. 2^24, an exposure or eps that is not finite and positive, a work
 * that is not aligned, result, err_map, ssim_map or work EQUAL to an input or to one another (any other overlap of the buffers is the
 * caller's to avoid); APT_ERR_STRUCT for a wrong struct_size.
 *
 * Out of scope: FLIP and other perceptual metrics; colour SSIM; multi-scale SSIM; bands for SSIM; any change to the other five
 * libraries or to any default. */
#define APT_COMPARE_WORDS 8
#define APT_SSIM_WORDS 2
#define APT_SSIM_TAPS 11
typedef struct apt_film_compare {
    uint32_t struct_size;       /* = sizeof(apt_film_compare)                                                   */
    uint32_t passes_a;          /* 1 .. 2^24: the frames film a holds (1: planes of mean radiance)              */
    uint32_t passes_b;          /* 1 .. 2^24: the frames the reference b holds                                  */
    uint32_t reserved;          /* not read                                                                     */
    float exposure;             /* finite, > 0: what the clipped error and SSIM multiply the means by           */
    float eps;                  /* finite, > 0: what the relative error adds to the squared reference           */
} apt_film_compare;
int apt_film_compare_default_host(apt_film_compare *c, uint32_t passes_a, uint32_t passes_b);
uint64_t apt_film_compare_work_doubles(uint64_t pixel_count);
int apt_film_compare_device(const apt_film_compare *c, void *stream, const float *a, const float *b, uint64_t pixel_count, double *work,
                            uint64_t *result, float *err_map);
int apt_film_compare_host(const apt_film_compare *c, const float *a, const float *b, uint64_t pixel_count, uint64_t *result, float *err_map);
int apt_film_ssim_weights_host(float *w);   /* w: APT_SSIM_TAPS floats */
uint64_t apt_film_ssim_work_bytes(uint32_t width, uint32_t height);
int apt_film_ssim_device(const apt_film_compare *c, void *stream, const float *a, const float *b, uint32_t width, uint32_t height, void *work,
                         uint64_t *result, float *ssim_map);
int apt_film_ssim_host(const apt_film_compare *c, const float *a, const float *b, uint32_t width, uint32_t height, uint64_t *result,
                       float *ssim_map);

/* This thread's last refusal by an entry above ("" after a call that returned APT_OK): every entry that returns a status clears it on
 * entry. */
const char *apt_film_metrics_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RENDER_MI355X_METRICS_H */
