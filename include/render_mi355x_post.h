/* render_mi355x_post.h -- C-ABI of libpost_mi355x.so: what stands between a film's mean radiance and its resolve (render_mi355x.h
 * "film"): METERING, an exposure derived from the image's own luminance histogram and adapted from frame to frame, and BLOOM, the
 * glare that carries the energy above a threshold into neighbouring pixels before the tone operator clips it.  Both read the planes
 * that Film.mean(), the denoiser (render_mi355x_denoise.h) or the history (render_mi355x_history.h) fill; bloom's output and the
 * metered exposure go to apt_film_resolve_* unchanged.  A library and a header of their own, as the denoiser's, the adaptive sampler's
 * and the history's: the other four headers and the export lists of the other four libraries are what they were.  The library needs
 * no symbol of the other four.  Status codes are render_mi355x.h's APT_OK / APT_ERR_*; the error text of a refused call is this
 * library's own, per thread: apt_film_post_last_error(). */
#ifndef RENDER_MI355X_POST_H
#define RENDER_MI355X_POST_H

#include <stddef.h>
#include <stdint.h>

#include "render_mi355x.h"   /* APT_OK, APT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* libpost_mi355x.so is built with -fvisibility=hidden and librender_mi355x.so's export list (csrc/apt_exports.map): what this
 * header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- conventions (EXTENSION) -----------------------------------------------------------------------------------------------------------
 * render_mi355x_denoise.h's.  Every `_device` entry takes DEVICE pointers and is asynchronous on `stream`; its `_host` twin takes HOST
 * pointers, runs the same operations and gives the same bits.  The entries allocate nothing and keep no state.  Every arithmetic step
 * below is ONE IEEE fp32 operation, no FMA, no transcendental; the divides are correctly rounded; max(a, b) is the select
 * a > b ? a : b;  lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b, the denoiser's.  bits(f) is the 32-bit pattern of the
 * float f.  K = (float)passes: a film holds SUMS over `passes` frames; planes of MEAN radiance go in with passes = 1.
 *
 * ---- metering ---------------------------------------------------------------------------------------------------------------------------
 * apt_film_meter_device / _host: the luminance histogram of film [3][pixel_count] float32 -> hist, APT_METER_WORDS uint32 words, STORED
 * (whatever they held is gone).  `film` may be a band of an image: the histograms of bands add word by word to the whole image's.
 * Per pixel i:
 *       c_ch = film[ch][i] / K;   l = lum(c)
 *       !(l > 0)  (zero, negative, NaN):  hist[256] counts it            (the pixels that take no part in the exposure)
 *       otherwise its bin is  clamp((int)(bits(l) >> 20) - 888, 0, 255):  the 8 exponent bits and the top 3 mantissa bits, 8 bins an
 *           octave over [2^-16, 2^16); what is smaller (subnormals too) goes to bin 0, what is larger and +inf to bin 255.
 *   The words sum to pixel_count (<= 2^28: no word overflows).  The binning is integer work on the bit pattern, so the result is exact
 *   and depends neither on the launch geometry nor on the order in which pixels arrive.  pixel_count == 0 is APT_OK with hist all zero
 *   (film and work are then not read and may be NULL).
 *   Device form: `work` holds apt_film_meter_work_words(pixel_count) uint32 words (at most 512 * APT_METER_WORDS), 4-byte aligned, every
 *   one of which a call may write.  Each workgroup counts into LDS sub-histograms of its own, one per wave, and stores their sum as one row
 *   of work with plain vector stores; a second launch sums the rows into hist.  No workgroup waits for another, no global atomic, no float
 *   atomic.  The loads are 16 bytes a lane when film is 16-byte aligned and pixel_count is a multiple of 4 (all three planes are then
 *   aligned), 4 bytes a lane otherwise.
 *
 * apt_film_exposure_host: hist (HOST, APT_METER_WORDS words) and the exposure `prev` of the frame before -> *exposure.  Host only: 257
 * words.  The selection is integer arithmetic in uint64:
 *       n = the sum of hist[0 .. 255];   n == 0 (nothing was metered):  *exposure = prev
 *       cum(b) = hist[0] + .. + hist[b];   P(q) = the smallest b with cum(b) * 65536 >= q * n      (the bin of percentile q / 65536)
 *       b_lo = P(low_q);   b_hi = P(high_q)
 *       C = the sum of hist[b], S = the sum of hist[b] * (2 b + 1) over the WHOLE bins b_lo .. b_hi;   m2 = S / C  (floor; C > 0)
 *       L = the float whose bits are (888 << 20) + (m2 << 19)
 *   m2 is the count-weighted mean position in half-bins, L the luminance there: a piecewise-linear log-average without a log or an exp.
 *   Then in fp32:
 *       t = key / L;   t = t < max_exposure ? t : max_exposure;   t = t > min_exposure ? t : min_exposure
 *       *exposure = adapt >= 1 ? t : prev + (t - prev) * adapt
 *   Pass the last frame's result as `prev`: with adapt < 1 the exposure follows the metered one frame by frame.  A film of constant
 *   luminance L0 inside the range is metered within half a bin: exposure * L0 / key lies in [16/17, 18/17].
 *
 * apt_film_meter_default_host fills the record for `passes`: low_q = 6554, high_q = 58982 (10 % .. 90 %), key = 0.18,
 * min_exposure = 2^-12, max_exposure = 2^12, adapt = 1.
 *
 * Refusals of the four entries, nothing written: APT_ERR_ARG for a NULL pointer (film and work with pixel_count == 0 excepted), passes
 * outside 1 .. 2^24, a percentile pair that is not 1 <= low_q <= high_q <= 65536, a key, min_exposure or max_exposure that is not
 * finite and positive, min_exposure > max_exposure, adapt outside [0, 1] or NaN, a prev that is not finite or negative, pixel_count
 * > 2^28; APT_ERR_STRUCT for a wrong struct_size.  Every entry that takes the record checks the whole record. */
#define APT_METER_BINS 256
#define APT_METER_WORDS 257
typedef struct apt_film_meter {
    uint32_t struct_size;       /* = sizeof(apt_film_meter)                                                     */
    uint32_t passes;            /* 1 .. 2^24: the frames the film holds (1: planes of mean radiance)            */
    uint32_t low_q, high_q;     /* 1 <= low_q <= high_q <= 65536: the metered percentile range, in 1/65536      */
    float key;                  /* finite, > 0: the luminance the metered one is mapped to                      */
    float min_exposure;         /* finite, > 0                                                                  */
    float max_exposure;         /* finite, >= min_exposure                                                      */
    float adapt;                /* 0 .. 1: the share of the way from prev to the metered exposure (1: all)      */
} apt_film_meter;
int apt_film_meter_default_host(apt_film_meter *m, uint32_t passes);
uint64_t apt_film_meter_work_words(uint64_t pixel_count);
int apt_film_meter_device(const apt_film_meter *m, void *stream, const float *film, uint64_t pixel_count, uint32_t *work, uint32_t *hist);
int apt_film_meter_host(const apt_film_meter *m, const float *film, uint64_t pixel_count, uint32_t *hist);
int apt_film_exposure_host(const apt_film_meter *m, const uint32_t *hist, float prev, float *exposure);

/* ---- bloom ------------------------------------------------------------------------------------------------------------------------------
 * apt_film_bloom_device / _host: film [3][N] float32 -> out [3][N] float32, the MEAN radiance plus the glare, for apt_film_resolve_*
 * with passes = 1.  Whole images only: N = width * height, 1 <= N <= 2^28, x-major (pixel (x, y) at x * height + y), as the
 * denoiser's.  `work` holds apt_film_bloom_work_floats(width, height, levels) floats, 16-byte aligned: the pyramid levels as 16-byte
 * per-pixel records (r, g, b, 0), every one of which a call writes.  out is STORED.  out == film is REFUSED (the pyramid is read from
 * film while out is written); any other overlap of the buffers is the caller's to avoid.
 *
 * Bright-pass, a pure function of film pixel p (recomputed wherever it is read; it is never stored):
 *       m_ch = film_ch / K
 *       x_ch = m_ch > 0 ? m_ch : 0;   x_ch = x_ch < cap ? x_ch : cap      (a NaN, a negative value and an infinite firefly never enter)
 *       l = lum(x);   g = max(l - threshold, 0) / max(l, 1e-6f);   v_ch = x_ch * g
 * Down, a source ws x hs -> wd = (ws + 1) >> 1, hd = (hs + 1) >> 1.  At (x, y), W and S_ch starting from 0, over the taps
 * (2x + dx, 2y + dy) INSIDE the source in the order dx = -1 .. 2 (outer), dy = -1 .. 2 (inner), with k = (1, 3, 3, 1):
 *       w = k[dx] * k[dy];   W = W + w;   S_ch = S_ch + w * v_ch
 *       down_ch = S_ch / W                                                 (taps outside are skipped and the sum renormalised)
 *   D_0 = down(bright image);  D_j = down(D_(j-1)),  j = 1 .. levels - 1.
 * Up, a coarse wc x hc -> a fine wf x hf.  Along each axis a fine index i reads the coarse indices i0 = (i - 1) >> 1 (arithmetic: -1
 * for i = 0) and i0 + 1, with the weights (0.25, 0.75) for an even i and (0.75, 0.25) for an odd one; both indices are clamped into
 * the coarse image.  u_ch starting from 0, over x-tap 0, 1 (outer), y-tap 0, 1 (inner):
 *       u_ch = u_ch + (wx * wy) * v_ch
 * Combine:
 *       U_(levels-1) = D_(levels-1);   U_j = D_j + spread * up(U_(j+1))    (one product, one add)
 *       B = up(U_0) at width x height;   out_ch = m_ch + intensity * B_ch
 *   A NaN of the film stays in its own pixel and reaches no other.  B >= 0 everywhere while 64 * cap stays finite.  A film whose
 *   luminance never exceeds the threshold comes out as film / K bit for bit (B = 0, and m + 0 is m, apart from m = -0 -> +0).
 *
 * apt_film_bloom_default_host fills the record for `passes`: levels = 5, threshold = 1, cap = 2^16, spread = 1, intensity = 0.05.
 * The values were NOT tuned: DESIGN.md "Post".
 * apt_film_bloom_work_floats: 4 * the sum of the level sizes, 0 for arguments the entries refuse.
 *
 * Refusals, nothing written: APT_ERR_ARG for a NULL pointer, a zero width or height, N > 2^28, a work that is not 16-byte aligned, out
 * == film, passes outside 1 .. 2^24, levels outside 1 .. 6, a threshold, spread or intensity that is not finite or negative, a cap
 * that is not finite and positive; APT_ERR_STRUCT for a wrong struct_size.
 *
 * Out of scope: any change to the resolve, the denoiser or the history; bands for bloom; ascendpathtracing_amd/dist.py and
 * apt_multi_*; the mirror renderer; lens-flare or anamorphic shapes; local (per-region) exposure; centre-weighted metering; tuning of
 * the defaults. */
typedef struct apt_film_bloom {
    uint32_t struct_size;       /* = sizeof(apt_film_bloom)                                                     */
    uint32_t passes;            /* 1 .. 2^24: the frames the film holds (1: planes of mean radiance)            */
    uint32_t levels;            /* 1 .. 6: pyramid levels                                                       */
    uint32_t reserved;          /* not read                                                                     */
    float threshold;            /* finite, >= 0: the luminance above which a pixel glares                       */
    float cap;                  /* finite, > 0: the most a channel of a pixel gives to the pyramid              */
    float spread;               /* finite, >= 0: the weight of each coarser level relative to the finer one     */
    float intensity;            /* finite, >= 0: the weight of the glare in the output                          */
} apt_film_bloom;
int apt_film_bloom_default_host(apt_film_bloom *b, uint32_t passes);
uint64_t apt_film_bloom_work_floats(uint32_t width, uint32_t height, uint32_t levels);
int apt_film_bloom_device(const apt_film_bloom *b, void *stream, const float *film, uint32_t width, uint32_t height, float *work, float *out);
int apt_film_bloom_host(const apt_film_bloom *b, const float *film, uint32_t width, uint32_t height, float *work, float *out);

/* This thread's last refusal by an entry above ("" after a call that returned APT_OK): every entry that returns a status clears it on
 * entry. */
const char *apt_film_post_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RENDER_MI355X_POST_H */
