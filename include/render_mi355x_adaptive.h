/* render_mi355x_adaptive.h -- C-ABI of libadaptive_mi355x.so: adaptive sampling for the material renderer's film (render_mi355x.h
 * "film", render_mi355x_denoise.h "Moments").  After a few uniform passes the film's luminance moments say how uncertain each pixel's
 * mean still is; the entries here pick the pixels that are, as an ordered list for a list pass (render_mi355x.h APT_FLAG_PIXEL_LIST),
 * add such a pass to the film, and normalise a film whose pixels hold different numbers of passes.  A library and a header of their
 * own, as the denoiser's: render_mi355x.h's prototypes, render_mi355x_denoise.h and the export lists of librender_mi355x.so and
 * libdenoise_mi355x.so are what they were.  The library needs no symbol of the other two.  Status codes are render_mi355x.h's
 * APT_OK / APT_ERR_*; the error text of a refused call is this library's own, per thread: apt_film_adaptive_last_error(). */
#ifndef RENDER_MI355X_ADAPTIVE_H
#define RENDER_MI355X_ADAPTIVE_H

#include <stddef.h>
#include <stdint.h>

#include "render_mi355x.h"   /* APT_OK, APT_ERR_* */

#ifdef __cplusplus
extern "C" {
#endif

/* libadaptive_mi355x.so is built with -fvisibility=hidden and librender_mi355x.so's export list (csrc/apt_exports.map): what this
 * header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- adaptive sampling (EXTENSION) -------------------------------------------------------------------------------------------------
 * Conventions: render_mi355x_denoise.h's.  Every step below is one IEEE fp32 operation (no FMA; the divide and the square root are
 * correctly rounded); max(a, b) is the select a > b ? a : b, so a NaN `a` falls to b;
 * lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b.  Every `_device` entry takes DEVICE pointers and is asynchronous on
 * `stream`; its `_host` twin takes HOST pointers, runs the same operations and gives the same bits.  The entries allocate nothing
 * and keep no state.
 *
 * Data.  Whole images only: N = width * height pixels, 1 <= N <= 2^28, x-major as everywhere.  film [3][N] and moments [2][N] float32
 * are what apt_film_accumulate_* fills; they hold `base` uniform passes, 2 <= base <= 2^24.  extra [N] uint32 counts the passes a
 * pixel received BEYOND base: a new film zeroes it (a memset).  A pixel's sample count is n_u = base + extra[p] (a 64-bit sum: no
 * wrap-around).  The accumulate and resolve entries of the other two libraries, and what a film means without `extra`, are untouched.
 *
 * Select.  apt_film_select_device / apt_film_select_host: which pixels get another pass.  Per pixel p, m0 = moments[p],
 * m1 = moments[N + p]:
 *     n_u >= max_passes                  -> not selected
 *     otherwise n_u < min_passes         -> selected
 *     otherwise, in this order:
 *         n  = (float)n_u                 (exact: n_u < max_passes <= 2^24)
 *         lm = m0 / n;  s = m1 / n
 *         d  = max(s - lm * lm, 0)
 *         v  = d / (float)(n_u - 1)       (render_mi355x_denoise.h's variance of the pixel's mean luminance)
 *         e  = sqrt(v)
 *         r  = max(lm, floor)
 *         t  = threshold * r
 *         selected iff e > t              (e == t is not selected)
 *   A NaN moment falls to d = 0 (max) or fails the compare (a NaN e or t): such a pixel is NOT selected once it has min_passes.
 *   `list` has N uint32 words of capacity and receives the selected pixel indices in STRICTLY ASCENDING order; `count` is ONE uint32
 *   -- in DEVICE memory for the device form, in HOST memory for the twin -- and receives their number.  list words from `count` on
 *   are not written.  The caller reads `count` back (one 4-byte copy per round) to size the list launch.  `work` is the caller's
 *   buffer of apt_film_select_work_words(N) uint32 words (one per 256 pixels); the twin takes one as well and does not touch it.  The
 *   device form is an ordered stream compaction in three plain launches on `stream` -- per-workgroup counts from 64-bit ballots, one
 *   workgroup's scan of the counts, ranks from the ballot prefix -- in which no workgroup waits for another and no atomic decides a
 *   position: the output is a function of the input alone.
 *   apt_film_select_default_host fills the record for `base_passes`: threshold = 0.1, floor = 1 / 16, min_passes = the larger of
 *   base_passes and 4, max_passes = the larger of 16 * base_passes and min_passes (at most 2^24).  DESIGN.md "Adaptive sampling"
 *   records the run these values were taken from, and how little it settles.  APT_ERR_ARG for a NULL record or a base_passes
 *   outside 2 .. 2^24.
 *   Selection reads the same samples the estimate is made of: a pixel whose first passes happen to agree stops early, which biases
 *   the film's mean slightly (towards the values that looked converged).  min_passes is the guard: no pixel is judged on fewer.
 *
 * Accumulate a list pass.  apt_film_accumulate_list_device / _host: pass_planes is [3][list_count] float32, the compact scratch a
 * list launch of apt_render_frame_film fills (word c * list_count + i holds entry i's pixel).  For each i < list_count, p = list[i]:
 *     p >= N: skipped (the list launch left that entry's scratch words untouched: they stay out of the film)
 *     otherwise, one fp32 operation each:  film[c][p] = film[c][p] + pass[c][i];  l = lum(pass[.][i]);  m0[p] = m0[p] + l;
 *     m1[p] = m1[p] + l * l;  and extra[p] = extra[p] + 1.
 *   A list with a repeated entry is the caller's error: which of the adds wins is unspecified; nothing faults.
 *
 * Mean.  apt_film_mean_device / _host: out[c][p] = film[c][p] / (float)(base + extra[p]), out [3][N] float32; extra may be NULL,
 * which stands for all zero.  apt_film_resolve_* takes `out` with passes = 1, as it takes the denoiser's; its first step divides,
 * and x / 1 is exact, so with extra all zero the result is bit for bit what the resolve makes of the film with passes = base.
 *
 * Refusals, nothing written: APT_ERR_ARG for a NULL pointer (but mean's extra), N == 0 or N > 2^28, list_count > N, a base outside
 * 2 .. 2^24, a record with min_passes < 2, max_passes > 2^24, min_passes > max_passes, or a threshold or floor that is not finite
 * or is negative; APT_ERR_STRUCT for a wrong struct_size.  list_count == 0 is APT_OK and nothing is done.
 * Out of scope: bands, ascendpathtracing_amd/dist.py and apt_multi_*; the denoiser on a film whose pixels hold different numbers of
 * passes (its prepare divides by ONE passes); chromatic or tone-aware error measures; tile-granular selection. */
typedef struct apt_film_select {
    uint32_t struct_size;       /* = sizeof(apt_film_select)                                                  */
    uint32_t base_passes;       /* uniform passes in the film and the moments, 2 .. 2^24                      */
    uint32_t min_passes;        /* >= 2: a pixel with fewer passes is always selected                         */
    uint32_t max_passes;        /* min_passes .. 2^24: a pixel that has them is never selected                */
    float threshold;            /* finite, >= 0: relative standard error of the mean luminance that is enough */
    float floor;                /* finite, >= 0: the luminance below which the error is taken absolutely      */
} apt_film_select;
int apt_film_select_default_host(apt_film_select *s, uint32_t base_passes);
uint64_t apt_film_select_work_words(uint64_t pixel_count);
int apt_film_select_device(const apt_film_select *s, void *stream, const float *moments, const uint32_t *extra, uint64_t pixel_count,
                           uint32_t *work, uint32_t *list, uint32_t *count);
int apt_film_select_host(const apt_film_select *s, const float *moments, const uint32_t *extra, uint64_t pixel_count, uint32_t *work,
                         uint32_t *list, uint32_t *count);
int apt_film_accumulate_list_device(void *stream, const float *pass_planes, const uint32_t *list, uint64_t list_count, uint64_t pixel_count,
                                    float *film, float *moments, uint32_t *extra);
int apt_film_accumulate_list_host(const float *pass_planes, const uint32_t *list, uint64_t list_count, uint64_t pixel_count, float *film,
                                  float *moments, uint32_t *extra);
int apt_film_mean_device(void *stream, const float *film, const uint32_t *extra, uint32_t base_passes, uint64_t pixel_count, float *out);
int apt_film_mean_host(const float *film, const uint32_t *extra, uint32_t base_passes, uint64_t pixel_count, float *out);

/* This thread's last refusal by an entry above ("" after a call that returned APT_OK): every entry clears it on entry. */
const char *apt_film_adaptive_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RENDER_MI355X_ADAPTIVE_H */
