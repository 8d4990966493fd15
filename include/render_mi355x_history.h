/* render_mi355x_history.h -- C-ABI of libhistory_mi355x.so: temporal accumulation for the material renderer's film (render_mi355x.h
 * "film", "features" and "camera"; render_mi355x_denoise.h).  A film is valid for one camera; when the camera moves, the entries here
 * carry radiance, luminance moments and a per-pixel history length from the previous frame to the surface the current pixel sees, and
 * blend the current frame in.  A library and a header of their own, as the denoiser's and the adaptive sampler's: render_mi355x.h,
 * render_mi355x_denoise.h, render_mi355x_adaptive.h and the export lists of the other three libraries are what they were.  The library
 * needs no symbol of the other three.  Status codes are render_mi355x.h's APT_OK / APT_ERR_*; the error text of a refused call is this
 * library's own, per thread: apt_film_history_last_error(). */
#ifndef RENDER_MI355X_HISTORY_H
#define RENDER_MI355X_HISTORY_H

#include <stddef.h>
#include <stdint.h>

#include "render_mi355x.h"   /* APT_OK, APT_ERR_*, APT_FEATURE_*, apt_camera */

#ifdef __cplusplus
extern "C" {
#endif

/* libhistory_mi355x.so is built with -fvisibility=hidden and librender_mi355x.so's export list (csrc/apt_exports.map): what this
 * header declares is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ---- temporal accumulation (EXTENSION) ----------------------------------------------------------------------------------------------
 * Conventions: render_mi355x_denoise.h's.  Every `_device` entry takes DEVICE pointers and is asynchronous on `stream`; its `_host`
 * twin takes HOST pointers, runs the same operations and gives the same bits.  The entries allocate nothing and keep no state.
 *
 * Buffers.  Whole images only: N = width * height pixels, 1 <= N <= 2^28, x-major (pixel (x, y) at x * height + y).
 *   cur            [3][N] float32: the MEAN radiance of the current frame (a film divided by its passes).
 *   cur_features,
 *   prev_features  [APT_FEATURE_PLANES][N] float32, as apt_render_frame_features writes them for the current and the previous camera.
 *   prev_hist,
 *   out_hist       [6][N] float32 history buffers: planes 0..2 the mean radiance, plane 3 the mean luminance, plane 4 the mean squared
 *                  luminance, plane 5 the history length h (>= 1 in every pixel an entry here has written).  out_hist is STORED,
 *                  whatever it held, NaN included, is gone; it never aliases prev_hist.
 *   prev_hist == NULL is the first frame: every pixel is a reset, and prev_features and prev_cam are not read (they may be NULL).
 *
 * Cameras.  cur_cam and prev_cam are apt_camera records (render_mi355x.h "camera"), passed by pointer and read during the call only.
 * The library checks what it relies on and does not call into librender_mi355x.so: struct_size; pos, g, cx, cy and offset finite;
 * g, cx and cy non-zero.  A frame rendered without a context camera is described by apt_camera_default_host's record.  The thin lens
 * is IGNORED: reprojection uses the ray from pos through the pixel centre whatever aperture holds, so the planes of a frame with
 * depth of field -- means over the lens -- reproject approximately.  The projection below inverts the camera when g, cx and cy are
 * mutually orthogonal, which is what apt_camera_default_host and apt_camera_build_host make.
 *
 * Geometry.  All float64, every operation rounded on its own, NO FMA; the divides and the square root are correctly rounded; feature
 * values, the record's tolerances and pixel indices widen exactly.  dot(p, q) = (p0*q0 + p1*q1) + p2*q2;  norm(p) = sqrt(dot(p, p)).
 * w = (double)width, h = (double)height.
 *   The world point of pixel (x, y) of a camera (pos, g, cx, cy, offset) whose planes hold cov, depth and normal there:
 *       a = (x + 0.5) / w - 0.5;   b = (y + 0.5) / h - 0.5
 *       d[k] = (cx[k]*a + cy[k]*b) + g[k]
 *       o[k] = pos[k] + d[k]*offset
 *       t    = depth / cov
 *       X[k] = o[k] + (d[k] / norm(d)) * t
 *       n[k] = normal[k] / cov                                   (the pixel's mean normal)
 *   Current pixel p = (x, y): X, n_p from cur_cam and cur_features;  r = norm(X - pos)  (pos: the current camera's).
 *   Projection of X into the previous camera (pos', g', cx', cy'):
 *       wv[k] = X[k] - pos'[k]
 *       f  = dot(wv, g') / dot(g', g')
 *       a' = dot(wv, cx') / (f * dot(cx', cx'));   b' = dot(wv, cy') / (f * dot(cy', cy'))
 *       u  = (a' + 0.5) * w - 0.5;   v = (b' + 0.5) * h - 0.5
 *       x0 = floor(u);  y0 = floor(v);  fx = u - x0;  fy = v - y0
 *   The four taps, in TAP ORDER ex = 0, 1 (outer), ey = 0, 1 (inner): q = (x0 + ex, y0 + ey), with the bilinear weight of their corner
 *       w_q = (float)((ex ? fx : 1 - fx) * (ey ? fy : 1 - fy))      (one float64 product, rounded once to fp32)
 *   A tap is ACCEPTED iff all of the following hold; every comparison is written so that a NaN fails it:
 *       f > 0
 *       0 <= x0 + ex <= w - 1  and  0 <= y0 + ey <= h - 1           (compared in float64, before any conversion to an integer)
 *       cov_p > 0  and  cov'_q > 0                                  (cov'_q, depth'_q, normal'_q: prev_features at q)
 *       h'_q >= 1                                                   (plane 5 of prev_hist at q)
 *       |dot(X'_q - X, n_p)| <= tol_plane * r                       (X'_q: the tap's own world point in the previous camera)
 *       dot(n_p, n'_q) >= tol_normal                                (n'_q = normal'_q / cov'_q)
 *   W = the fp32 sum of the accepted weights in tap order, starting from 0.  The pixel is VALID iff W >= min_weight.
 *
 * Blend.  From here every step is one IEEE fp32 operation (no FMA; the divides are correctly rounded);
 * lum(r, g, b) = (0.2126f * r + 0.7152f * g) + 0.0722f * b, the denoiser's;  min(a, b) is the select a < b ? a : b.
 *       l = lum(cur_p);  new = (cur_p.r, cur_p.g, cur_p.b, l, l * l)
 *   Reset (the pixel is not valid, or prev_hist is NULL):  out = (new, h = 1).
 *   Valid:
 *       S_j = the sum of w_q * H'_q,j over the accepted taps in tap order, starting from 0 (S = S + w_q * H'_q,j), for each of the five
 *             history values j;  H_j = S_j / W
 *       hl = (the sum of w_q * h'_q, likewise) / W
 *       hn = min(hl + 1, (float)max_history)
 *       alpha = 1 / hn
 *       out_j = H_j + alpha * (new_j - H_j);   out h = hn
 *   With max_history = 1 the result is the current frame (alpha = 1, up to the two roundings of H + (new - H)) with h = 1.  A NaN in an accepted tap's history values or in
 *   cur_p reaches the output pixel; a NaN in a guide (a feature value or a history length) fails a comparison and rejects the tap.
 *
 * Export.  apt_film_history_export_device / _host: the hand-over of a history buffer hist [6][pixel_count] to the UNCHANGED denoiser
 * (render_mi355x_denoise.h) with passes = 2: film [3][pixel_count] and moments [2][pixel_count] are stored.  Per pixel, c the radiance,
 * lm, q, h planes 3, 4, 5, one fp32 operation each:
 *       film_c = c + c;   m0 = lm + lm
 *       hm = h - 1
 *       hm >= 1:    var = max(q - lm * lm, 0) / hm                  (max(a, b) = a > b ? a : b: the variance of the accumulated mean)
 *       otherwise:  var = q                                         (history 1, or a NaN h: a freshly disoccluded pixel counts as
 *                                                                    noisy, not as exact)
 *       q' = lm * lm + var;   m1 = q' + q'
 *   The denoiser's prepare with passes = 2 then recovers the mean exactly (x + x and its half are exact) and, as
 *   max(q' - lm * lm, 0) / 1, the variance var of the accumulated mean up to the rounding of one add and one subtract.
 *
 * apt_film_history_default_host fills the record: max_history = 32, tol_plane = 0.01, tol_normal = 0.9, min_weight = 2^-10.
 * DESIGN.md "Temporal accumulation" records what the values rest on.  APT_ERR_ARG for a NULL record.
 *
 * Refusals, nothing written: APT_ERR_ARG for a NULL pointer (apart from prev_hist, and with it prev_features and prev_cam), a zero
 * width or height, N > 2^28 (pixel_count == 0 or > 2^28 for the export), out_hist == prev_hist, max_history outside 1 .. 2^24, a
 * tolerance or min_weight that is not finite, tol_plane < 0, min_weight outside (0, 1], a camera field of those named above that is
 * not finite, or a zero g, cx or cy; APT_ERR_STRUCT for a wrong struct_size of the record or of a camera.
 *
 * Limits.  The FIRST surface is reprojected: what is seen in a mirror or through glass moves differently from that surface and
 * ghosts.  The scene is assumed static: moving lights or geometry leave stale radiance in the history for about max_history frames.
 * The lens: see "Cameras".
 * Out of scope: bands; ascendpathtracing_amd/dist.py and apt_multi_*; the mirror renderer; motion of spheres; a film with per-pixel
 * pass counts as `cur` beyond the mean of it (render_mi355x_adaptive.h's mean); any change to the denoiser. */
typedef struct apt_film_history {
    uint32_t struct_size;       /* = sizeof(apt_film_history)                                                  */
    uint32_t max_history;       /* 1 .. 2^24: the history length is clamped here (alpha >= 1 / max_history)    */
    uint32_t reserved;          /* not read                                                                    */
    float tol_plane;            /* finite, >= 0: plane distance of a tap, relative to the point's distance     */
    float tol_normal;           /* finite: the least cosine between the mean normals                           */
    float min_weight;           /* finite, in (0, 1]: the least accepted bilinear weight of a valid pixel      */
} apt_film_history;
int apt_film_history_default_host(apt_film_history *rec);
int apt_film_history_device(const apt_film_history *rec, void *stream, const apt_camera *cur_cam, const apt_camera *prev_cam, const float *cur,
                            const float *cur_features, const float *prev_features, const float *prev_hist, uint32_t width, uint32_t height,
                            float *out_hist);
int apt_film_history_host(const apt_film_history *rec, const apt_camera *cur_cam, const apt_camera *prev_cam, const float *cur,
                          const float *cur_features, const float *prev_features, const float *prev_hist, uint32_t width, uint32_t height,
                          float *out_hist);
int apt_film_history_export_device(void *stream, const float *hist, uint64_t pixel_count, float *film, float *moments);
int apt_film_history_export_host(const float *hist, uint64_t pixel_count, float *film, float *moments);

/* This thread's last refusal by an entry above ("" after a call that returned APT_OK): every entry clears it on entry. */
const char *apt_film_history_last_error(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RENDER_MI355X_HISTORY_H */
