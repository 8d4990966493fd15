// history_host.cpp -- the host side of libhistory_mi355x.so (include/render_mi355x_history.h): the checks that the device and the host form of each entry share, the defaults and the CPU twins.  Compiled with the
// product's -ffp-contract=off -fno-fast-math: a twin is a loop over the pixels and the call of history_ops.h that history.hip's
// kernel makes for its lane, so both give the same bits.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "../../include/render_mi355x_history.h"
#include "history_host.h"
#include "history_ops.h"

namespace {
bool finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
bool zero3(const double *v) { return v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0; }
}

namespace apt {
// what the geometry relies on of a camera record; the library does not call apt_camera_check_host
static int camera_check(const apt_camera *c, const char *what) {
    if (c->struct_size != sizeof(apt_camera)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_camera.struct_size mismatch", what);
    if (!finite3(c->pos) || !finite3(c->g) || !finite3(c->cx) || !finite3(c->cy) || !std::isfinite(c->offset))
        return stage_set_error(APT_ERR_ARG, "%s: a camera's pos, g, cx, cy and offset must be finite", what);
    if (zero3(c->g) || zero3(c->cx) || zero3(c->cy)) return stage_set_error(APT_ERR_ARG, "%s: a camera's g, cx and cy must be non-zero", what);
    return APT_OK;
}

int film_history_check(const apt_film_history *rec, const apt_camera *cur_cam, const apt_camera *prev_cam, const float *cur,
                       const float *cur_features, const float *prev_features, const float *prev_hist, uint32_t width, uint32_t height,
                       float *out_hist, HsArgs *args, const char *what) {
    if (!rec || !cur_cam || !cur || !cur_features || !out_hist)
        return stage_set_error(APT_ERR_ARG, "%s: rec/cur_cam/cur/cur_features/out_hist must be non-null", what);
    if (prev_hist && (!prev_features || !prev_cam))
        return stage_set_error(APT_ERR_ARG, "%s: prev_features/prev_cam must be non-null with a prev_hist", what);
    if (rec->struct_size != sizeof(apt_film_history)) return stage_set_error(APT_ERR_STRUCT, "%s: apt_film_history.struct_size mismatch", what);
    if (int rc = stage_pixels_check((uint64_t)width * height, "width * height", what)) return rc;
    if (out_hist == prev_hist) return stage_set_error(APT_ERR_ARG, "%s: out_hist must not be prev_hist", what);
    if (int rc = stage_passes_check(rec->max_history, "max_history", what)) return rc;
    if (!(std::isfinite(rec->tol_plane) && rec->tol_plane >= 0.0f) || !std::isfinite(rec->tol_normal))
        return stage_set_error(APT_ERR_ARG, "%s: tol_plane must be finite and not negative, tol_normal finite", what);
    if (!(rec->min_weight > 0.0f && rec->min_weight <= 1.0f)) return stage_set_error(APT_ERR_ARG, "%s: min_weight must lie in (0, 1]", what);
    if (int rc = camera_check(cur_cam, what)) return rc;
    if (prev_hist)
        if (int rc = camera_check(prev_cam, what)) return rc;
    args->cur = cur; args->cf = cur_features; args->pf = prev_hist ? prev_features : nullptr; args->ph = prev_hist; args->out = out_hist;
    args->w = width; args->h = height;
    args->min_weight = rec->min_weight; args->max_history = (float)rec->max_history;
    args->tol_plane = (double)rec->tol_plane; args->tol_normal = (double)rec->tol_normal;
    args->cc = hs_cam(*cur_cam);
    args->pc = hs_cam(prev_hist ? *prev_cam : *cur_cam);       // (not read on the first frame)
    return APT_OK;
}

int film_history_export_check(const void *hist, uint64_t pixel_count, const void *film, const void *moments, const char *what) {
    if (!hist || !film || !moments) return stage_set_error(APT_ERR_ARG, "%s: hist/film/moments must be non-null", what);
    if (int rc = stage_pixels_check(pixel_count, "pixel_count", what)) return rc;
    return APT_OK;
}
} // namespace apt
using apt::stage_set_error;

extern "C" {

const char *apt_film_history_last_error(void) { return apt::stage_last_error(); }

int apt_film_history_default_host(apt_film_history *rec) {
    apt::stage_clear_error();
    if (!rec) return stage_set_error(APT_ERR_ARG, "%s: the record is null", "apt_film_history_default_host");
    memset(rec, 0, sizeof *rec);
    rec->struct_size = sizeof *rec;
    rec->max_history = 32;
    rec->tol_plane = 0.01f; rec->tol_normal = 0.9f; rec->min_weight = 0.0009765625f;   // DESIGN.md "Temporal accumulation": what the values rest on
    return APT_OK;
}

int apt_film_history_host(const apt_film_history *rec, const apt_camera *cur_cam, const apt_camera *prev_cam, const float *cur,
                          const float *cur_features, const float *prev_features, const float *prev_hist, uint32_t width, uint32_t height,
                          float *out_hist) {
    apt::stage_clear_error();
    apt::HsArgs a;
    const int rc = apt::film_history_check(rec, cur_cam, prev_cam, cur, cur_features, prev_features, prev_hist, width, height, out_hist, &a,
                                           "apt_film_history_host");
    if (rc) return rc;
    for (uint32_t x = 0; x < width; ++x)
        for (uint32_t y = 0; y < height; ++y) apt::hs_pixel(a, x, y);
    return APT_OK;
}

int apt_film_history_export_host(const float *hist, uint64_t pixel_count, float *film, float *moments) {
    apt::stage_clear_error();
    const int rc = apt::film_history_export_check(hist, pixel_count, film, moments, "apt_film_history_export_host");
    if (rc) return rc;
    for (uint64_t i = 0; i < pixel_count; ++i) apt::hs_export(hist, film, moments, pixel_count, i);
    return APT_OK;
}

} // extern "C"
