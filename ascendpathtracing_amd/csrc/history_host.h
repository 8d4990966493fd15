// history_host.h -- what history.hip (the device entries) and history_host.cpp (the host entries) of libhistory_mi355x.so share
// beside film_stage_host.h: one check function per entry pair (include/render_mi355x_history.h).
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x_history.h"
#include "film_stage_host.h"

namespace apt {
struct HsArgs;
// What both forms of an entry refuse, in the header's order: APT_OK or the error record set.  film_history_check also fills *args
// -- the pointers, the checked record and the cameras as the arithmetic reads them -- when it returns APT_OK.
int film_history_check(const apt_film_history *rec, const apt_camera *cur_cam, const apt_camera *prev_cam, const float *cur,
                       const float *cur_features, const float *prev_features, const float *prev_hist, uint32_t width, uint32_t height,
                       float *out_hist, HsArgs *args, const char *what);
int film_history_export_check(const void *hist, uint64_t pixel_count, const void *film, const void *moments, const char *what);
}
