// metrics_host.h -- what metrics.hip (the device entries) and metrics_host.cpp (the host entries) of libmetrics_mi355x.so share
// beside film_stage_host.h: one check function per entry pair (include/render_mi355x_metrics.h).
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x_metrics.h"
#include "film_stage_host.h"

namespace apt {
struct MxRec;
// What both forms of an entry refuse, in the header's order: APT_OK, and *rec the record as the arithmetic reads it, or the error
// record set.  `work` is checked by the device form alone (need_work).
int film_compare_check(const apt_film_compare *c, const float *a, const float *b, uint64_t pixel_count, const void *work, bool need_work,
                       const void *result, const void *err_map, MxRec *rec, const char *what);
int film_ssim_check(const apt_film_compare *c, const float *a, const float *b, uint32_t width, uint32_t height, const void *work,
                    bool need_work, const void *result, const void *ssim_map, MxRec *rec, const char *what);
}
