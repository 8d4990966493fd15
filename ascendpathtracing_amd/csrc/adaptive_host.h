// adaptive_host.h -- what adaptive.hip (the device entries) and adaptive_host.cpp (the host entries) of libadaptive_mi355x.so share
// beside film_stage_host.h: one check function per entry pair (include/render_mi355x_adaptive.h).
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x_adaptive.h"
#include "film_stage_host.h"

namespace apt {
// What both forms of an entry refuse, in the header's order: APT_OK or the error record set.
int film_select_check(const apt_film_select *s, const void *moments, const void *extra, uint64_t pixel_count, const void *work, const void *list,
                      const void *count, const char *what);
int film_accumulate_list_check(const void *pass_planes, const void *list, uint64_t list_count, uint64_t pixel_count, const void *film,
                               const void *moments, const void *extra, const char *what);
int film_mean_check(const void *film, uint32_t base_passes, uint64_t pixel_count, const void *out, const char *what);
}
