// upscale_host.h -- what upscale.hip (the device entries) and upscale_host.cpp (the host entries) of libupscale_mi355x.so share
// beside film_stage_host.h: one check function per entry pair (include/render_mi355x_upscale.h).
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x_upscale.h"
#include "film_stage_host.h"

namespace apt {
struct UpArgs;
// What both forms of an entry refuse, in the header's order: APT_OK or the error record set.  film_upscale_check also fills *args
// -- the pointers, the three record arrays of `work` and the checked record -- when it returns APT_OK.
int film_upscale_check(const apt_film_upscale *rec, const float *lo, const float *lo_features, uint32_t lo_width, uint32_t lo_height,
                       const float *hi_features, uint32_t width, uint32_t height, float *work, float *out, uint32_t *resolved, UpArgs *args,
                       const char *what);
int film_upscale_patch_check(const void *sums, const void *list, uint64_t list_count, uint32_t passes, uint64_t pixel_count, const void *out,
                             const char *what);
}
