// post_host.h -- what post.hip (the device entries) and post_host.cpp (the host entries) of libpost_mi355x.so share beside
// film_stage_host.h: one check function per entry pair (include/render_mi355x_post.h).
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x_post.h"
#include "film_stage_host.h"

namespace apt {
struct PoBloom;
// What both forms of an entry refuse, in the header's order: APT_OK or the error record set.  `work` is checked by the device form
// alone (need_work).  film_bloom_check also fills *args -- the pointers, the checked record and the levels' sizes and places in work --
// when it returns APT_OK.
int film_meter_check(const apt_film_meter *m, const void *film, uint64_t pixel_count, const void *work, bool need_work, const void *hist,
                     const char *what);
int film_bloom_check(const apt_film_bloom *b, const float *film, uint32_t width, uint32_t height, float *work, float *out, PoBloom *args,
                     const char *what);
}
