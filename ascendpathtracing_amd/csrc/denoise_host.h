// denoise_host.h -- what denoise.hip (the device entries) and denoise_host.cpp (the host entries) of libdenoise_mi355x.so share
// beside film_stage_host.h: one check function per entry pair (include/render_mi355x_denoise.h).
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x_denoise.h"
#include "film_stage_host.h"

namespace apt {
// What both forms of the film accumulate and of the film denoise refuse, in the header's order: APT_OK or the error record set.
int film_accumulate_check(const void *pass_planes, uint64_t pixel_count, const void *film, const void *moments, const char *what);
int film_denoise_check(const apt_film_denoise *d, const void *film, const void *moments, const void *features, uint32_t width, uint32_t height,
                       const void *work, const void *out, const char *what);
}
