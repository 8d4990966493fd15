// film_stage_host.h -- what the host side of every film-stage library (denoise, adaptive, history, post, metrics, upscale) is built on:
// the per-thread error record behind the library's apt_film_*_last_error(), the limits all of them share and the two range rules with
// their message texts.  film_stage_host.cpp is compiled once and linked into each of the six libraries; with -fvisibility=hidden and
// the version script each library keeps a copy of its own, so a refusal in one leaves the records of the others alone.  Nothing of
// HIP is needed to compile it.
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x.h"

namespace apt {

constexpr uint64_t kMaxPixels = 1ull << 28;   // pixels (or list entries) of one call: 32-bit indices, and at most 2^20 workgroups a launch
constexpr uint32_t kMaxPasses = 1u << 24;     // passes in a film (and frames in a history): the count is exact as a float

void stage_clear_error();                                          // every entry that returns a status calls this first
int stage_set_error(int code, const char *fmt, const char *what);  // returns `code`; fmt holds one %s
const char *stage_last_error();                                    // what the library's apt_film_*_last_error() returns

// The two range rules: APT_OK, or APT_ERR_ARG with "<what>: <name> must lie in [1, 2^28]" / "... [1, 2^24]" in the record.
int stage_pixels_check(uint64_t count, const char *name, const char *what);
int stage_passes_check(uint32_t passes, const char *name, const char *what);

} // namespace apt
