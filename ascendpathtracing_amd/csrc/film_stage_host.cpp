// film_stage_host.cpp -- the error record and the range rules of film_stage_host.h.  One object file, linked into each of the six
// film-stage libraries: t_err below exists once per library (and once per thread in it).
#include <stdio.h>

#include <string>

#include "film_stage_host.h"

namespace {
thread_local std::string t_err;

int range_error(const char *what, const char *name, const char *range) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s must lie in %s", what, name, range);
    t_err = buf;
    return APT_ERR_ARG;
}
}

namespace apt {

void stage_clear_error() { t_err.clear(); }

int stage_set_error(int code, const char *fmt, const char *what) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, what);
    t_err = buf;
    return code;
}

const char *stage_last_error() { return t_err.c_str(); }

int stage_pixels_check(uint64_t count, const char *name, const char *what) {
    return count < 1 || count > kMaxPixels ? range_error(what, name, "[1, 2^28]") : APT_OK;
}

int stage_passes_check(uint32_t passes, const char *name, const char *what) {
    return passes < 1 || passes > kMaxPasses ? range_error(what, name, "[1, 2^24]") : APT_OK;
}

} // namespace apt
