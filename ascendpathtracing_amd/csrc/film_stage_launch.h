// film_stage_launch.h -- what the device entries of every film-stage library do around a launch: the size of a 1-D grid and the check
// that the runtime took what was launched, reported through the library's error record (film_stage_host.h).  Needs HIP.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "film_stage_host.h"

namespace apt {

// Workgroups of `block` lanes that cover n lanes.  Every n an entry's check lets through is at most kMaxPixels = 2^28 and every block
// at least 256 lanes, so a grid has at most 2^20 workgroups; apt_film_accumulate_device alone takes a larger n, and its own check keeps
// the grid below 2^31.
inline unsigned blocks_for(uint64_t n, uint32_t block) { return (unsigned)((n + block - 1) / block); }

// -> APT_OK when the runtime took the launches since the entry began, APT_ERR_DEVICE with its text in the error record otherwise
inline int launched() {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return APT_OK;
    return stage_set_error(APT_ERR_DEVICE, "%s", hipGetErrorString(e));
}

} // namespace apt
