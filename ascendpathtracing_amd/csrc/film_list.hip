// film_list.hip -- the list passes of the film (APT_FLAG_PIXEL_LIST; pt_materials.h kMatList, pt_frame.h frame_lane_list;
// include/render_mi355x.h "List passes"): the material frame kernels whose lanes take their pixel from a device list, and their launch:
// a seventh material code object (`make asm` writes it to film_list.s), so that render_kernels.hip, materials.hip, environment.hip,
// film.hip, features.hip and mis.hip are built from the instantiations they always held.  As in film.hip these are the
// general-camera, gloss, environment instantiations, and with the film tail only: 3 scene forms x 3 light modes x 2 groups, and the
// kMatMis forms of those with a light mode, 3 x 2 x 2: 30 kernels.  A launch without a camera gets the default record, one without an
// environment the all-zero record (materials.hip mat_render_frame).  The launch itself: pt_mat_launch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_materials.h"
#include "pt_core.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

constexpr int kPins = kMatEnv | kMatGloss | kMatCamera | kMatFilm | kMatList, kMisPins = kPins | kMatMis;

} // namespace

namespace apt {

void film_list_launch_frame(const MatFrameCall &c) {
    if (c.t.mis) launch_mat_frame<kMisPins>(c);
    else launch_mat_frame<kPins>(c);
}

} // namespace apt
