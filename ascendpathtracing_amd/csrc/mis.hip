// mis.hip -- the material kernels of APT_FLAG_MIS (pt_materials.h kMatMis; include/render_mi355x.h "Multiple importance sampling")
// and their launches: a sixth material code object (`make asm` writes it to mis.s), so that render_kernels.hip, materials.hip,
// environment.hip, film.hip and features.hip are built from the instantiations they always held.  As in environment.hip and film.hip
// these are the general-camera, gloss, environment instantiations only, and only those with a light mode -- the flag is read with
// APT_FLAG_NEE or a light table --: 3 scene forms x 2 light modes x 2 groups of frame kernels, each with the decode tail and with the
// film tail, and 3 x 2 buffer kernels.  A launch without a camera gets the default record, one without an environment the all-zero
// record (materials.hip mat_render_frame / mat_render_paths).  The launch itself: pt_mat_launch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_materials.h"
#include "pt_core.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

constexpr int kPathsPins = kMatEnv | kMatGloss | kMatMis, kFramePins = kPathsPins | kMatCamera;

} // namespace

namespace apt {

void mis_launch_frame(const MatFrameCall &c) { launch_mat_frame<kFramePins>(c); }
void mis_launch_paths(const MatPathsCall &c) { launch_mat_paths<kPathsPins>(c); }

} // namespace apt
