// environment.hip -- the material kernels with an environment (pt_materials.h kMatEnv; include/render_mi355x.h "environment") and
// their launches: a translation unit and code object of their own (`make asm` writes it to environment.s), so that materials.hip's --
// every material kernel a launch without an environment runs -- is built from the instantiations it always held.  To keep the build
// in hand these are the general-camera, gloss instantiations only: 3 scene forms x 3 light modes x 2 groups of frame kernels and 9
// buffer kernels.  The default camera record gives the reference camera's rays bit for bit and a table without gloss words the image
// of the kernels without kMatGloss (materials.hip mat_render_frame, which hands both in).  The launch itself: pt_mat_launch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_materials.h"
#include "pt_core.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

constexpr int kPathsPins = kMatEnv | kMatGloss, kFramePins = kPathsPins | kMatCamera;

} // namespace

namespace apt {

void env_launch_frame(const MatFrameCall &c) { launch_mat_frame<kFramePins>(c); }
void env_launch_paths(const MatPathsCall &c) { launch_mat_paths<kPathsPins>(c); }

} // namespace apt
