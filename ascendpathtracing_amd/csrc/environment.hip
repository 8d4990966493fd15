// environment.hip -- the material kernels with an environment (pt_materials.h kMatEnv; include/render_mi355x.h "environment") and
// their launches: a translation unit and code object of their own (`make asm` writes it to environment.s), so that materials.hip's --
// every material kernel a launch without an environment runs -- is built from the instantiations it always held.  To keep the build
// in hand these are the general-camera, gloss instantiations only: 3 scene forms x 3 light modes x 2 groups of frame kernels and 9
// buffer kernels.  The default camera record gives the reference camera's rays bit for bit and a table without gloss words the image
// of the kernels without kMatGloss (tests/test_gpu_environment.py holds both against the launches without an environment).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_materials.h"
#include "pt_core.h"
#include "pt_dispatch.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

MatEnv mat_env(const apt_environment &e, bool gloss) {
    MatEnv m;
    for (int k = 0; k < 3; ++k) { m.horizon[k] = e.horizon[k]; m.zenith[k] = e.zenith[k]; m.sun[k] = e.sun_dir[k]; m.sun_rad[k] = e.sun_radiance[k]; }
    m.omc = e.sun_omc;
    m.sample = ((e.flags & APT_ENV_SAMPLE_SUN) && e.sun_omc > 0.0f) ? 1u : 0u;
    m.gloss = gloss ? 1u : 0u;
    return m;
}

constexpr int env_scene_form(bool ns8, bool grid, bool nee, bool lights, bool camera) {
    return mat_scene_form(ns8, grid, nee, lights, true, camera) | kMatEnv;
}

} // namespace

namespace apt {

void env_render_frame(const MatFrameCall &c, const apt_environment &env) {
    FrameArgs fa;
    const CameraEx cx = camera_ex(*c.camera, c.width, c.height);
    fa.cam = cx.base;
    fa.width = c.width; fa.height = c.height; fa.samples = c.samples; fa.seed = c.t.seed;
    fa.pixel_begin = c.pixel_begin; fa.pixel_count = c.pixel_count; fa.fb = c.fb; fa.fb_u8 = c.fb_u8;
    const MatKernelArgs ka = mat_trace_args(c.t);
    const MatEnv ev = mat_env(env, c.t.gloss);
    LeafProg lp;
    (void)make_leaf_plan(c.samples, lp);                   // the caller checked mat_camera_fits
    const int group = c.samples >= 8 ? 8 : 1;
    const uint64_t blocks = (c.pixel_count * 4u * (uint64_t)group + kBlock - 1) / kBlock;   // <= 2^31 - 1: checked by the caller
    const size_t lds = lp.nleaves > 1 ? (size_t)kMaxStack * 3 * kStackSlots * sizeof(float) : 0;
    hipStream_t st = (hipStream_t)c.stream;
    with_flag(c.t.ns == 8, [&](auto ns8) { with_flag(c.t.grid != nullptr, [&](auto gr) { with_flag(group == 8, [&](auto g8) {
        with_flag(c.t.nee, [&](auto nee) { with_flag(c.t.lights != nullptr, [&](auto lt) {
            hipLaunchKernelGGL((render_frame_mat_kernel<env_scene_form(ns8, gr, nee, lt, true), g8 ? 8 : 1>), dim3((unsigned)blocks),
                               dim3(kBlock), lds, st, c.spheres, c.materials, fa, ka, lp, cx.t, ev);
        }); });
    }); }); });
}

void env_render_paths(const MatPathsCall &c, const apt_environment &env) {
    const MatKernelArgs ka = mat_trace_args(c.t);
    const MatEnv ev = mat_env(env, c.t.gloss);
    const uint64_t blocks = (c.c + kBlock - 1) / kBlock;    // <= 2^31 - 1: checked by the caller
    hipStream_t st = (hipStream_t)c.stream;
    with_flag(c.t.ns == 8, [&](auto ns8) { with_flag(c.t.grid != nullptr, [&](auto gr) {
        with_flag(c.t.nee, [&](auto nee) { with_flag(c.t.lights != nullptr, [&](auto lt) {
            hipLaunchKernelGGL((render_paths_mat_kernel<env_scene_form(ns8, gr, nee, lt, false)>), dim3((unsigned)blocks), dim3(kBlock), 0, st,
                               c.rays, c.spheres, c.materials, c.colors, c.n, c.b, c.c, ka, ev);
        }); });
    }); });
}

} // namespace apt
