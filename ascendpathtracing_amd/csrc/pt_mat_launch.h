// pt_mat_launch.h -- what the translation units that launch the material kernels share (materials.hip, environment.hip): a call's
// plain data (apt_materials.h) as the kernels' own argument types (pt_materials.h).  Host code only.
#pragma once
#include "apt_materials.h"
#include "pt_materials.h"

namespace {

MatKernelArgs mat_trace_args(const apt::MatTrace &t) {
    MatKernelArgs ka;
    TraceArgs &ta = ka.ta;
    ta.ns = t.ns; ta.depth = t.depth; ta.light = t.light;   // read with APT_FLAG_NEE only
    ta.eps = t.eps; ta.gain = 0.0f; ta.traced = t.traced;
    ta.status = t.status;
    ta.refill_lanes = 0;
    ta.grid = t.grid;
    ta.grid_walk = 0;
    ta.emission = 0;
    ta.rr_start = t.rr_start;
    ta.seed = t.seed;
    ka.lights = t.lights;   // null without a table
    return ka;
}

// The scene form of a launch: the 8-sphere scene ignores a grid, as the mirror entries do.  APT_FLAG_NEE is a bit of it (kMatNee), or a
// light table (kMatLights), which stands for the flag: never both.
// APT_FLAG_GLOSS is another (kMatGloss): without the flag a launch runs the instantiations it ran before the flag existed.
constexpr int mat_scene_form(bool ns8, bool grid, bool nee, bool lights, bool gloss, bool camera = false) {
    return (ns8 ? kScene8 : (grid ? kSceneGrid : kSceneTiles)) | (lights ? kMatLights : (nee ? kMatNee : 0)) | (gloss ? kMatGloss : 0) |
           (camera ? kMatCamera : 0);
}

// An apt_camera (checked by the entry that took it) as the kernels read it.
CameraEx camera_ex(const apt_camera &r, uint32_t width, uint32_t height) {
    CameraEx c;
    for (int k = 0; k < 3; ++k) {
        c.base.pos[k] = r.pos[k]; c.base.g[k] = r.g[k]; c.base.cx[k] = r.cx[k]; c.base.cy[k] = r.cy[k];
        c.t.lens_u[k] = r.lens_u[k]; c.t.lens_v[k] = r.lens_v[k];
    }
    c.base.inv_w = 1.0 / (double)width;   // correctly rounded, as camera_init's
    c.base.inv_h = 1.0 / (double)height;
    c.t.offset = r.offset; c.t.focus = r.focus; c.t.oof = r.offset_over_focus;
    c.t.aperture = (float)r.aperture;
    c.t.lens = r.aperture > 0.0 ? 1u : 0u;   // the rule: from the float64 value, not from its fp32 rounding
    return c;
}

} // namespace
