// pt_mat_launch.h -- the launch path of the material kernels, shared by the translation units that hold them (materials.hip,
// environment.hip, film.hip, mis.hip, film_list.hip): a call's plain data (apt_materials.h) as the kernels' own argument types (pt_materials.h), and one frame
// and one buffer launcher.  Each translation unit instantiates a launcher with the scene-form bits it pins -- the instantiations its
// code object holds -- and wraps it in a function of its own; materials.hip routes a call to one of them.  Host code only.
#pragma once
#include "apt_materials.h"
#include "pt_dispatch.h"
#include "pt_materials.h"

namespace apt {   // the wrappers of the code objects behind mat_render_frame / mat_render_paths: call.camera and call.env non-null
void env_launch_frame(const MatFrameCall &call);    // environment.hip
void env_launch_paths(const MatPathsCall &call);
void film_launch_frame(const MatFrameCall &call);   // film.hip: call.film is not None
void mis_launch_frame(const MatFrameCall &call);    // mis.hip: call.t.mis, with or without a film
void mis_launch_paths(const MatPathsCall &call);
void film_list_launch_frame(const MatFrameCall &call);   // film_list.hip: call.list is set (a film call), with or without call.t.mis
} // namespace apt

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

// An apt_environment (checked when it was set) as the kMatEnv kernels read it.  film_add: "store or add" of a kMatFilm launch travels
// in bit 1 of the gloss word (kMatEnvFilmAdd): no kernel argument of its own.
MatEnv mat_env(const apt_environment &e, bool gloss, bool film_add) {
    MatEnv m;
    for (int k = 0; k < 3; ++k) { m.horizon[k] = e.horizon[k]; m.zenith[k] = e.zenith[k]; m.sun[k] = e.sun_dir[k]; m.sun_rad[k] = e.sun_radiance[k]; }
    m.omc = e.sun_omc;
    m.sample = ((e.flags & APT_ENV_SAMPLE_SUN) && e.sun_omc > 0.0f) ? 1u : 0u;
    m.gloss = (gloss ? 1u : 0u) | (film_add ? kMatEnvFilmAdd : 0u);
    return m;
}

// PIN: the scene-form bits a translation unit pins (kMatGloss, kMatCamera, kMatEnv, kMatFilm, kMatMis, kMatList).  A pinned bit is set in every kernel
// the launcher names, whatever the call says -- what the call says then travels as data (MatEnv::gloss, the camera record) -- and is
// resolved here, at compile time: with_flag would instantiate the kernels without it as well.
template <int PIN, int BIT, class F> void with_pinned(bool b, F &&f) {
    if constexpr ((PIN & BIT) != 0) f(std::true_type{});
    else with_flag(b, f);
}
// The film tail of a frame launch: a pinned bit, except for the launcher that pins kMatMis WITHOUT kMatFilm (mis.hip's), which holds
// both tails and takes the call's.
template <int PIN, class F> void with_film(bool film, F &&f) {
    if constexpr ((PIN & kMatMis) != 0 && (PIN & kMatFilm) == 0) with_flag(film, f);
    else f(std::integral_constant<bool, (PIN & kMatFilm) != 0>{});
}
template <int PIN> MatEnvArg<PIN> mat_env_arg(const apt_environment *e, bool gloss, bool film_add) {
    if constexpr ((PIN & kMatEnv) != 0) return mat_env(*e, gloss, film_add);
    else return MatNoEnv{};
}
// The camera of a frame call.  Without one, which only a launcher that does not pin kMatCamera takes: the reference's, and a zero
// tail that the kernels do not read.
template <int PIN> CameraEx mat_camera(const apt::MatFrameCall &c) {
    if constexpr ((PIN & kMatCamera) == 0)
        if (!c.camera) { CameraEx cx = {}; camera_init(cx.base, c.width, c.height); return cx; }
    return camera_ex(*c.camera, c.width, c.height);
}

// What every frame launch makes of its call besides the records above.  The caller checked that the plan exists (with a camera, an
// environment or a film: mat_camera_fits) and that there are at most 2^31 - 1 workgroups.
struct MatFrame { FrameArgs fa; FrameShape s; };
MatFrame mat_frame(const apt::MatFrameCall &c, const Camera &cam) {
    MatFrame f;
    f.fa.cam = cam;
    f.fa.width = c.width; f.fa.height = c.height; f.fa.samples = c.samples; f.fa.seed = c.t.seed;
    f.fa.pixel_begin = c.pixel_begin; f.fa.pixel_count = c.pixel_count; f.fa.fb = c.fb; f.fa.fb_u8 = c.fb_u8;
    // a list launch (kMatList kernels): the list's address in the word a film launch never reads
    if (c.list) f.fa.fb_u8 = reinterpret_cast<uint8_t *>(const_cast<uint32_t *>(c.list));
    (void)frame_shape(c.samples, c.pixel_count, f.s);
    return f;
}

template <int PIN> void launch_mat_frame(const apt::MatFrameCall &c) {
    const CameraEx cx = mat_camera<PIN>(c);
    const MatFrame f = mat_frame(c, cx.base);
    const MatKernelArgs ka = mat_trace_args(c.t);
    const MatEnvArg<PIN> ev = mat_env_arg<PIN>(c.env, c.t.gloss, c.film == apt::MatFilm::Add);
    hipStream_t st = (hipStream_t)c.stream;
    with_flag(c.t.ns == 8, [&](auto ns8) { with_flag(c.t.grid != nullptr, [&](auto gr) { with_flag(f.s.group == 8, [&](auto g8) {
        // (kMatMis stands for a light mode: without a table its kernels are the APT_FLAG_NEE ones, which is what the call then carries)
        with_pinned<PIN, kMatMis>(c.t.nee, [&](auto nee) { with_flag(c.t.lights != nullptr, [&](auto lt) {
            with_pinned<PIN, kMatCamera>(c.camera != nullptr, [&](auto cam) { with_pinned<PIN, kMatGloss>(c.t.gloss, [&](auto gl) {
                with_film<PIN>(c.film != apt::MatFilm::None, [&](auto film) {
                    hipLaunchKernelGGL((render_frame_mat_kernel<mat_scene_form(ns8, gr, nee, lt, gl, cam) | (PIN & (kMatEnv | kMatMis | kMatList)) | (film ? kMatFilm : 0), g8 ? 8 : 1>),
                                       dim3((unsigned)f.s.blocks), dim3(kBlock), f.s.lds, st, c.spheres, c.materials, f.fa, ka, f.s.lp, cx.t, ev);
                });
            }); });
        }); });
    }); }); });
}

template <int PIN> void launch_mat_paths(const apt::MatPathsCall &c) {
    const MatKernelArgs ka = mat_trace_args(c.t);
    const MatEnvArg<PIN> ev = mat_env_arg<PIN>(c.env, c.t.gloss, false);
    const uint64_t blocks = (c.c + kBlock - 1) / kBlock;    // <= 2^31 - 1: checked by the caller
    hipStream_t st = (hipStream_t)c.stream;
    with_flag(c.t.ns == 8, [&](auto ns8) { with_flag(c.t.grid != nullptr, [&](auto gr) {
        with_pinned<PIN, kMatMis>(c.t.nee, [&](auto nee) { with_flag(c.t.lights != nullptr, [&](auto lt) { with_pinned<PIN, kMatGloss>(c.t.gloss, [&](auto gl) {
            hipLaunchKernelGGL((render_paths_mat_kernel<mat_scene_form(ns8, gr, nee, lt, gl) | (PIN & (kMatEnv | kMatMis))>), dim3((unsigned)blocks),
                               dim3(kBlock), 0, st, c.rays, c.spheres, c.materials, c.colors, c.n, c.b, c.c, ka, ev);
        }); }); });
    }); });
}

} // namespace
