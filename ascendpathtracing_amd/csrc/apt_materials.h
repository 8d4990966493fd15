// apt_materials.h -- what render_kernels.hip (argument checks, C-ABI) hands to materials.hip (the material kernels and their
// launches; include/render_mi355x.h "per-sphere materials").  The material kernels live in a translation unit of their own, so
// that the code object of render_kernels.hip -- every kernel the mirror renderer had before -- is built exactly as before.
// Plain data only: the kernels' own argument types are internal to each translation unit.
#pragma once
#include <stdint.h>

#include "../../include/render_mi355x.h"   // apt_camera

namespace apt {

struct MatTrace {                 // the parts of apt_render_params the material kernels read, after the checks
    uint32_t ns, depth, rr_start; // rr_start: first bounce count of APT_FLAG_RR, 0 = no roulette
    int32_t light;                // APT_FLAG_NEE: the light sphere, 0 <= light < ns (checked by the entry); not read otherwise
    bool nee;                     // APT_FLAG_NEE
    float eps;
    uint64_t seed;
    const uint32_t *grid;         // the uniform grid the caller vouches for (accel with APT_FLAG_GRID_SLOTS): the grid form; null: the
                                  // 8-sphere form (ns == 8) or the tile form.  Never set without a status word to report a broken promise through.
    uint32_t *status;             // the context's device status word, or null
    unsigned long long *traced;   // apt_set_trace_counter block, or null
    const uint32_t *lights;       // the *_lights entries: the light table (device), which then stands for `light` / `nee`; else null.
                                  // Never set without a status word: a table that is not this scene's is reported through it.
    bool gloss;                   // APT_FLAG_GLOSS: the material table may hold APT_MAT_GLOSS words (the gloss instantiations)
};

struct MatFrameCall {             // render_frame with materials: pixels [pixel_begin, pixel_begin + pixel_count), pixel_count > 0
    MatTrace t;
    const float *spheres;
    const uint32_t *materials;
    uint32_t width, height, samples;
    uint64_t pixel_begin, pixel_count;
    float *fb;
    uint8_t *fb_u8;
    void *stream;
    const apt_camera *camera;     // the context's camera (checked when it was set), or null: the reference's
};

struct MatPathsCall {             // render_do_ex with materials: paths [b, b + c) of buffers whose planes hold n paths (already shifted)
    MatTrace t;
    const float *rays, *spheres;
    const uint32_t *materials;
    float *colors;
    uint64_t n, b, c;
    void *stream;
};

struct CamRaysCall {              // apt_gen_rays_camera_device: paths [b, b + c) of a buffer whose planes hold n paths (already shifted)
    const apt_camera *camera;     // checked by the entry
    uint32_t width, height, samples;
    uint64_t seed;
    float *rays;
    uint64_t n, b, c;
    void *stream;
};

// Can a frame of `samples` carry a camera?  The contract's limit (include/render_mi355x.h "camera"): a plan of at most 44 leaves.
bool mat_camera_fits(uint32_t samples);

// Enqueue the launch (hipGetLastError() tells the caller whether it was accepted).
void mat_render_frame(const MatFrameCall &call);
void mat_render_paths(const MatPathsCall &call);
void mat_gen_rays_camera(const CamRaysCall &call);

// The same two launches with the context's environment (include/render_mi355x.h "environment"; checked when it was set): the kMatEnv
// kernels, which live in environment.hip -- a third code object, so that a launch without an environment runs the very kernels it ran
// before there was one.  They are always the general-camera and gloss instantiations: call.camera must be non-null (without a camera
// set the caller hands in apt_camera_default_host's record, the reference's camera bit for bit), and call.t.gloss travels as data.
void env_render_frame(const MatFrameCall &call, const apt_environment &env);
void env_render_paths(const MatPathsCall &call, const apt_environment &env);

// The film launches (include/render_mi355x.h "film"), film.hip: a fourth code object.  film_render_frame is env_render_frame with a film
// tail: call.fb is the film, call.fb_u8 null, `add` false for pass 0 (a store).  Always the kMatEnv kernels: without an environment the
// caller hands in the all-zero record.  film_resolve: the checked arguments of apt_film_resolve_device, pixel_count > 0.
void film_render_frame(const MatFrameCall &call, const apt_environment &env, bool add);
void film_resolve(const apt_film_resolve &r, void *stream, const float *film, uint64_t pixel_count, const float *table_dev, float *out_or_null,
                  uint8_t *u8_or_null);

// apt_selftest_direction's launch (count > 0): the test kernel is kept out of render_kernels.hip's code object as well.
void selftest_direction(void *stream, const double *d3_dev, uint64_t count, uint64_t *result5_dev, uint8_t *flags_dev);

} // namespace apt
