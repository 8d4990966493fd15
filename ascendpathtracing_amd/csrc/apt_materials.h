// apt_materials.h -- what render_kernels.hip (argument checks, C-ABI) hands to the material kernels' launches (include/render_mi355x.h
// "per-sphere materials").  The material kernels live in translation units of their own (materials.hip, environment.hip, film.hip,
// features.hip, mis.hip, film_list.hip), so
// that the code object of render_kernels.hip -- every kernel the mirror renderer had before -- is built exactly as before.  Which of
// them serves a call is decided behind mat_render_frame / mat_render_paths (materials.hip).
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
    bool mis;                     // APT_FLAG_MIS with `gloss` and a light mode (`nee` or `lights`): GLOSS hits sample the lights too
};

enum class MatFilm { None, Store, Add };   // Store: pass 0; Add: a later pass

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
    const apt_environment *env;   // the context's environment ("environment" in the header; checked when it was set), or null
    MatFilm film;                 // the film entries ("film" in the header): fb is the film and fb_u8 null
    const uint32_t *list = nullptr;   // APT_FLAG_PIXEL_LIST ("List passes" in the header; film entries only, film == Store): the device list
                                  // of pixel_count image pixels, checked by the entry; pixel_begin is 0 and fb the compact scratch
};

struct MatPathsCall {             // render_do_ex with materials: paths [b, b + c) of buffers whose planes hold n paths (already shifted)
    MatTrace t;
    const float *rays, *spheres;
    const uint32_t *materials;
    float *colors;
    uint64_t n, b, c;
    void *stream;
    const apt_environment *env;   // as MatFrameCall's
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

// Enqueue the launch (hipGetLastError() tells the caller whether it was accepted).  mat_render_frame -> APT_OK, or, with the error
// record set and nothing launched, what a call that needs the reference's camera as a record is refused with last: the status of
// apt_camera_default_host for an image shape that has none, then APT_ERR_ARG for a film entry's null fb (the contract's order).
int mat_render_frame(const MatFrameCall &call);
void mat_render_paths(const MatPathsCall &call);
void mat_gen_rays_camera(const CamRaysCall &call);

// film.hip's resolve: the checked arguments of apt_film_resolve_device, pixel_count > 0.
void film_resolve(const apt_film_resolve &r, void *stream, const float *film, uint64_t pixel_count, const float *table_dev, float *out_or_null,
                  uint8_t *u8_or_null);

// features.hip's launch ("features" in the header): the checked arguments of apt_render_frame_features, pixel_count > 0 and no more
// pixels than a film launch takes.  grid and status: as MatTrace's.  -> APT_OK with the launch enqueued, or, with the error record set
// and nothing launched, the entry's last two refusals in the contract's order: the status of apt_camera_default_host for an image
// shape that has no record (camera null), then APT_ERR_ARG for a null `features`.
struct FeaturesCall {
    const float *spheres;
    uint32_t ns;
    float eps;
    uint64_t seed;
    const uint32_t *grid;
    uint32_t *status;
    uint32_t width, height, samples;
    uint64_t pixel_begin, pixel_count;
    float *features;
    void *stream;
    const apt_camera *camera;     // the context's camera, or null: the reference's
};
int mat_render_features(const FeaturesCall &call);

// apt_selftest_direction's launch (count > 0): the test kernel is kept out of render_kernels.hip's code object as well.
void selftest_direction(void *stream, const double *d3_dev, uint64_t count, uint64_t *result5_dev, uint8_t *flags_dev);

} // namespace apt
