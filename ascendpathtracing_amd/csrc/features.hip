// features.hip -- the first-hit feature planes (include/render_mi355x.h "features"): coverage, depth, normal and albedo of the first
// surface under each pixel, from the rays a material frame launch traces.  A fifth material code object (`make asm` writes it to
// features.s), so that render_kernels.hip, materials.hip, environment.hip and film.hip are built from what they always held.
// One lane = one pixel: it generates the pixel's 4 * samples camera rays in ascending path order (pt_camera.h, the frame kernels'
// ray-generate), finds each one's first hit with the material kernels' own hit routines (pt_materials.h mat_hit8 / mat_hit_tiles /
// mat_hit_grid, no skip sphere) and adds the eight per-path values to eight float64 sums that stay in registers; the means are
// rounded once to fp32 and stored.  Consecutive lanes own consecutive pixels of the x-major range, so each of the eight plane stores
// of a wave is one contiguous 256-byte run along y.  Every fp32 operation is the one the header names (-ffp-contract=off):
// tests/features_ref.py restates it and the GPU tests compare bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_host.h"
#include "apt_materials.h"
#include "pt_core.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

// The 8-sphere form's LDS table: load_scene8<false>'s geometry [0, 8) and albedo [8, 16) entries.
constexpr int kFeatTab = 16;

// SC: the scene form (kScene8 / kSceneTiles / kSceneGrid), chosen as the material launches choose it.  fa.fb is the feature buffer
// [APT_FEATURE_PLANES][pixel_count]; fa.fb_u8 is not read.  Of ta the kernel reads ns, eps, grid and status.
// No lane returns before the loop ends: the tile form's scan has barriers, and ray-generate votes over the wave (camera_ray_ex).  A
// lane past the range traces the range's first pixel and stores nothing.
template <int SC>
__global__ __launch_bounds__(kBlock) void features_kernel(const float *__restrict__ sph, FrameArgs fa, TraceArgs ta, CameraTail ct) {
    __shared__ float4 tab[SC == kScene8 ? kFeatTab : 1];
    __shared__ float4 tile[SC == kSceneTiles ? kTile : 1];
    __shared__ CameraEx cam;
    GridHeader gh;
    if (!mat_grid_header<SC>(ta, gh)) return;                             // (launch-uniform) not this scene's grid: nothing is written
    park_camera_ex(cam, fa, ct);
    Scene8 sc;
    if (SC == kScene8) (void)load_scene8<false>(sph, sc, tab);            // ends with a barrier
    else __syncthreads();

    const uint64_t pl = (uint64_t)blockIdx.x * kBlock + threadIdx.x;      // < 2^31 * 256: the launch's size was checked
    const bool valid = pl < fa.pixel_count;
    const uint64_t q = fa.pixel_begin + (valid ? pl : 0);
    const uint32_t pi = (uint32_t)(q / fa.height), pj = (uint32_t)(q % fa.height);
    const size_t ns = ta.ns;
    uint32_t n_cells = 0, n_tests = 0;                                    // the grid walk's statistics: not reported here

    double acc[APT_FEATURE_PLANES];
#pragma unroll
    for (int c = 0; c < APT_FEATURE_PLANES; ++c) acc[c] = 0.0;
    uint64_t path = q * 4u * fa.samples;                                  // path index of the pixel's first path
    for (uint32_t sub = 0; sub < 4u; ++sub) {
        for (uint32_t k = 0; k < fa.samples; ++k, ++path) {
            double u1, u2;
            path_uniforms(fa.seed, path, u1, u2);
            float lx = 0.0f, ly = 0.0f;
            if (cam.t.lens) cam_lens_point(fa.seed, path, cam.t.aperture, lx, ly);   // launch-uniform branch
            float rox, roy, roz, rdx, rdy, rdz;
            camera_ray_ex(cam, fa.width, fa.height, pi, pj, sub >> 1, sub & 1u, u1, u2, lx, ly, rox, roy, roz, rdx, rdy, rdz);
            MatPath s;
            mat_path_init(s, rox, roy, roz, rdx, rdy, rdz);
            float t;
            int idx;
            if (SC == kScene8) mat_hit8<false>(sc, s, ta.eps, t, idx);
            else if (SC == kSceneGrid) mat_hit_grid(gh, ta.grid, s, ta.eps, t, idx, n_cells, n_tests);
            else mat_hit_tiles(sph, tile, s, ta.ns, ta.eps, t, idx);
            const bool hit = idx >= 0;
            const size_t g = hit ? (size_t)idx : 0;                       // a miss reads sphere 0's record and uses none of it
            float cx, cy, cz, ar, ag, ab;
            if (SC == kScene8) {
                const float4 geo = tab[g], alb = tab[8 + g];
                cx = geo.x; cy = geo.y; cz = geo.z; ar = alb.x; ag = alb.y; ab = alb.z;
            } else {
                cx = sph[ns + g]; cy = sph[2 * ns + g]; cz = sph[3 * ns + g];
                ar = sph[7 * ns + g]; ag = sph[8 * ns + g]; ab = sph[9 * ns + g];
            }
            float hx = s.dx * t, hy = s.dy * t, hz = s.dz * t;            // the bounce's hit point and normal (mat_shade)
            hx = s.ox + hx; hy = s.oy + hy; hz = s.oz + hz;
            float nx, ny, nz;
            mat_normalise(hx - cx, hy - cy, hz - cz, nx, ny, nz);
            const bool into = mat_dot(s.dx, s.dy, s.dz, nx, ny, nz) < 0.0f;
            const float v[APT_FEATURE_PLANES] = {1.0f, t, into ? nx : -nx, into ? ny : -ny, into ? nz : -nz, ar, ag, ab};
#pragma unroll
            for (int c = 0; c < APT_FEATURE_PLANES; ++c) acc[c] = acc[c] + (double)(hit ? v[c] : 0.0f);
        }
    }
    if (valid) {
        const double count = (double)(4u * fa.samples);
#pragma unroll
        for (int c = 0; c < APT_FEATURE_PLANES; ++c) fa.fb[(uint64_t)c * fa.pixel_count + pl] = (float)(acc[c] / count);
    }
}

} // namespace

namespace apt {

int mat_render_features(const FeaturesCall &c) {
    apt_camera reference;
    reference.struct_size = sizeof reference;
    const apt_camera *camera = c.camera;
    if (!camera) {
        if (int rc = apt_camera_default_host(c.width, c.height, &reference)) return rc;   // (its own error record)
        camera = &reference;
    }
    if (!c.features) return set_error(APT_ERR_ARG, "features must be non-null%s");   // the last refusal: after the camera record's
    const CameraEx cx = camera_ex(*camera, c.width, c.height);
    FrameArgs fa;
    fa.cam = cx.base;
    fa.width = c.width; fa.height = c.height; fa.samples = c.samples; fa.seed = c.seed;
    fa.pixel_begin = c.pixel_begin; fa.pixel_count = c.pixel_count; fa.fb = c.features; fa.fb_u8 = nullptr;
    TraceArgs ta = {};
    ta.ns = c.ns; ta.eps = c.eps; ta.grid = c.grid; ta.status = c.status; ta.seed = c.seed; ta.light = -1;
    const uint64_t blocks = (c.pixel_count + kBlock - 1) / kBlock;        // fewer than a film launch's, which the caller checked
    hipStream_t st = (hipStream_t)c.stream;
    if (c.ns == 8) hipLaunchKernelGGL((features_kernel<kScene8>), dim3((unsigned)blocks), dim3(kBlock), 0, st, c.spheres, fa, ta, cx.t);
    else if (c.grid) hipLaunchKernelGGL((features_kernel<kSceneGrid>), dim3((unsigned)blocks), dim3(kBlock), 0, st, c.spheres, fa, ta, cx.t);
    else hipLaunchKernelGGL((features_kernel<kSceneTiles>), dim3((unsigned)blocks), dim3(kBlock), 0, st, c.spheres, fa, ta, cx.t);
    return APT_OK;
}

} // namespace apt
