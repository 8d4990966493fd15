// materials.hip -- the material kernels' translation unit (pt_materials.h) and their launches.  render_kernels.hip checks the
// arguments and calls in through apt_materials.h; keeping these kernels out of its code object leaves every kernel that was there
// before byte for byte as it was (`make asm` writes this code object to materials.s).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/render_mi355x.h"
#include "apt_materials.h"
#include "pt_core.h"
#include "pt_dispatch.h"
#include "pt_materials.h"
#include "pt_mat_launch.h"

namespace {

// Self-test of ray-generate's fast direction (pt_core.h fast_direction, dir_probe) with the real v_rsq_f64, against this device's exact
// form -- sqrt() and '/', what a rejected wave redoes.  A test kernel: it lives in this code object, like everything added after the
// mirror renderer's kernels.  res: [0] += rays accepted, [1] += rays rejected, [2] += accepted components that differ, [3] += rays the
// ray-level part rejects, [4] = max over the rays of the bits of |certificate|.
__global__ __launch_bounds__(kBlock) void selftest_direction_kernel(const double *__restrict__ d3, uint64_t count, unsigned long long *res,
                                                                    uint8_t *flags) {
    unsigned long long acc = 0, rej = 0, bad = 0, ray_rej = 0, max_cert = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kBlock) {
        const double d0 = d3[3 * i], d1 = d3[3 * i + 1], d2 = d3[3 * i + 2];
        const double n2 = norm3_sq(d0, d1, d2), n = sqrt(n2);
        double cert;
        const uint32_t f = dir_probe(d0, d1, d2, __builtin_amdgcn_rsq(n2), (float)(d0 / n), (float)(d1 / n), (float)(d2 / n), cert);
        if ((f & 71u) == 71u) ++acc; else ++rej;
        bad += __popc(f & (f >> 3) & 7u);
        ray_rej += (f & 64u) ? 0u : 1u;
        const double ac = fabs(cert);
        if (ac <= 1.7976931348623157e308) max_cert = max(max_cert, (unsigned long long)__double_as_longlong(ac));
        if (flags) flags[i] = (uint8_t)f;
    }
    if (acc) atomicAdd(res, acc);
    if (rej) atomicAdd(res + 1, rej);
    if (bad) atomicAdd(res + 2, bad);
    if (ray_rej) atomicAdd(res + 3, ray_rej);
    if (max_cert) atomicMax(res + 4, max_cert);
}

} // namespace

namespace apt {

void selftest_direction(void *stream, const double *d3, uint64_t count, uint64_t *result5, uint8_t *flags) {
    const uint64_t blocks = std::min<uint64_t>((count + kBlock - 1) / kBlock, 256 * 16);
    hipLaunchKernelGGL(selftest_direction_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, d3, count,
                       (unsigned long long *)result5, flags);
}

void mat_render_frame(const MatFrameCall &c) {
    FrameArgs fa;
    CameraEx cx = {};                                       // without a camera the kernels do not read the tail
    if (c.camera) { cx = camera_ex(*c.camera, c.width, c.height); fa.cam = cx.base; }
    else camera_init(fa.cam, c.width, c.height);
    fa.width = c.width; fa.height = c.height; fa.samples = c.samples; fa.seed = c.t.seed;
    fa.pixel_begin = c.pixel_begin; fa.pixel_count = c.pixel_count; fa.fb = c.fb; fa.fb_u8 = c.fb_u8;
    const MatKernelArgs ka = mat_trace_args(c.t);
    LeafProg lp;
    (void)make_leaf_plan(c.samples, lp);                   // the caller checked that the plan exists (with a camera: mat_camera_fits)
    const int group = c.samples >= 8 ? 8 : 1;
    const uint64_t blocks = (c.pixel_count * 4u * (uint64_t)group + kBlock - 1) / kBlock;   // <= 2^31 - 1: checked by the caller
    const size_t lds = lp.nleaves > 1 ? (size_t)kMaxStack * 3 * kStackSlots * sizeof(float) : 0;
    hipStream_t st = (hipStream_t)c.stream;
    with_flag(c.t.ns == 8, [&](auto ns8) { with_flag(c.t.grid != nullptr, [&](auto gr) { with_flag(group == 8, [&](auto g8) {
        with_flag(c.t.nee, [&](auto nee) { with_flag(c.t.lights != nullptr, [&](auto lt) { with_flag(c.camera != nullptr, [&](auto cam) {
            with_flag(c.t.gloss, [&](auto gl) {
                hipLaunchKernelGGL((render_frame_mat_kernel<mat_scene_form(ns8, gr, nee, lt, gl, cam), g8 ? 8 : 1>), dim3((unsigned)blocks),
                                   dim3(kBlock), lds, st, c.spheres, c.materials, fa, ka, lp, cx.t, MatNoEnv{});
            });
        }); }); });
    }); }); });
}

void mat_render_paths(const MatPathsCall &c) {
    const MatKernelArgs ka = mat_trace_args(c.t);
    const uint64_t blocks = (c.c + kBlock - 1) / kBlock;    // <= 2^31 - 1: checked by the caller
    hipStream_t st = (hipStream_t)c.stream;
    with_flag(c.t.ns == 8, [&](auto ns8) { with_flag(c.t.grid != nullptr, [&](auto gr) {
        with_flag(c.t.nee, [&](auto nee) { with_flag(c.t.lights != nullptr, [&](auto lt) { with_flag(c.t.gloss, [&](auto gl) {
            hipLaunchKernelGGL((render_paths_mat_kernel<mat_scene_form(ns8, gr, nee, lt, gl)>), dim3((unsigned)blocks), dim3(kBlock), 0, st,
                               c.rays, c.spheres, c.materials, c.colors, c.n, c.b, c.c, ka, MatNoEnv{});
        }); }); });
    }); });
}

bool mat_camera_fits(uint32_t samples) {
    LeafProg lp;
    return make_leaf_plan(samples, lp) && lp.nleaves <= kCamMaxLeaves;
}

void mat_gen_rays_camera(const CamRaysCall &c) {
    const CameraEx cam = camera_ex(*c.camera, c.width, c.height);
    const uint64_t blocks = (c.c + kBlock - 1) / kBlock;    // <= 2^31 - 1: checked by the caller
    hipLaunchKernelGGL(gen_rays_camera_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)c.stream, cam, c.width, c.height,
                       c.samples, c.seed, c.n, c.b, c.c, c.rays);
}

} // namespace apt
