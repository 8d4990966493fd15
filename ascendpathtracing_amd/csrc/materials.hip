// materials.hip -- the material kernels' translation unit (pt_materials.h): the kernels a launch without an environment or a film
// runs, and the one place that routes a material launch to its code object (this one, environment.hip's, film.hip's, mis.hip's or
// film_list.hip's).
// render_kernels.hip checks the arguments and calls in through apt_materials.h; keeping these kernels out of its code object leaves
// every kernel that was there before byte for byte as it was (`make asm` writes this code object to materials.s).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/render_mi355x.h"
#include "apt_host.h"
#include "apt_materials.h"
#include "pt_core.h"
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

// This code object pins nothing: 3 scene forms x 3 light modes x 2 groups x camera x gloss frame kernels, 18 buffer kernels.
// The kernels with an environment (environment.hip) and with a film (film.hip) exist as the general-camera, gloss instantiations only,
// and the film's with an environment only.  A frame without a camera set gets apt_camera_default_host's record there, the reference's
// camera bit for bit; a film without an environment the all-zero record, the same image bit for bit; and APT_FLAG_GLOSS travels as
// data (tests/test_gpu_environment.py holds all three against the launches without an environment).  The same holds for the kernels of
// APT_FLAG_MIS (mis.hip; call.t.mis), which hold both tails.  A list call (film_list.hip; call.list, a film call) has kernels of its
// own for both.
int mat_render_frame(const MatFrameCall &call) {
    if (!call.env && call.film == MatFilm::None && !call.t.mis) { launch_mat_frame<0>(call); return APT_OK; }
    MatFrameCall c = call;
    apt_camera reference;
    reference.struct_size = sizeof reference;
    if (!c.camera) {
        if (int rc = apt_camera_default_host(c.width, c.height, &reference)) return rc;   // (its own error record)
        c.camera = &reference;
    }
    apt_environment black = {};
    black.struct_size = sizeof black;
    if (!c.env) c.env = &black;
    if (!c.fb) return set_error(APT_ERR_ARG, "film must be non-null%s");   // a film entry's last refusal: after the camera record's
    if (c.list) film_list_launch_frame(c);
    else if (c.t.mis) mis_launch_frame(c);
    else if (c.film != MatFilm::None) film_launch_frame(c);
    else env_launch_frame(c);
    return APT_OK;
}

void mat_render_paths(const MatPathsCall &call) {
    if (call.t.mis) {
        MatPathsCall c = call;
        apt_environment black = {};
        black.struct_size = sizeof black;
        if (!c.env) c.env = &black;
        mis_launch_paths(c);
    } else if (call.env) env_launch_paths(call);
    else launch_mat_paths<0>(call);
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
