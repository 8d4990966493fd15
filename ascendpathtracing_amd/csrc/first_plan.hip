// first_plan.hip -- the kernel that makes the first-bounce plan record of the two-path frame kernel (pt_first_plan.h), a code object
// of its own: render_kernels.hip's holds the render kernels and what its launch matrix lists (tests/test_gpu_launch_matrix.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "apt_host.h"
#include "pt_first_plan.h"

namespace {

// One wave per entry of the record (the entries' bisections are independent), lane 0 of each makes its entry.
__global__ __launch_bounds__(64) void first_plan_kernel(const float *__restrict__ sph, apt::Camera cam, uint32_t width, uint32_t height, float eps,
                                                        uint64_t *__restrict__ rec, uint64_t ticket) {
    if (threadIdx.x != 0 || blockIdx.x >= (uint32_t)apt::kFirstPlanWords) return;
    apt::FirstPlanGeom g;
    apt::first_plan_setup(cam, width, height, sph, eps, g);
    apt::first_plan_premise_origin(g);
    rec[blockIdx.x] = apt::first_plan_pack(apt::first_plan_entry(g, (int)blockIdx.x), ticket);   // one 64-bit store: value and ticket together
}

} // namespace

namespace apt {

// Enqueue only: in front of the frame kernel on its stream, on every call -- the table's contents can change behind an unchanged pointer.
// -> false when the launch failed (the error is cleared: the caller renders without a plan)
bool launch_first_plan(void *stream, const float *spheres_dev, const Camera &cam, uint32_t width, uint32_t height, float eps, uint32_t *status_dev, uint64_t ticket) {
    uint64_t *const rec = reinterpret_cast<uint64_t *>(status_dev + first_plan_slot_word(ticket));
    hipLaunchKernelGGL(first_plan_kernel, dim3(kFirstPlanWords), dim3(64), 0, (hipStream_t)stream, spheres_dev, cam, width, height, eps, rec, ticket);
    return hipGetLastError() == hipSuccess;
}

} // namespace apt
