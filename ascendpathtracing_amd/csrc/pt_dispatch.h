// pt_dispatch.h -- run-time settings -> template arguments, and the launch shape of a fused frame: shared by the launch code of
// render_kernels.hip and of the material translation units (pt_mat_launch.h).  Host functions only; pt_trace.h is here for the
// constants the kernels and their launches share.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/render_mi355x.h"
#include "pt_core.h"
#include "pt_trace.h"   // kBlock, kMaxStack, kStackSlots; pt_leaf.h

namespace {

// `f` is called with the value as a std::integral_constant, so a launch inside it names its kernel as kernel<m, ...>.  Every
// combination `f` can reach is instantiated: a call site that must not reach one (render_frame_kernel's and render_paths_kernel's
// static_asserts) handles that case before it dispatches.
template <class F> void with_mode(uint32_t mode, F &&f) {
    if (mode == APT_MODE_ORACLE) f(std::integral_constant<int, apt::kModeOracle>{});
    else f(std::integral_constant<int, apt::kModeKernel>{});
}
template <class F> void with_flag(bool b, F &&f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}

// The launch shape of a fused frame kernel (render_frame_kernel, render_frame_mat_kernel) over `pixel_count` pixels: the pairwise-sum
// plan, the lanes per sub-pixel, the workgroups and the dynamic LDS of the plan's stack.
struct FrameShape { LeafProg lp; int group; uint64_t blocks; size_t lds; };   // blocks: the caller refuses more than 2^31 - 1
// -> false: `samples` has no plan (pt_leaf.h)
bool frame_shape(uint32_t samples, uint64_t pixel_count, FrameShape &s) {
    if (!make_leaf_plan(samples, s.lp)) return false;
    s.group = samples >= 8 ? 8 : 1;
    s.blocks = (pixel_count * 4u * (uint64_t)s.group + kBlock - 1) / kBlock;
    s.lds = s.lp.nleaves > 1 ? (size_t)kMaxStack * 3 * kStackSlots * sizeof(float) : 0;
    return true;
}

} // namespace
