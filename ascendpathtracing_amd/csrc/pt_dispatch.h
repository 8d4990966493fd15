// pt_dispatch.h -- run-time settings -> template arguments, shared by the launch code of render_kernels.hip and materials.hip.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "../../include/render_mi355x.h"
#include "pt_core.h"

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

} // namespace
