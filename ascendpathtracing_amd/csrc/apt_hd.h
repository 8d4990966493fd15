// apt_hd.h -- APT_HD: what marks a function that a gfx950 kernel and its CPU twin both run.  Under hipcc it is compiled for both
// sides and always inlined; under a plain C++ compiler (the host translation units, and the sanitizer drivers that build them alone)
// it is an inline function and nothing of HIP is needed.  APT_UNROLL in front of a loop of such a function: the kernel's full unroll
// (a plain C++ compiler does not know the pragma and is left to its own judgement; the result is the same either way).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define APT_HD __host__ __device__ __forceinline__
#define APT_UNROLL _Pragma("unroll")
#else
#define APT_HD inline
#define APT_UNROLL
#endif
