// selftest_seeded.hip -- apt_selftest_div3_seeded (include/render_mi355x.h): the self-test of the two-path bounce's divide.  A code
// object of its own, like materials.hip: render_kernels.hip's holds the render kernels and the self-tests that came with them, and
// tests/test_gpu_launch_matrix.py keeps a census of it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/render_mi355x.h"
#include "apt_host.h"
#include "pt_core.h"

using namespace apt;

namespace {

constexpr int kSelftestBlock = 256;

// ---- kernel: self-test of the seeded two-path divide (pt_core.h div3_seeded_packed2) ----------------------------------------
// The helper of the two-path bounce against the plain `/`, bit for bit, with the seed the bounce hands it: the device's own
// v_rsq_f32(len2).  A set counts as accepted when div3_operands_ok() holds (the bounce's validity chain) and the helper's flag
// e1 == kDiv3SeededStuck is not raised (the bounce sends such a lane to its exact form).
//   part 0  operand set i of [begin, begin + count) of selftest_div3_kernel's generator (the same sets, set for set); the second
//           half of every pair carries the set with its numerators rotated
//   part 1  i = the bit pattern of len2: every float, d = sqrtf(len2), four numerator triples each (hashed mantissas at the divisor's
//           exponent and up to 13 below it; one triple of powers of two and all-ones mantissas)
//   part 2  ONE divisor, bits in `begin`; i in [0, 3 * 2^23): every numerator mantissa at three exponents (the divisor's, one and
//           twelve below).  Seeds: v_rsq_f32 of every len2 within 2 ulps of RN(d * d) whose sqrtf() is d (the seeds the bounce can hand
//           over for this divisor; the other neighbours become NaN, which div3_operands_ok() rejects), and three synthetic ones,
//           RN(1/d) - 1, + 0, + 1 ulp, with len2 = RN(d * d)
// result: [0] += accepted sets with a wrong quotient, [1] = min(first such i), [2] += accepted, [3] += flagged (operands in range,
// e1 == kDiv3SeededStuck), [4] += flagged although the divisor's mantissa is not all ones, [5] += sets with div3_operands_ok(),
// [6] += sets div3_shared's own flags accept (part 0: [5] + [6] is what selftest_div3_kernel reports as accepted on the same range),
// [7] += accepted sets whose refined reciprocal differs from 1.0f / d.
struct Div3SeededTally { unsigned long long bad = 0, first = ~0ull, accepted = 0, flagged = 0, flagged_other = 0, in_range = 0, shared_ok = 0, recip_off = 0; };
// (tally_y = false: half .y is compared, but only its mismatches are counted -- it is a second look at a set half .x tallies)
__device__ __forceinline__ void div3_seeded_probe(Div3SeededTally &t, uint64_t id, f2 nx, f2 ny, f2 nz, f2 d, f2 len2, f2 r0, bool tally_y = true) {
#if defined(__HIP_DEVICE_COMPILE__)
    f2 ux, uy, uz, e1, e1r;
    div3_seeded_packed2(nx, ny, nz, d, r0, ux, uy, uz, e1);
    const f2 r = refine_seed_packed2(d, r0, e1r);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float n0 = k ? nx.y : nx.x, n1 = k ? ny.y : ny.x, n2 = k ? nz.y : nz.x, dk = k ? d.y : d.x;
        const bool tally = k == 0 || tally_y;
        if (!div3_operands_ok(k ? len2.y : len2.x, n0, n1, n2)) continue;
        if (tally) ++t.in_range;
        if ((k ? e1.y : e1.x) == kDiv3SeededStuck) {
            if (tally) ++t.flagged;
            if (tally && (__float_as_uint(dk) & 0x7fffffu) != 0x7fffffu) ++t.flagged_other;
            continue;
        }
        if (tally) ++t.accepted;
        if (tally && __float_as_uint(k ? r.y : r.x) != __float_as_uint(1.0f / dk)) ++t.recip_off;
        const float w0 = n0 / dk, w1 = n1 / dk, w2 = n2 / dk;
        if (__float_as_uint(k ? ux.y : ux.x) != __float_as_uint(w0) || __float_as_uint(k ? uy.y : uy.x) != __float_as_uint(w1) ||
            __float_as_uint(k ? uz.y : uz.x) != __float_as_uint(w2)) { ++t.bad; if (t.first == ~0ull) t.first = id; }
    }
#endif
}
__global__ __launch_bounds__(kSelftestBlock) void selftest_div3_seeded_kernel(int part, uint64_t begin, uint64_t count,
                                                                      unsigned long long *result) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t stride = (uint64_t)gridDim.x * kSelftestBlock;
    Div3SeededTally t;
    for (uint64_t i = (uint64_t)blockIdx.x * kSelftestBlock + threadIdx.x; i < count; i += stride) {
        if (part == 0) {   // selftest_div3_kernel's generator, statement for statement
            const uint64_t ctr = begin + i;
            uint64_t h = splitmix64(ctr);
            float v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                h = splitmix64(h);
                uint32_t man = (uint32_t)h & 0x7fffffu, ex = 127u - 100u + (uint32_t)((h >> 23) % 134u), sg = (uint32_t)(h >> 63);
                if ((ctr & 3u) == 0u) {
                    const uint32_t pick = (uint32_t)(h >> 40) & 7u;
                    man = pick == 0 ? 0x7fffffu : pick == 1 ? 0u : pick == 2 ? 1u : pick == 3 ? 0x7ffffeu
                        : pick == 4 ? 0x400000u : pick == 5 ? 0x3fffffu : pick == 6 ? 0x400001u : man;
                    if (((h >> 44) & 3u) == 0u) ex = ((h >> 46) & 1u) ? 127u - 96u : 127u + 29u;
                }
                v[k] = __uint_as_float((sg << 31) | (ex << 23) | man);
            }
            if ((ctr & 63u) == 1u) v[(ctr >> 6) % 3u] = (ctr & 64u) ? 0.0f : -0.0f;
            const uint32_t how = (uint32_t)((ctr >> 2) % 3u);
            float len2, d;
            if (how == 0) {
                len2 = 0.0f + v[0] * v[0];
                len2 = len2 + v[1] * v[1];
                len2 = len2 + v[2] * v[2];
                d = sqrtf(len2);
            } else if (how == 1) {
                const float p0 = v[0] * v[0], p1 = v[1] * v[1], p2 = v[2] * v[2];
                double acc = 0.0 + (double)p0;
                acc = acc + (double)p1;
                acc = acc + (double)p2;
                len2 = (float)acc;
                d = sqrtf(len2);
            } else {
                h = splitmix64(h);
                uint32_t man = (uint32_t)h & 0x7fffffu;
                const uint32_t ex = 127u - 50u + (uint32_t)((h >> 23) % 84u);
                if ((ctr & 3u) == 0u) man = ((h >> 40) & 1u) ? 0x7fffffu : 0u;
                d = __uint_as_float((ex << 23) | man);
                len2 = d * d;
            }
            {
                float ux, uy, uz, amin = 1.0f;
                uint32_t hiflag = 0;
                div3_shared(v[0], v[1], v[2], d, len2, ux, uy, uz, amin, hiflag);
                if (!(amin < 0x1p-96f || (int32_t)hiflag < 0)) ++t.shared_ok;
            }
            const float r0 = __builtin_amdgcn_rsqf(len2);
            div3_seeded_probe(t, ctr, f2{v[0], v[1]}, f2{v[1], v[2]}, f2{v[2], v[0]}, f2{d, d}, f2{len2, len2}, f2{r0, r0}, false);
        } else if (part == 1) {
            const uint32_t bits = (uint32_t)(begin + i);
            const float len2 = __uint_as_float(bits), d = sqrtf(len2), r0 = __builtin_amdgcn_rsqf(len2);
            const uint32_t dex = (__float_as_uint(d) >> 23) & 0xffu;
            uint64_t h = splitmix64(bits);
            float v[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                h = splitmix64(h);
                uint32_t man = (uint32_t)h & 0x7fffffu, sg = (uint32_t)(h >> 63);
                uint32_t ex = dex - (k < 3 ? 0u : (uint32_t)((h >> 23) % 14u));
                if (k >= 9) man = ((h >> 40) & 1u) ? 0x7fffffu : 0u;
                if ((int32_t)ex < 1) ex = 1u;   // (far below the chain's 2^-29: such a triple is out of range)
                v[k] = __uint_as_float((sg << 31) | ((ex & 0xffu) << 23) | man);
            }
            div3_seeded_probe(t, bits, f2{v[0], v[3]}, f2{v[1], v[4]}, f2{v[2], v[5]}, f2{d, d}, f2{len2, len2}, f2{r0, r0});
            div3_seeded_probe(t, bits, f2{v[6], v[9]}, f2{v[7], v[10]}, f2{v[8], v[11]}, f2{d, d}, f2{len2, len2}, f2{r0, r0});
        } else {
            const float d = __uint_as_float((uint32_t)begin);
            const uint32_t dex = ((uint32_t)begin >> 23) & 0xffu, man = (uint32_t)i & 0x7fffffu, which = (uint32_t)(i >> 23);
            const uint32_t ex = dex - (which == 0 ? 0u : which == 1 ? 1u : 12u);
            const float n0 = __uint_as_float((ex << 23) | man), n1 = __uint_as_float(0x80000000u | (ex << 23) | (man ^ 0x555555u));
            const float n2 = __uint_as_float((ex << 23) | (0x7fffffu - man));
            const float sq = d * d, rn = 1.0f / d;
            float seeds[8], l2[8];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                l2[k] = __uint_as_float(__float_as_uint(sq) + (uint32_t)(k - 2));
                seeds[k] = __builtin_amdgcn_rsqf(l2[k]);
                if (sqrtf(l2[k]) != d) l2[k] = __uint_as_float(0x7fc00000u);   // not a len2 of this divisor: NaN fails div3_operands_ok(), the probe skips it
            }
#pragma unroll
            for (int k = 5; k < 8; ++k) { l2[k] = sq; seeds[k] = __uint_as_float(__float_as_uint(rn) + (uint32_t)(k - 6)); }
#pragma unroll
            for (int k = 0; k < 8; k += 2)
                div3_seeded_probe(t, i, f2{n0, n0}, f2{n1, n1}, f2{n2, n2}, f2{d, d}, f2{l2[k], l2[k + 1]}, f2{seeds[k], seeds[k + 1]});
        }
    }
    if (t.bad) { atomicAdd(&result[0], t.bad); atomicMin(&result[1], t.first); }
    atomicAdd(&result[2], t.accepted);
    if (t.flagged) atomicAdd(&result[3], t.flagged);
    if (t.flagged_other) atomicAdd(&result[4], t.flagged_other);
    atomicAdd(&result[5], t.in_range);
    atomicAdd(&result[6], t.shared_ok);
    if (t.recip_off) atomicAdd(&result[7], t.recip_off);
#endif
}


} // namespace

int apt_selftest_div3_seeded(void *stream, int part, uint64_t first, uint64_t count, uint64_t *device_result8) {
    apt::clear_error();
    if (!device_result8 || part < 0 || part > 2) return apt::set_error(APT_ERR_ARG, "apt_selftest_div3_seeded: bad arguments%s");
    if (part == 1 && first + count > (1ull << 32)) return apt::set_error(APT_ERR_ARG, "apt_selftest_div3_seeded: range beyond 2^32%s");
    if (part == 2 && (first >> 32 || count > (3ull << 23))) return apt::set_error(APT_ERR_ARG, "apt_selftest_div3_seeded: bad divisor or count%s");
    if (count == 0) return APT_OK;
    hipLaunchKernelGGL(selftest_div3_seeded_kernel, dim3(256 * 16), dim3(kSelftestBlock), 0, (hipStream_t)stream, part, first, count,
                       (unsigned long long *)device_result8);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? APT_OK : apt::set_error(APT_ERR_DEVICE, "HIP: %s", hipGetErrorString(e));
}
