// pt_camera.h -- the movable camera of the material renderer (include/render_mi355x.h "camera"): the device form of an apt_camera and
// ray generation in the general form d = (cx*a + cy*b) + g with an optional thin lens.  camera_ray_t (pt_core.h) stays what the
// reference's one frame needs; this is what every other frame needs.  Shared by materials.hip (the kernels) and host_helpers.cpp
// (the record's checks use the same bounds).  Compiled with -ffp-contract=off: every float64 operation is rounded on its own, the only
// fma calls are norm3_sq's.
#pragma once
#include "pt_core.h"

namespace apt {

// the lens's stream: splitmix64(seed ^ splitmix64(path) ^ salt), next to the bounce's, roulette's, NEE's and the light table's
constexpr uint64_t kLensKeySalt = 0xA54FF53A5F1D36F1ull;

// The magnitude bound of the header: inside it every float64 intermediate of camera_ray_ex_t and every fp32 result is finite
// (|d[k]| <= 2^20 * 0.5 * 2 + 2 < 2^21 with |a|, |b| <= 0.5 + 2^-11; lens: |v[k]| <= 2^21 * 2^30 + 2^30 + 2^22 < 2^52, t = offset / focus
// <= 2^50, |o[k]| < 2^103).  The fast sequences' own validity is tested per ray (camera_ray_ex_t), so a record inside the bound can at
// worst send waves to the exact form.
constexpr double kCamMaxPos = 0x1p30, kCamMaxAxis = 0x1p20, kCamMaxUnit = 2.0, kCamMinFocus = 0x1p-20;
constexpr double kCamMinScale = 0x1p-20, kCamMaxScale = 0x1p20, kCamMinNorm = 0x1p-30, kCamMinSin2 = 0x1p-40;

// What a camera instantiation reads beyond the Camera of FrameArgs: 20 dwords.  The frame kernels get it as an argument of its own
// (FrameArgs is shared with the mirror renderer's kernels and keeps its layout), the ray-buffer generator as part of its CameraEx.
struct CameraTail {
    double offset, focus, oof;      // oof = RN(offset / focus), host-made
    double lens_u[3], lens_v[3];
    float aperture;                 // (float)apt_camera.aperture
    uint32_t lens;                  // aperture > 0, decided on the host from the float64 value
};
static_assert(sizeof(CameraTail) == 80, "CameraTail is 20 dwords");
constexpr uint32_t kCamTailWords = sizeof(CameraTail) / 4;
struct CameraEx {
    Camera base;
    CameraTail t;
};

// Ray-generate for a CameraEx.  lx, ly: the lens point in lens coordinates (fp32; read when c.t.lens).  Same structure as camera_ray_t:
// FAST (device) = RN-reciprocal quotients, sqrt_f64_core and ONE validity test per ray that covers whichever norm and quotients the ray
// has -- the lens replaces d by v = (pos + d*focus) - s, so there is one norm and three quotients either way.
template <bool FAST>
APT_HD bool camera_ray_ex_t(const CameraEx &c, uint32_t w, uint32_t h, uint32_t i, uint32_t j, uint32_t sy, uint32_t sx, double u1,
                            double u2, float lx, float ly, float &rox, float &roy, float &roz, float &rdx, float &rdy, float &rdz) {
    double arg1, arg2;
    const double ddx = tent_t<FAST>(u1, arg1), ddy = tent_t<FAST>(u2, arg2);
    const double xa = ((double)sx + 0.5 + ddx) / 2 + (double)i, xb = ((double)sy + 0.5 + ddy) / 2 + (double)j;
    double a, b;
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST) {
        a = div_by_rn_reciprocal(xa, (double)w, c.base.inv_w) - 0.5;
        b = div_by_rn_reciprocal(xb, (double)h, c.base.inv_h) - 0.5;
    } else
#endif
    {
        a = xa / (double)w - 0.5;
        b = xb / (double)h - 0.5;
    }
    double v0 = (c.base.cx[0] * a + c.base.cy[0] * b) + c.base.g[0];
    double v1 = (c.base.cx[1] * a + c.base.cy[1] * b) + c.base.g[1];
    double v2 = (c.base.cx[2] * a + c.base.cy[2] * b) + c.base.g[2];
    double s0 = c.base.pos[0], s1 = c.base.pos[1], s2 = c.base.pos[2], t = c.t.offset;
    if (c.t.lens) {                                                          // launch-uniform
        const double dlx = (double)lx, dly = (double)ly;
        s0 = c.base.pos[0] + (c.t.lens_u[0] * dlx + c.t.lens_v[0] * dly);
        s1 = c.base.pos[1] + (c.t.lens_u[1] * dlx + c.t.lens_v[1] * dly);
        s2 = c.base.pos[2] + (c.t.lens_u[2] * dlx + c.t.lens_v[2] * dly);
        v0 = (c.base.pos[0] + v0 * c.t.focus) - s0;
        v1 = (c.base.pos[1] + v1 * c.t.focus) - s1;
        v2 = (c.base.pos[2] + v2 * c.t.focus) - s2;
        t = c.t.oof;
    }
    const double n2 = norm3_sq(v0, v1, v2);
    rox = (float)(s0 + v0 * t);
    roy = (float)(s1 + v1 * t);
    roz = (float)(s2 + v2 * t);
#if defined(__HIP_DEVICE_COMPILE__)
    if (FAST) {
        const double n = sqrt_f64_core(n2);
        const double y = refined_reciprocal(n);
        rdx = (float)div_by_rn_reciprocal(v0, n, y);
        rdy = (float)div_by_rn_reciprocal(v1, n, y);
        rdz = (float)div_by_rn_reciprocal(v2, n, y);
        double lo = min3_abs_f64(arg1, arg2, xa);
        lo = min3_abs_f64(lo, xb, v0);
        lo = min3_abs_f64(lo, v1, v2);
        asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(lo), "v"(n2));
        return lo >= 0x1p-60 && n <= 0x1p60;
    }
#endif
    const double n = sqrt(n2);
    rdx = (float)(v0 / n);
    rdy = (float)(v1 / n);
    rdz = (float)(v2 / n);
    return true;
}

APT_HD void camera_ray_ex(const CameraEx &c, uint32_t w, uint32_t h, uint32_t i, uint32_t j, uint32_t sy, uint32_t sx, double u1,
                          double u2, float lx, float ly, float &rox, float &roy, float &roz, float &rdx, float &rdy, float &rdz) {
#if defined(__HIP_DEVICE_COMPILE__)
    const bool ok = camera_ray_ex_t<true>(c, w, h, i, j, sy, sx, u1, u2, lx, ly, rox, roy, roz, rdx, rdy, rdz);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!ok) == 0, 1)) return;
    asm volatile("" ::: "memory"); // keeps the exact form out of the hot path's schedule
#endif
    (void)camera_ray_ex_t<false>(c, w, h, i, j, sy, sx, u1, u2, lx, ly, rox, roy, roz, rdx, rdy, rdz);
}

} // namespace apt
