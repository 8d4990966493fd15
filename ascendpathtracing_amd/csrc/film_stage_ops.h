// film_stage_ops.h -- the arithmetic that more than one film-stage library runs, each step once: one fp32 operation per line, in one
// order (-ffp-contract=off on both sides), so that every kernel and every CPU twin that calls a step gives the same bits.  The stages'
// own *_ops.h headers call these; nothing of HIP is needed to compile it.
#pragma once
#include <math.h>

#include "apt_hd.h"

namespace apt {

struct alignas(16) FsRec { float x, y, z, w; };   // one record of a stage's work buffer: a 16-byte load or store on the device

// the luminance of include/render_mi355x_denoise.h, which every stage's header refers to
APT_HD float fs_lum(float r, float g, float b) {
    float l = 0.2126f * r;
    l = l + 0.7152f * g;
    return l + 0.0722f * b;
}
APT_HD float fs_max(float a, float b) { return a > b ? a : b; }

// The albedo that demodulates a pixel of coverage `cov`, channel by channel: what the pixel leaves uncovered counts as white, and
// `floor_` keeps the quotient finite.  u = fs_uncovered(cov), computed once for the three channels.
APT_HD float fs_uncovered(float cov) { return 1.0f - cov; }
APT_HD float fs_albedo(float albedo, float u, float floor_) { return fs_max(albedo + u, floor_); }

// ---- the guided edge-stopping weight of a tap q seen from the centre p ---------------------------------------------------------------
struct FsGuide { float nx, ny, nz, z, cov, ar, ag, ab; };   // a pixel's mean normal, depth, coverage and demodulating albedo
struct FsSigma { float n, z, c, a; };                       // the sigmas of the four terms

// The sum x of the normal, depth, coverage and albedo terms; iz = 1 / (p.z + 1e-6), which the caller computes once per centre.  A
// caller with a term of its own (the denoiser's luminance) adds it to the sum before the falloff.
APT_HD float fs_edge_sum(const FsGuide &p, float iz, const FsGuide &q, const FsSigma &s) {
    const float cc = p.cov * q.cov;
    float dt = 0.0f + p.nx * q.nx;
    dt = dt + p.ny * q.ny;
    dt = dt + p.nz * q.nz;
    const float xn = s.n * fs_max(cc - dt, 0.0f);
    const float xz = (s.z * fabsf(p.z - q.z)) * iz;
    const float xc = s.c * fabsf(p.cov - q.cov);
    float da = fabsf(p.ar - q.ar) + fabsf(p.ag - q.ag);
    da = da + fabsf(p.ab - q.ab);
    const float xa = s.a * da;
    float xs = xn + xz;
    xs = xs + xc;
    xs = xs + xa;
    return xs;
}

// The falloff max(1 - x / 8, 0)^8 of a sum x.
APT_HD float fs_edge_falloff(float xs) {
    float t = fs_max(1.0f - xs * 0.125f, 0.0f);
    t = t * t;
    t = t * t;
    return t * t;
}

} // namespace apt
