/*
 * render_mi355x.h -- C-ABI of librender_mi355x.so, the MI355X (gfx950) drop-in for the
 * hot path of KVM-Explorer/AscendPathTracing (reference paths are relative to the
 * reference repository root):
 *
 *     ray-generate -> ray/sphere intersect -> mirror-reflect / throughput loop -> colour
 *
 * Every entry point below names the reference interface it replaces.  Plain pointers and
 * sizes only; no C++ or torch types.  All device entry points ENQUEUE work on the HIP
 * stream they are given and return without synchronising (the caller synchronises, as
 * src/main.cpp:75 does with aclrtSynchronizeStream); they never allocate, free or retain
 * memory, so they are legal inside a hipGraph capture.  (The exceptions say so: apt_render_host and
 * apt_multi_* are synchronous conveniences that own device buffers.)
 *
 * Thread safety.  apt_last_error() / apt_last_status() are PER THREAD and describe the last call made on
 * that thread: every entry point clears the record on entry and sets it on failure.  The settings the
 * reference keeps as compile-time constants live in an apt_context; its setters and the snapshot a render
 * call takes are serialised inside the context, so concurrent calls on one context are safe and each call
 * sees one consistent set of values; different contexts share nothing.  The context-free forms
 * (render_do, apt_set_default_params, apt_set_trace_counter, apt_set_refill_lanes) act on one process-wide
 * default context with the same guarantees -- two threads that want DIFFERENT render_do parameters use two
 * contexts.
 *
 * Buffers (little-endian IEEE float32):
 *   rays     [6][N]   planes ox,oy,oz,dx,dy,dz              scripts/gen_data.py:65-71
 *   spheres  [10][Ns] planes r^2,x,y,z,emX,emY,emZ,colX,colY,colZ, zero padded to a
 *                     multiple of 512 bytes                  scripts/gen_data.py:106-127
 *   colors   [3][N]   planes r,g,b                           src/render.cpp:218-220
 *   path index p = (((i*H + j)*2 + sy)*2 + sx)*S + k         scripts/gen_data.py:32-36
 *   N = W*H*4*S.
 */
#ifndef RENDER_MI355X_H
#define RENDER_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* librender_mi355x.so is built with -fvisibility=hidden and an export list (csrc/apt_exports.map): what this header declares --
 * and the C++-mangled render_do of src/main.cpp:9-10 -- is all it exports. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define APT_ABI_VERSION 3   /* additive since 3 (round 5): apt_grid_flags, apt_context_get_debug / apt_get_debug, APT_FLAG_GRID_SLOTS, APT_DEV_GRID_MISMATCH */

/* status codes returned by the *_ex / frame entry points (render_do itself is void,
 * like the reference, and reports through apt_last_status() / apt_last_error()). */
enum {
    APT_OK = 0,
    APT_ERR_ARG = 1,       /* null pointer, zero size, size not representable            */
    APT_ERR_STRUCT = 2,    /* struct_size does not match this library                    */
    APT_ERR_SCENE = 3,     /* num_spheres == 0 or light_index out of range               */
    APT_ERR_DEVICE = 4,    /* HIP runtime error (no device, launch failure, ...), or a kernel  */
                           /* reported a failure through the device status word (below)   */
    APT_ERR_IO = 5         /* file contract helpers                                      */
};

/* arithmetic modes */
enum {
    APT_MODE_KERNEL = 0,   /* K-mode: operation order of src/rt_helper.h, all fp32       */
    APT_MODE_ORACLE = 1    /* O-mode: scripts/gen_data.py:246-429 test_soa; the two dot  */
                           /* products of the shading step accumulate in float64 and an  */
                           /* all-miss selects sphere index -1 (Python wrap-around)      */
};

/* flags */
enum {
    APT_FLAG_RETIRE = 1u,  /* retirement of finished paths: a path whose alive bit is     */
                           /* cleared or whose throughput is (0,0,0) stops bouncing.      */
                           /* Colours are bit-identical either way when every albedo      */
                           /* component is finite with a clear sign bit; otherwise 0 *    */
                           /* albedo is -0 or NaN and a RETIRE frame equals the oracle's  */
                           /* RETIRE frame, not the full trace.                           */
    APT_FLAG_BAND_BUFFERS = 8u, /* render_do_ex / apt_gen_rays_device / apt_gen_rays_mt_device_ex: `rays` and  */
                           /* `colors` hold ONLY paths [path_begin, path_begin+path_count): planes of      */
                           /* path_count floats, element (plane k, path p) at [k*path_count + p-path_begin] */
                           /* (default: full [6][N] / [3][N] buffers indexed by the absolute path).  With    */
                           /* it the reference's exact pipeline runs band by band in a bounded buffer.       */
    APT_FLAG_EMISSION = 4u,/* colour = throughput * emission(light sphere) per channel       */
                           /* (spheres.bin planes 4..6) instead of the literal gain 12 of      */
                           /* render.cpp:194-196; identical on the reference scene (em = 12).  */
    APT_FLAG_GRID_SLOTS = 16u, /* render_frame with `accel`: the CALLER states that the grid at `accel` was built for this scene and    */
                           /* carries the pair-slot tables (apt_grid_flags() says so for a built grid).  The frame then takes ONE     */
                           /* launch -- the sample-queue kernel's grid form -- instead of two (without the flag both frame kernels are  */
                           /* launched and the grid's own header decides ON THE DEVICE which one renders; the other returns at once).   */
                           /* A grid that does not keep the promise is not walked: the kernel renders nothing and reports              */
                           /* APT_DEV_GRID_MISMATCH through the device status word.  Same image either way.                            */
    APT_FLAG_NEE = 32u,    /* EXTENSION, *_materials entries only (every other entry ignores the bit): direct light sampling of  */
                           /* the sphere light_index at every diffuse hit, "direct light sampling" below.  Needs light_index >= 0  */
                           /* (APT_ERR_SCENE otherwise).  Unbiased; changes the image by noise only, at any depth.                 */
    APT_FLAG_GLOSS = 64u,  /* EXTENSION, *_materials and *_lights entries only (every other entry ignores the bit): the CALLER states  */
                           /* that the material table may hold APT_MAT_GLOSS words ("GLOSS" below; apt_materials_flags_host() says so */
                           /* for a table).  Without it such a word is a bad code as before and every launch is the one it was.       */
    APT_FLAG_MIS = 128u,   /* EXTENSION: multiple importance sampling of the lights at GLOSS hits ("Multiple importance sampling" below). */
                           /* Read only next to APT_FLAG_GLOSS, by the *_materials entries with APT_FLAG_NEE and by the *_lights entries  */
                           /* (their film entries and buffer mode included); every other launch ignores the bit and is the one it was.    */
                           /* Unbiased; changes the image by noise only, and at depth 1 by nothing.                                      */
    APT_FLAG_PIXEL_LIST = 256u, /* EXTENSION, apt_render_frame_film / apt_context_render_frame_film only (every other entry ignores the bit): */
                           /* the launch renders the pixels of a DEVICE list instead of a range, "List passes" in "film" below.         */
    APT_FLAG_RR = 2u      /* EXTENSION (not in the reference; BASELINE config 5): Russian */
                           /* roulette.  After shading bounce d (0-based) with d+1 >=       */
                           /* rr_start, a path that is alive with q = max(r,g,b) > 0        */
                           /* survives with probability p = clamp(q, 0.05, 0.95): u =       */
                           /* 24-bit uniform from splitmix64(key + (d+1)*0x9E3779B97F4A7C15) */
                           /* >> 40, key = splitmix64(seed ^ splitmix64(path index)); u >= p */
                           /* zeroes the throughput, otherwise it is multiplied by 1/p.      */
                           /* Unbiased; changes the image by noise only.  Same fp32 ops on   */
                           /* GPU and in the CPU restatement (bitwise equal).                */
};

/* Run-time form of the reference's compile-time constants
 * (src/common.h:4-14, src/render.cpp:141,194-196, scripts/gen_data.py:6-10). */
typedef struct apt_render_params {
    uint32_t struct_size;   /* = sizeof(apt_render_params)                               */
    uint32_t width;         /* WIDTH   (common.h:4)                                      */
    uint32_t height;        /* HEIGHT  (common.h:5)                                      */
    uint32_t samples;       /* SAMPLES (common.h:6); samples per pixel = 4*samples       */
    uint32_t depth;         /* bounce count, literal 5 at render.cpp:141                 */
    uint32_t num_spheres;   /* SPHERE_NUM (common.h:10)                                  */
    int32_t  light_index;   /* literal 7 at rt_helper.h:776 / gen_data.py:381            */
    float    eps;           /* EPSILON (common.h:9)                                      */
    float    gain;          /* literal 12 at render.cpp:194-196                          */
    uint32_t mode;          /* APT_MODE_*                                                */
    uint32_t flags;         /* APT_FLAG_*                                                */
    uint32_t rr_start;      /* APT_FLAG_RR: first bounce count at which roulette applies; 0 = 3 */
    uint64_t path_begin;    /* first path index this call renders (multi-GPU shard)      */
    uint64_t path_count;    /* number of paths this call renders; 0 = all N              */
    uint64_t seed;          /* device ray generation only                                */
    uint64_t accel;         /* DEVICE address of a grid built by apt_build_grid_host, or 0 */
} apt_render_params;

/* Fill *p with the reference defaults: 16x16, samples 1, depth 5, 8 spheres, light 7,
 * eps 1e-4, gain 12, K-mode, no flags, whole image. */
void apt_default_params(apt_render_params *p);

/* ---- the reference boundary ---------------------------------------------------------
 * Replaces  void render_do(uint32_t blockDim, void *l2ctrl, void *stream,
 *                          uint8_t *rays, uint8_t *spheres, uint8_t *colors)
 * declared at src/main.cpp:9-10, defined at src/render.cpp:262-266 (body:
 * render<<<blockDim, l2ctrl, stream>>>(rays, spheres, colors)).
 *   blockDim  number of contiguous partitions in the reference (8); the result does not
 *             depend on it here, it is accepted and ignored
 *   l2ctrl    ignored
 *   stream    hipStream_t (0 = the default stream)
 *   rays, spheres, colors   DEVICE pointers, sizes 24*N, 512 and 12*N bytes
 *                           (src/main.cpp:47-49) with the reference's compile-time
 *                           W=H=16, S=1, depth 5; override with apt_set_default_params.
 * Asynchronous; errors are recorded for apt_last_error(). */
void render_do(uint32_t blockDim, void *l2ctrl, void *stream,
               uint8_t *rays, uint8_t *spheres, uint8_t *colors);

/* The same entry under a second name.  The reference declares render_do with C++ linkage
 * (`extern void render_do(...)` without extern "C", src/main.cpp:9-10), so an UNMODIFIED main.o references
 * the mangled symbol _Z9render_dojPvS_PhS0_S0_: the library exports that symbol as well (render_do_cxx.cpp,
 * which forwards here), and a translation unit holding the reference's declaration verbatim links against
 * librender_mi355x.so as it is (tests/test_host_abi.py builds one). */
void apt_render_do(uint32_t blockDim, void *l2ctrl, void *stream,
                   uint8_t *rays, uint8_t *spheres, uint8_t *colors);

/* The parameters render_do() uses (the process-wide default context).  Returns APT_OK or APT_ERR_*. */
int apt_set_default_params(const apt_render_params *p);

/* The CPU-simulator shape of the boundary: src/main.cpp:21-44 calls ICPU_RUN_KF(render, blockDim, rays,
 * spheres, colors) on HOST buffers and the call is synchronous.  This entry takes the same HOST buffers
 * (24*N, 512 (padded table) and 12*N bytes for the default context's parameters), copies them to device 0's
 * current device, renders, copies the colours back and returns when they are there.  Allocates and frees its
 * device buffers; not capture-safe.  Whole frames only, like the reference's call: APT_ERR_ARG when the default
 * parameters carry a strict path sub-range (path_begin != 0, or a path_count that is neither 0 nor N).  Checks the device
 * status word before it returns.  (The arithmetic still runs on the GPU: there is no CPU path.) */
int apt_render_host(uint32_t blockDim, const uint8_t *rays, const uint8_t *spheres, uint8_t *colors);

/* ---- contexts: per-caller settings instead of process-wide ones ---------------------------------
 * A context holds what the reference fixes at compile time (the parameters its render_do renders with) and
 * the diagnostics knobs below.  See "Thread safety" at the top. */
typedef struct apt_context apt_context;
apt_context *apt_context_create(void);                 /* reference defaults; NULL when out of memory */
void apt_context_destroy(apt_context *ctx);
int  apt_context_set_params(apt_context *ctx, const apt_render_params *p);
int  apt_context_set_trace_counter(apt_context *ctx, uint64_t *device_counter);
int  apt_context_set_refill_lanes(apt_context *ctx, uint32_t lanes);

/* Device-side failure channel (the reference asserts INSIDE its kernel: src/render.cpp:68-73 DataFormatCheck / ASSERT).  Every context
 * owns one uint32 status word per device it has launched on; a kernel that has to give up ORs a bit into it (APT_DEV_*), and the frame
 * it wrote is then incomplete.  The word is STICKY: it keeps every failure since the last check.
 *   apt_context_check(ctx, stream)  waits for `stream` (synchronising; not capture-safe), reads the word of the current device and
 *       clears it: APT_OK, or APT_ERR_DEVICE with the bits named in apt_last_error().  apt_check(stream) = the default context.
 *   apt_render_host and apt_multi_render check it themselves before they return.
 * The word is allocated on a context's first launch on a device -- through ANY launching entry point, render_do / render_do_ex /
 * render_frame / apt_render_frame_mt included: the one allocation those otherwise allocation-free calls ever make -- (one hipMalloc of
 * 8256 bytes -- the word, and behind it the records render_frame's two-paths-per-lane kernel reads its first-bounce plan from --, once per context and device, device indices 0..15; a device beyond that runs without a word; skipped while `stream` is being
 * captured -- a context whose FIRST launch on a device happens inside a graph capture runs without the word until a launch or an
 * apt_context_check outside a capture has made it). */
enum {
    APT_DEV_QUEUE_GUARD = 1u,  /* sample-queue kernel (APT_FLAG_RETIRE, 8 spheres): the bound on a wave's loop turns ran out      */
    APT_DEV_GRID_TURNS = 2u,   /* sample-queue kernel, grid form: the bound on a wave's walk turns ran out                         */
    APT_DEV_LDS_BASE = 4u,     /* sample-queue kernels: the dynamic LDS region does not start at LDS address 0 (a build problem)    */
    APT_DEV_GRID_MISMATCH = 8u, /* APT_FLAG_GRID_SLOTS: the grid at `accel` is not this scene's or has no pair-slot tables          */
    APT_DEV_BAD_MATERIAL = 16u, /* *_materials entries: a path hit a sphere whose material code is not an APT_MAT_* value            */
    APT_DEV_LIGHTS_MISMATCH = 32u, /* *_lights entries: the light table is not one for this scene (magic, num_spheres, 1 <= n <= Ns)  */
    APT_DEV_LIST_RANGE = 64u   /* APT_FLAG_PIXEL_LIST: an entry of the pixel list is >= width * height; its slot was left untouched   */
};
int  apt_context_check(apt_context *ctx, void *stream);
int  apt_check(void *stream);

/* Measurement knobs of a context (0 = the library's own choice); tests and profiling scripts select kernels through these, never
 * through the process environment (the APT_* variables of earlier rounds are read once, when a context is created, as initial values):
 *   "queue_ppw" 1..4096 pixels per wave of the sample-queue kernels    "queue_nbuf" 2..16 colour buffers    "queue_lds_pad" bytes
 *   "grid_walk" 1 = frames of a scene behind a grid use render_frame_kernel's nested item walk only (bit-identical, slower)
 *   "grid_spheres_per_cell" cell size of apt_build_grid_host / apt_build_grid_device (default context's value)
 * APT_ERR_ARG for an unknown key or a value out of range.  apt_set_debug = the default context.
 * apt_context_get_debug / apt_get_debug read a knob's current value (so that a caller can restore what it found). */
int  apt_context_set_debug(apt_context *ctx, const char *key, double value);
int  apt_set_debug(const char *key, double value);
int  apt_context_get_debug(apt_context *ctx, const char *key, double *value);
int  apt_get_debug(const char *key, double *value);
void apt_context_render_do(apt_context *ctx, uint32_t blockDim, void *l2ctrl, void *stream,
                           uint8_t *rays, uint8_t *spheres, uint8_t *colors);
int  apt_context_render_do_ex(apt_context *ctx, const apt_render_params *p, void *stream,
                              const float *rays, const float *spheres, float *colors);
int  apt_context_render_frame(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                              uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8);

/* Extended form of the same boundary with run-time parameters.
 * rays/colors are the FULL [6][N] / [3][N] device buffers; the call reads and writes only
 * paths [path_begin, path_begin+path_count). */
int render_do_ex(const apt_render_params *p, void *stream,
                 const float *rays, const float *spheres, float *colors);

/* ---- rays generated on the device, samples accumulated on the device ----------------
 * Fuses gen_rays (scripts/gen_data.py:21-75, camera maths in float64; the two uniforms of path p
 * are outputs 2p+1 and 2p+2 of the SplitMix64 stream seeded with splitmix64(p->seed) -- 52 high
 * bits each -- instead of the host MT19937 stream), the render loop
 * (src/render.cpp:104-207) and decode_color (scripts/data_visualization.py:20-59: mean
 * over S, sum over the 2x2 sub-pixels in float64, /4, clip, *255 truncation).
 *   pixel_begin, pixel_count   range of x-major pixel indices q = i*H + j rendered
 *   fb      device, float32 [3][pixel_count]: clipped pixel value in [0,1], planes r,g,b,
 *           indexed by q - pixel_begin (y NOT flipped; apt_write_ppm flips)
 *   fb_u8   device, uint8 [pixel_count][3] = trunc(clip * 255) from the float64 value,
 *           or NULL
 * p->path_begin/path_count are ignored here. */
int render_frame(const apt_render_params *p, void *stream, const float *spheres,
                 uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8);

/* ---- per-sphere materials (EXTENSION: smallpt's DIFF / SPEC / REFR, scripts/gen_data.py:77-102, and a rough metal, GLOSS) ----------
 * Opt-in: the entries below take a DEVICE uint32_t materials[num_spheres]; every other entry point renders mirrors as before.  Callers
 * detect the feature by its symbols (APT_ABI_VERSION is unchanged).  Arguments are checked before any HIP call: check_params' rules
 * (except that a light_index of -1 is accepted with APT_FLAG_EMISSION, which is not read here), then APT_ERR_ARG for materials == NULL,
 * mode != APT_MODE_KERNEL, accel != 0 without APT_FLAG_GRID_SLOTS, and the pixel / path ranges as render_frame / render_do_ex check
 * them, then APT_ERR_SCENE for APT_FLAG_NEE with light_index < 0.  APT_FLAG_RR applies; APT_FLAG_RETIRE is accepted and changes nothing
 * (paths run to full depth); gain and APT_FLAG_EMISSION are not read, light_index is read with APT_FLAG_NEE only.
 * accel: a grid is taken only on the caller's word that it was built for this scene -- APT_FLAG_GRID_SLOTS, what apt_grid_flags() hands
 * out for a built grid.  Each call is then still ONE launch, which finds every segment's hit by walking the grid.  The grid changes
 * which spheres are tested, never the result: the image is the one specified below, bit for bit.  A grid that does not keep the
 * promise (its header's magic or num_spheres is wrong) is not walked: the kernel writes nothing and ORs APT_DEV_GRID_MISMATCH into the
 * status word.  num_spheres == 8 ignores accel, as the mirror entries do.  When the context has no status word for the device (its
 * first launch there is inside a stream capture), the call renders the same image without the grid.
 *
 * The arithmetic, operation by operation (fp32, every operation rounded on its own: no FMA; sqrt and division are IEEE; a dot
 * product dot(x, y) is the chain ((0 + x0*y0) + x1*y1) + x2*y2):
 *   state   o, d = the camera ray (render_frame) or the ray buffer (render_paths); L = (0,0,0), T = (1,1,1); skip = none.
 *   bounce d = 0 .. depth-1:
 *     hit     the K-mode test of render_do_ex for every sphere but `skip` (t = t0 > eps ? t0 : t1, accepted when t > eps, strict '<'
 *             arg-min, lowest index on ties, kMissT = 1e20 never wins).  No sphere: the path ends (L keeps its value; with an environment set it first gathers the sky
 *             and the sun, "environment" below).
 *     code    m = materials[k] of the hit sphere k; m > 2: the kernel ORs APT_DEV_BAD_MATERIAL into the status word and the path ends.
 *             With APT_FLAG_GLOSS a word APT_MAT_GLOSS_WORD(q) -- low byte 3, q in bits 8..23 with 1 <= q <= 65535, bits 24..31 zero --
 *             is a GLOSS sphere of roughness alpha = q * 2^-16 (exact in fp32); every other word above 2 (q == 0, a set bit 24..31, a
 *             low byte above 3) is bad as before.  Words 0..2 mean what they mean without the flag.
 *     point   h = o + d*t (mul, then add); n = (h - c) / sqrt(dot(h - c, h - c)) (three divisions), as render_do_ex's K-mode.
 *     light   L += T * emission(k) per channel (planes 4..6), then T *= albedo(k) (planes 7..9).
 *     orient  ddn = dot(d, n); into = ddn < 0; nl = into ? n : -n.
 *     draws   mkey = splitmix64(seed ^ splitmix64(path) ^ 0x6A09E667F3BCC909), h = splitmix64(mkey + 0x9E3779B97F4A7C15 * (d + 1))
 *             (uint64 wrap-around), u1 = (float)(h >> 40) * 2^-24, u2 = (float)((h >> 16) & 0xFFFFFF) * 2^-24.  A stream of its own,
 *             separate from APT_FLAG_RR's.  `path` = the path index of the header's layout.
 *     reflect k2 = ddn * 2; d = d - n * k2 per component (render_do_ex's K-mode mirror).
 *     SPEC    reflect.
 *     DIFF    x = u1 * 4 (exact), quadrant q = (int)x, f = x - q (exact), z = f * f;
 *             s = f * (S1 + z*(S3 + z*(S5 + z*(S7 + z*(S9 + z*S11))))), c = 1 + z*(C2 + z*(C4 + z*(C6 + z*(C8 + z*(C10 + z*C12))))),
 *             evaluated innermost first, with the APT_MAT_S* / APT_MAT_C* constants below (fp32 hex literals); then
 *             (sin, cos) of 2*pi*u1 = q 0: (s, c)  1: (c, -s)  2: (-s, -c)  3: (-c, s)  (|error| <= 2^-22 against float64 sin / cos).
 *             r = sqrt(u2); Duff et al. 2017 basis of nl: sg = copysign(1, nl.z), a = -1 / (sg + nl.z), b = (nl.x * nl.y) * a,
 *             t = (1 + ((sg * nl.x) * nl.x) * a, sg * b, -sg * nl.x), bt = (b, sg + (nl.y * nl.y) * a, -nl.y);
 *             v = (t * (cos * r) + bt * (sin * r)) + nl * sqrt(1 - u2) per component; d = v / sqrt(dot(v, v)).
 *     REFR    smallpt's glass, nc = 1, nt = 1.5: dn = into ? ddn : -ddn; nnt = into ? APT_MAT_NNT_IN : 1.5;
 *             cos2t = 1 - (nnt * nnt) * (1 - dn * dn).  cos2t < 0 (total internal reflection): reflect, weight 1.  Otherwise
 *             g = dn * nnt + sqrt(cos2t), g = into ? g : -g; v = d * nnt - n * g per component; tdir = v / sqrt(dot(v, v));
 *             c = 1 - (into ? -ddn : dot(tdir, n)); Re = APT_MAT_R0 + APT_MAT_1MR0 * ((((c * c) * c) * c) * c); Tr = 1 - Re;
 *             P = 0.25 + 0.5 * Re; u1 < P: reflect, weight Re / P; otherwise d = tdir, weight Tr / (1 - P); T *= weight per channel.
 *     GLOSS   (APT_FLAG_GLOSS) a rough conductor: the GGX (Trowbridge-Reitz) distribution of roughness alpha, the separable Smith
 *             shadowing term, reflectance = albedo at every angle (no Fresnel term, as SPEC has none: alpha -> 0 tends to SPEC); the
 *             half vector is drawn from the distribution of visible normals in its spherical-cap form (Dupuy & Benyoub 2023), which
 *             leaves the weight albedo * G1(l) <= 1.  (t, bt) = the Duff basis of nl, as DIFF's.
 *             v = (dot(-d, t), dot(-d, bt), dot(-d, nl))                  the view direction in the frame (negation is exact)
 *             s0 = (alpha * v.x, alpha * v.y, v.z); s = s0 / sqrt(dot(s0, s0))                       (three divisions)
 *             (sin, cos) of 2*pi*u1 by DIFF's polynomial; z = (1 - u2) * (1 + s.z) - s.z; w = 1 - z * z; r = sqrt(w > 0 ? w : 0)
 *             m0 = (alpha * (r * cos + s.x), alpha * (r * sin + s.y), z + s.z); m = m0 / sqrt(dot(m0, m0))
 *             l = m * (2 * dot(v, m)) - v per component (mul, then sub).  !(l.z > 0): the path ends here; L keeps its value (this
 *             hit's emission included), no status bit is set.  Otherwise
 *             a2 = alpha * alpha; g = (2 * l.z) / (l.z + sqrt(a2 + (1 - a2) * (l.z * l.z))); T *= g per channel     (G1(l))
 *             q = (t * l.x + bt * l.y) + nl * l.z per component; d = q / sqrt(dot(q, q)).
 *             For direct light sampling and the light tables below a GLOSS hit is a bounce that does not sample, like SPEC: it draws
 *             no shadow segment, leaves `sampled` false, and whatever the path hits next adds its emission in full -- unless the
 *             launch carries APT_FLAG_MIS ("Multiple importance sampling" below).
 *     skip    o = h.  A branch that leaves on the sphere's OUTER side does not test sphere k on the next segment (skip = k; a convex
 *             sphere cannot be re-hit going outward, while the near root of a wall of radius 1e5 is fp32 noise of ~5e-3 >> eps):
 *             DIFF, SPEC, GLOSS and the REFR reflection leave outward iff `into`, the REFR refraction iff `!into`; otherwise skip = none.
 *     roulette  APT_FLAG_RR as specified above, on T (the path counts as alive until it ends).
 *   colour  L.  render_frame's decode (numpy's pairwise mean, float64 sum of the 4 sub-pixels, clip, x255 truncation) is unchanged.
 *
 * Direct light sampling (APT_FLAG_NEE; next-event estimation, smallpt's "explicit" form).  Without the flag nothing below applies and
 * every image is the one specified above.  With it the light is Lt = sphere light_index: centre c and r2 (planes 1..3, 0), emission e
 * (planes 4..6); one light only.  A path carries a flag `sampled`, false at its start.  The bounce above changes in two places:
 *     light   L += T * emission(k) is left out when `sampled` and k == light_index: that light was counted by the sample of the
 *             previous bounce.  Every other emission is added as before: of other spheres, of the light on the camera ray, after a
 *             SPEC / REFR bounce, and after a DIFF hit that could not sample.  Then sampled = false.
 *     sample  after the DIFF direction is drawn, when d + 1 < depth, k != light_index and h is strictly outside the light:
 *             w0 = c - h per component; d2 = dot(w0, w0); the condition is d2 > r2 (false for NaN).  Then
 *             x = r2 / d2; cmax = sqrt(1 - x); omc = x / (1 + cmax)        (1 - cos_max without the cancellation of 1 - cmax)
 *             nkey = splitmix64(seed ^ splitmix64(path) ^ 0xBB67AE8584CAA73B); (v1, v2) from nkey exactly as (u1, u2) from mkey
 *             (a third stream: h = splitmix64(nkey + 0x9E3779B97F4A7C15 * (d + 1)), the same 24-bit split)
 *             cos_a = 1 - v1 * omc; sin_a = sqrt(1 - cos_a * cos_a); (sin, cos) of 2*pi*v2 by DIFF's polynomial
 *             dl = sqrt(d2); w = w0 / dl (three divisions); (t, bt) = the Duff basis of w, as DIFF's of nl
 *             q = (t * (cos * sin_a) + bt * (sin * sin_a)) + w * cos_a per component; l = q / sqrt(dot(q, q)); cosl = dot(l, nl)
 *             wgt = cosl * (2 * omc)                                        (cos * solid angle / pi; 2 * omc is exact)
 *             sampled = true, whatever follows.
 *     shadow  if cosl > 0: a shadow segment from h along l through the hit test above, every sphere but this bounce's skip sphere
 *             (k if `into`, none otherwise: the DIFF bounce's own).  The light is visible iff the arg-min of that test IS light_index
 *             (no second epsilon, no "anything before the light" test: the shadow ray sees the scene the bounce ray sees, whatever
 *             the test does near t = 0).  Visible: L += (T * e) * wgt per channel, T being the throughput after `T *= albedo` and
 *             before this bounce's roulette.
 *   There is NO sample at the last bounce (d + 1 == depth): a sample at bounce d stands for the emission the plain renderer gathers at
 *   hit d + 1, which a path of `depth` segments does not have.  With this rule a frame with the flag has exactly the expectation of
 *   the same frame without it at the same depth; the flag changes the image by noise only, as APT_FLAG_RR does, and at depth 1 by
 *   nothing.  A traced shadow segment counts as a traced segment in the trace counter (and its cells / candidates in the grid
 *   statistics).  Roulette, APT_DEV_BAD_MATERIAL, the grid rules and APT_FLAG_RETIRE are as above.  d2 > r2 is an fp32 decision for
 *   points near the light's surface: either answer is unbiased because `sampled` follows it.  A light of any material code or albedo
 *   needs no special case. */
enum { APT_MAT_SPEC = 0, APT_MAT_DIFF = 1, APT_MAT_REFR = 2, APT_MAT_GLOSS = 3 };   /* a zero-filled table = all mirrors */
#define APT_MAT_GLOSS_WORD(q) ((uint32_t)APT_MAT_GLOSS | ((uint32_t)(q) << 8))   /* with APT_FLAG_GLOSS: alpha = q * 2^-16, 1 <= q <= 65535 */
#define APT_MAT_S1  0x1.921fb6p+0f
#define APT_MAT_S3  -0x1.4abbcep-1f
#define APT_MAT_S5  0x1.466bc2p-4f
#define APT_MAT_S7  -0x1.32d168p-8f
#define APT_MAT_S9  0x1.501ce2p-13f
#define APT_MAT_S11 -0x1.cd915cp-19f
#define APT_MAT_C2  -0x1.3bd3ccp+0f
#define APT_MAT_C4  0x1.03c1f0p-2f
#define APT_MAT_C6  -0x1.55d3c2p-6f
#define APT_MAT_C8  0x1.e1f2bcp-11f
#define APT_MAT_C10 -0x1.a65e60p-16f
#define APT_MAT_C12 0x1.e3718cp-22f
#define APT_MAT_NNT_IN 0x1.555556p-1f  /* RN(1 / 1.5)                    */
#define APT_MAT_R0     0x1.47ae14p-5f  /* RN(0.04), smallpt's (nt - nc)^2 / (nt + nc)^2 */
#define APT_MAT_1MR0   0x1.eb851ep-1f  /* RN(1 - APT_MAT_R0)                            */

/* render_frame / apt_context_render_frame with materials (the frame entry's pixel range, fb and fb_u8 rules). */
int apt_render_frame_materials(const apt_render_params *p, void *stream, const float *spheres, const uint32_t *materials,
                               uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8);
int apt_context_render_frame_materials(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                                       const uint32_t *materials, uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8);
/* render_do_ex with materials: colors [3][N] = L per path; path_begin / path_count and APT_FLAG_BAND_BUFFERS as render_do_ex. */
int apt_render_paths_materials(const apt_render_params *p, void *stream, const float *rays, const float *spheres,
                               const uint32_t *materials, float *colors);
int apt_context_render_paths_materials(apt_context *ctx, const apt_render_params *p, void *stream, const float *rays,
                                       const float *spheres, const uint32_t *materials, float *colors);
/* ---- several lights: a light table for the material renderer (EXTENSION) -------------------------------------------------------------
 * The *_lights entries are the *_materials entries with one more argument, a DEVICE light table (apt_build_lights_host, uploaded by the
 * caller): at every diffuse bounce ONE light of the table is chosen and sampled directly.  Their argument checks are the *_materials
 * entries' in the same order, except that neither APT_FLAG_NEE nor (beyond check_params' range rule) light_index is read, and right
 * after the materials checks -- before the pixel / path range is looked at -- lights == NULL is APT_ERR_ARG.  accel +
 * APT_FLAG_GRID_SLOTS, APT_FLAG_RR, APT_FLAG_RETIRE, ranges and APT_FLAG_BAND_BUFFERS are as for the *_materials entries.  The kernel
 * checks the table's head once (scalar loads) before it reads anything else: a table whose magic or num_spheres is not this launch's,
 * or whose n is not in [1, num_spheres], is not read further; the kernel writes nothing and ORs APT_DEV_LIGHTS_MISMATCH into the status
 * word.  A call whose context has no status word for the device (its first launch there is inside a stream capture) is refused on the
 * host with APT_ERR_DEVICE instead of being launched: a wrong table means wrong sphere indices, which are not tried out.
 *
 * The table lists n >= 1 DISTINCT spheres g[0..n) with selection probabilities P[i] > 0, sum P = 1, fixed per table.  The estimator,
 * in the terms of "Direct light sampling" above (same fp32 rules).  A path carries `sampled` (false at its start) and `kprev`.
 *   S(j, k, h) = j != k and dot(c_j - h, c_j - h) > r2_j       (w0 = c_j - h per component, d2 = dot(w0, w0), d2 > r2_j; false for NaN)
 *   light   at a hit on sphere m from segment origin o: L += T * emission(m) is left out iff `sampled`, m is listed, and S(m, kprev, o).
 *           (o is the previous bounce's h bit for bit, c_m / r2_m the planes' values: the same decision that bounce took for light m.)
 *           Then sampled = false.
 *   sample  after the DIFF direction is drawn, when d + 1 < depth (a "sampling bounce" on sphere k at h):
 *           lkey = splitmix64(seed ^ splitmix64(path) ^ 0x3C6EF372FE94F82B); u = the first of the two uniforms of
 *           splitmix64(lkey + 0x9E3779B97F4A7C15 * (d + 1)) (its top 24 bits * 2^-24: a fourth stream); i = the first entry with
 *           u < cdf[i]; j = g[i].  If S(j, k, h): the sample and shadow steps of "Direct light sampling" with Lt = sphere j -- the same
 *           nkey stream, (v1, v2) and operations --, except wgt = (cosl * (2 * omc)) * invp[i], the light is visible iff the arg-min
 *           IS j, and visible adds L += (T * e_j) * wgt.  If not S: nothing is added and no segment is traced.
 *           Either way sampled = true and kprev = k.
 *   No sample at the last bounce, as above.  Everything else (camera-ray hits, hits after SPEC / REFR or after a last DIFF bounce,
 *   unlisted emitters) adds emission as the plain renderer does.
 * Unbiased: at a sampling bounce the listed lights split into those with S true, whose direct light the one-sample estimate
 * sum_i P[i] * D_i / P[i] has as its expectation, and those with S false (the sphere we stand on, a light we are inside of), which the
 * next hit gathers as before; both sides decide by the same fp32 predicate on the same values, so no light is counted twice or dropped.
 * With one light g[0] = Lt (cdf = [1], invp = [1]) every rule reduces to APT_FLAG_NEE with light_index = Lt: the same frame, path
 * colours and trace counter bit for bit.  At depth 1 the table changes nothing.
 *
 * The table, words of 4 bytes: head[16] = (magic 0x4C474854 "LGHT", num_spheres, n, total words, bits[0], zeros), uint32 idx[n] = g,
 * float cdf[n], float invp[n], uint32 bits[(num_spheres + 31) / 32] with bit (k & 31) of word k >> 5 set iff sphere k is listed;
 * apt_lights_bytes(num_spheres, n) bytes in all.  Construction (float64 unless said otherwise, every operation on its own, in order):
 *   w[i] = ((e_x + e_y) + e_z) * r2 of sphere g[i] (emitted power up to a constant), replaced by 0 unless 0 < w[i] < inf;
 *   W = ((0 + w[0]) + w[1]) + ...;  f = 0.5 / n;  q[i] = (0.5 * w[i]) / W + f  when 0 < W < inf, else f + f   (half by power, half uniform)
 *   S[i] = ((0 + q[0]) + ...) + q[i];  m[i] = floor(S[i] * 2^24 + 0.5) for i < n - 1, m[n-1] = 2^24;  refused unless 0 < m[0] < m[1] < ...
 *   cdf[i] = m[i] * 2^-24 and P[i] = (m[i] - m[i-1]) * 2^-24 (m[-1] = 0), both exact in fp32: u is a multiple of 2^-24, so P[i] IS the
 *   probability of entry i;  invp[i] = 1 / P[i], one IEEE fp32 division.
 * apt_build_lights_host: spheres = HOST [10][Ns] table; indices = HOST list of num_indices sphere indices (kept in this order), or
 * NULL (num_indices not read) = every sphere with an emission channel > 0, ascending; lights = HOST buffer of `capacity` bytes;
 * *out_bytes (optional) receives the table's size.  apt_lights_bytes(num_spheres, num_spheres) bounds every table of a scene.
 * Nothing is written unless APT_OK.  APT_ERR_ARG: spheres or lights NULL, capacity too small (*out_bytes is set).  APT_ERR_SCENE:
 * num_spheres == 0, an empty list (or no emitter for NULL), an index >= num_spheres, a sphere listed twice, a P[i] below 2^-24. */
size_t apt_lights_bytes(uint32_t num_spheres, uint32_t num_lights);
int apt_build_lights_host(const float *spheres_host, uint32_t num_spheres, const uint32_t *indices, uint32_t num_indices, void *lights,
                          size_t capacity, size_t *out_bytes);
int apt_render_frame_lights(const apt_render_params *p, void *stream, const float *spheres, const uint32_t *materials, const void *lights,
                            uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8);
int apt_context_render_frame_lights(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                                    const uint32_t *materials, const void *lights, uint64_t pixel_begin, uint64_t pixel_count, float *fb,
                                    uint8_t *fb_u8);
int apt_render_paths_lights(const apt_render_params *p, void *stream, const float *rays, const float *spheres, const uint32_t *materials,
                            const void *lights, float *colors);
int apt_context_render_paths_lights(apt_context *ctx, const apt_render_params *p, void *stream, const float *rays, const float *spheres,
                                    const uint32_t *materials, const void *lights, float *colors);

/* ---- Multiple importance sampling of the lights at GLOSS hits (APT_FLAG_MIS; EXTENSION) ---------------------------------------------------
 * Opt-in and additive (APT_ABI_VERSION is unchanged, no entry is added).  The bit is read only in a launch that also carries APT_FLAG_GLOSS
 * and that samples lights: a *_materials entry with APT_FLAG_NEE, or a *_lights entry -- the film entries and buffer mode included,
 * through the same flag word.  Every other launch ignores it and is the launch it was: the mirror entries, the feature planes, a
 * *_materials launch without APT_FLAG_NEE, any launch without APT_FLAG_GLOSS.  A table without a GLOSS word renders the image of the
 * launch without the bit, bit for bit.
 *
 * Without the bit a GLOSS hit reaches a light only when the direction it draws happens to find it: the noisiest thing the renderer
 * draws is the broad highlight of a small lamp.  With it a GLOSS hit samples the light as well, and the two strategies -- the light's
 * cone and the visible-normal sampler -- share every direction by the balance heuristic.  The arithmetic, in the terms of "per-sphere
 * materials", "Direct light sampling" and "several lights" above (fp32, every operation rounded on its own: no FMA; IEEE sqrt and
 * division; dot as the chain above).  PI = 0x1.921fb6p+1f and 2PI = 0x1.921fb6p+2f are RN(pi) and RN(2 pi).  A path carries, next to
 * `sampled` and `kprev`, one more bit `glprev` (false at its start) and one float `pbprev`.  In the frame (t, bt, nl) of a GLOSS hit,
 * with a2 = alpha * alpha:
 *     G1(z)   = (2 * z) / (z + sqrt(a2 + (1 - a2) * (z * z)))                                     (the GLOSS block's own G1, of a z component)
 *     D(m)    = a2 / ((PI * k) * k) with k = (m.x * m.x + m.y * m.y) + a2 * (m.z * m.z)          (GGX of a UNIT half vector: m.x^2 + m.y^2
 *               stands for 1 - m.z^2, so there is no cancellation of (m.z^2)(a2 - 1) + 1; k >= ~a2 > 0 for every q >= 1, and at q = 1,
 *               a2 = 2^-32, D <= ~2^32 / pi stays inside fp32)
 *     pb(m)   = (G1(v.z) * D(m)) / (4 * v.z)                        (the density under which the visible-normal sampler draws l = reflect(v, m))
 *     pl(r2, d2, P) = P / (2PI * omc) with x = r2 / d2, cmax = sqrt(1 - x), omc = x / (1 + cmax)     (the density of the cone sampler)
 *   GLOSS   a GLOSS hit on sphere k at h, bounce d with d + 1 < depth, is a SAMPLING BOUNCE -- whether or not its own direction l is
 *           accepted: a path that ends here (!(l.z > 0)) still takes the light sample below first; tying the light sample to what the
 *           other strategy drew would scale it by that strategy's acceptance rate.  T *= G1(l) takes effect after the shadow step.
 *           glprev = true; pbprev = pb(m) of the drawn m.
 *           choice  as a DIFF hit: with APT_FLAG_NEE the light is j = light_index, P = 1, and the predicate is k != j and d2 > r2
 *                   (then, and only then, sampled = true); with a table i is drawn from the lkey stream, j = g[i], P = cdf[i] - cdf[i-1]
 *                   (cdf[-1] = 0; exact), the predicate is S(j, k, h), and sampled = true, kprev = k either way.
 *           sample  predicate true: "Direct light sampling"'s sample step for sphere j up to l -- the same nkey stream, (v1, v2), omc
 *                   and operations (a bounce has one hit, so a DIFF and a GLOSS hit never draw from the same counter) --, called c here.
 *                   wl = (dot(c, t), dot(c, bt), dot(c, nl)).  !(wl.z > 0): nothing is added and no segment is traced.  Otherwise
 *                   m' = (v + wl) / sqrt(dot(v + wl, v + wl)) (three additions, three divisions); p_b = pb(m'); p_l = pl(r2_j, d2, P);
 *                   sum = p_b + p_l.  !(sum > 0 and sum < inf) -- a vanishing v.z makes p_b NaN or inf, a vanishing omc p_l inf --:
 *                   nothing is added and no segment is traced.  Otherwise wgt = G1(wl.z) * (p_b / sum).
 *           shadow  the DIFF sample's: from h along c, every sphere but this bounce's skip sphere, visible iff the arg-min IS j;
 *                   visible: L += (T * e_j) * wgt per channel, T being the throughput after `T *= albedo` and before G1(l) and
 *                   roulette.  (BRDF * cos / p_l is albedo * G1(wl) * p_b / p_l; the balance heuristic multiplies it by p_l / sum.)
 *   light   at the next hit, on sphere m from origin o: where the rules above LEAVE OUT emission(m) -- `sampled` and m == light_index,
 *           or, with a table, `sampled`, m listed and S(m, kprev, o) -- and glprev is set, it is weighted instead:
 *           p_l' = pl(r2_m, dot(c_m - o, c_m - o), P_m) with P_m = 1 or the P of the entry that lists m: that light's own density
 *           from o, the sampling bounce's operations on the sampling bounce's values, bit for bit;  sum = pbprev + p_l';
 *           w = (sum > 0 and sum < inf) ? pbprev / sum : 1;  L += (T * emission(m)) * w per channel.  Then glprev = false.
 *           Everything else is unchanged: emission after a DIFF sample is left out, after SPEC, REFR, an unsampled bounce or of an
 *           unlisted emitter added in full; the camera ray, roulette, the APT_DEV_* bits, the grid rules and the trace counter are
 *           as above, and a traced shadow segment counts.
 *   sun     the sun sample of "environment" stays a DIFF-only matter: a miss after a GLOSS hit adds the sun in full, as without the bit.
 * Finite: with finite inputs D, G1 and both densities are finite or are caught by the `sum` test, whose failure gives the light sample
 * nothing and the next hit the emission in full -- both sides take the same decision only approximately (p_b is evaluated at m' on one
 * side and at the drawn m on the other), which is the balance heuristic's own fp32 rounding and no bias beyond it.
 * Properties: a frame with the bit has the expectation of the same frame without it at the same depth (the image changes by noise
 * only) and is the same frame bit for bit at depth 1; a one-light table equals APT_FLAG_NEE with that light bit for bit, trace counter
 * included; a table with the bit but no GLOSS word renders the flagless image bit for bit.  A table that is not the scene's is reported
 * with APT_DEV_LIGHTS_MISMATCH and nothing is written, as without the bit. */

/* HOST demo scene: gen_spheres' 8 spheres plus smallpt's glass ball (r 16.5 at (73, 16.5, 78), albedo 0.999) as sphere 8, light 7.
 * spheres = HOST float[128] ([10][9] planes, zero padded like gen_spheres), materials = HOST uint32_t[9]: walls and light DIFF,
 * mirror SPEC, glass REFR. */
int apt_gen_spheres_materials_host(float *spheres, uint32_t *materials);
/* HOST material codes for apt_gen_scene_host's scene of the same num_spheres and seed, materials = HOST uint32_t[num_spheres]: spheres
 * 0..5 (walls) and num_spheres-1 (light) APT_MAT_DIFF, sphere i in between (splitmix64(seed + i) >> 32) % 3 with the library's
 * SplitMix64 (x += 0x9E3779B97F4A7C15; x = (x ^ x>>30) * 0xBF58476D1CE4E5B9; x = (x ^ x>>27) * 0x94D049BB133111EB; x ^ x>>31) and
 * uint64 wrap-around.  num_spheres < 8: APT_ERR_SCENE, like apt_gen_scene_host; materials == NULL: APT_ERR_ARG. */
int apt_gen_scene_materials_host(uint32_t num_spheres, uint64_t seed, uint32_t *materials);
/* HOST: the flags a material table earns, the counterpart of apt_grid_flags: APT_FLAG_GLOSS when some materials_host[k], k < num_spheres,
 * is a well-formed APT_MAT_GLOSS_WORD (low byte 3, 1 <= q <= 65535, bits 24..31 zero), else 0 (also for NULL or an empty table).  OR the
 * result into apt_render_params.flags.  A table without such a word renders the same image with and without the flag. */
uint32_t apt_materials_flags_host(const uint32_t *materials_host, uint32_t num_spheres);

/* ---- camera (EXTENSION: a movable camera with a thin lens for the material renderer) -------------------------------------------------
 * The reference has one camera, written into gen_rays (scripts/gen_data.py:24-30): pos (50, 52, 295.6), dir (0, -0.042612, -1), the
 * factor 0.5135, and ray segments that start 140 units of forward depth along the ray.  An apt_camera holds that frame as data.  A
 * context carries at most one (apt_context_set_camera; none = the reference's camera, every entry, kernel and image as before).
 * With a camera set
 *   - the four material FRAME entries (apt_render_frame_materials, apt_render_frame_lights, their apt_context_* forms) render from it;
 *   - the mirror frame entries -- render_frame / apt_context_render_frame, apt_render_frame_mt, apt_multi_render (default context) --
 *     return APT_ERR_ARG after their own checks: they have exactly the reference's camera, and a frame silently taken from another
 *     viewpoint is worse than a refusal.  apt_gen_rays_camera_device + render_do_ex + apt_decode_color_device gives them any camera;
 *   - buffer-mode entries take rays and are unaffected;
 *   - a material frame whose sample count has a pairwise-sum plan of more than 44 leaves (4200 samples is the first; every count
 *     <= 4199 fits) is refused with APT_ERR_ARG: the record's tail travels in the plan's spare words.
 *
 * Ray generation, all float64, every operation rounded on its own (no FMA except where written), then ONE rounding to fp32.  a, b (the
 * tent-filtered image-plane coordinates in [-0.5, 0.5]), the path layout and the two SplitMix64 uniforms are render_frame's.
 *   d[k] = (cx[k]*a + cy[k]*b) + g[k]                                                  k = 0, 1, 2
 *   norm(v) = sqrt(fma(v2, v2, fma(v1, v1, v0*v0)))                                    np.linalg.norm's ddot
 *   pinhole (aperture == 0; decided by this rule, never by arithmetic on aperture, whatever `focus` holds):
 *     s[k] = pos[k];  v[k] = d[k];  t = offset
 *   thin lens (aperture > 0):
 *     lkey = splitmix64(seed ^ splitmix64(path) ^ 0xA54FF53A5F1D36F1); h = splitmix64(lkey + 0x9E3779B97F4A7C15);
 *     v1 = (float)(h >> 40) * 2^-24, v2 = (float)((h >> 16) & 0xFFFFFF) * 2^-24      (a stream of its own, the material streams' split)
 *     r = sqrtf(v1); (sin, cos) of 2*pi*v2 by DIFF's polynomial; lx = (cos*r)*(float)aperture, ly = (sin*r)*(float)aperture (fp32; both
 *     widen exactly)
 *     s[k] = pos[k] + (lens_u[k]*lx + lens_v[k]*ly)                                   the point on the lens
 *     v[k] = (pos[k] + d[k]*focus) - s[k]                                             towards the point in focus (d's forward part is 1)
 *     t = offset_over_focus                                                            RN(offset / focus), made on the host
 *   o[k] = (float)(s[k] + v[k]*t);  dir[k] = (float)(v[k] / norm(v))
 * With apt_camera_default_host's record this is render_frame's ray bit for bit (the terms it drops for the reference frame are exact
 * identities).  The device evaluates the quotients and the square roots with faster sequences that give the same bits while nothing
 * is scaled; one test per ray (the tent arguments, |xa|, |xb|, |v[k]| and norm^2 >= 2^-60, norm <= 2^60) sends the whole wave to IEEE
 * sqrt and division otherwise.  Magnitude bound (the helpers below refuse records outside it, which keeps every float64 intermediate
 * and every fp32 result finite): |pos[k]|, offset, focus <= 2^30; |cx[k]|, |cy[k]|, aperture <= 2^20; |g[k]|, |lens_u[k]|,
 * |lens_v[k]| <= 2; focus >= 2^-20 when aperture > 0.  Then |v[k]| < 2^53 and |o[k]| < 2^104. */
typedef struct apt_camera {
    uint32_t struct_size;       /* = sizeof(apt_camera)                                                     */
    uint32_t reserved;          /* 0                                                                        */
    double pos[3];              /* eye                                                                      */
    double g[3];                /* unit view direction                                                      */
    double cx[3], cy[3];        /* image-plane axes: full image width / height at forward depth 1           */
    double offset;              /* the segment starts this far along the ray, in units of forward depth (reference: 140, through the front wall) */
    double aperture;            /* lens radius; 0 = pinhole                                                 */
    double focus;               /* forward depth of the plane in focus (read when aperture > 0)              */
    double lens_u[3], lens_v[3];/* unit lens axes (right, up)                                               */
    double offset_over_focus;   /* RN(offset / focus) when aperture > 0, else not read                      */
} apt_camera;

/* Host helpers: no GPU, nothing written unless APT_OK.
 * apt_camera_default_host: the reference's frame for a width x height image, bit for bit gen_rays' (cx = (width*0.5135/height, 0, 0),
 *   cy = cross(cx, g) / norm * 0.5135), offset 140, aperture 0, focus 0, lens_u = (1, 0, 0), lens_v = cross(cx, g) / norm.
 * apt_camera_build_host: a look-along camera.  `scale` is what 0.5135 is to the reference: the full image height at forward depth 1
 *   (2 * tan(vfov / 2) for a vertical field of view; no angle is taken here, so that the result does not depend on a libm).  float64,
 *   one operation at a time, cross(p, q) = (p1*q2 - p2*q1, p2*q0 - p0*q2, p0*q1 - p1*q0):
 *     g = dir / norm(dir);  c = cross(g, up);  right = c / norm(c);  cx = right * ((width * scale) / height);
 *     e = cross(cx, g);  lens_v = e / norm(e);  cy = lens_v * scale;  lens_u = right;  pos = eye;
 *     offset_over_focus = aperture > 0 ? offset / focus : 0.
 *   APT_ERR_ARG: a NULL pointer, width or height 0, a non-finite input, |eye[k]|, |dir[k]|, |up[k]| > 2^30, norm(dir) or norm(up) <
 *   2^-30, up parallel to dir (norm(c)^2 < 2^-40 * norm(up)^2), scale outside [2^-20, 2^20], offset < 0, aperture < 0, aperture > 0
 *   with focus <= 0, or a finished record outside the magnitude bound above.
 * apt_camera_check_host: the same refusals for a record filled in by hand: APT_ERR_STRUCT for a wrong struct_size; APT_ERR_ARG for a
 *   NULL pointer, a non-finite field, a field outside the magnitude bound, g, cx or cy zero, offset < 0, aperture < 0, and with
 *   aperture > 0: focus <= 0, lens_u or lens_v zero, offset_over_focus != offset / focus.
 * All three return APT_ERR_STRUCT when out->struct_size is not sizeof(apt_camera): the caller sets it, as for apt_render_params. */
int apt_camera_default_host(uint32_t width, uint32_t height, apt_camera *out);
int apt_camera_build_host(const double eye[3], const double dir[3], const double up[3], double scale, double offset, double aperture,
                          double focus, uint32_t width, uint32_t height, apt_camera *out);
int apt_camera_check_host(const apt_camera *cam);
/* The context's camera: checked (apt_camera_check_host), copied, part of the snapshot every render call takes.  NULL: back to the
 * reference's camera.  A refused record leaves the previous one in place.  apt_set_camera = the default context. */
int apt_context_set_camera(apt_context *ctx, const apt_camera *cam_or_null);
int apt_set_camera(const apt_camera *cam_or_null);
/* apt_gen_rays_device for a camera: rays [6][N] for paths [path_begin, path_begin + path_count) (APT_FLAG_BAND_BUFFERS as there), the
 * rays the material frame entries trace with this camera set, bit for bit.  The record is the argument's, not the context's. */
int apt_gen_rays_camera_device(const apt_render_params *p, const apt_camera *cam, void *stream, float *rays);

/* ---- environment (EXTENSION: light from the directions where there is no geometry -- a sky and a sun -- for the material renderer) ------
 * Above, a path whose hit test finds no sphere ends and L keeps its value: every ray that leaves the scene is black.  An apt_environment
 * gives those directions a radiance: a sky that blends from `horizon` (d.y = -1) to `zenith` (d.y = +1; the scene's up is +y) and a sun,
 * "a sphere light at infinity": a cone of half angle a around the unit vector sun_dir, sun_omc = 1 - cos(a), of radiance sun_radiance.
 * A context carries at most one (apt_context_set_environment; none = every entry, kernel and image as before).  With one set
 *   - the material and light-table entries -- apt_render_frame_materials, apt_render_paths_materials, apt_render_frame_lights,
 *     apt_render_paths_lights and their apt_context_* forms, frame and buffer mode alike -- read it;
 *   - the mirror frame entries that refuse while a camera is set (render_frame / apt_context_render_frame, apt_render_frame_mt,
 *     apt_multi_create / apt_multi_render) refuse in the same way, APT_ERR_ARG after their own checks: they have no environment;
 *   - a material frame takes a pairwise-sum plan of at most 44 leaves, as with a camera set (APT_ERR_ARG otherwise), and with no camera
 *     set it is rendered from apt_camera_default_host's record, which is the reference's camera bit for bit (APT_ERR_ARG for an image
 *     shape that record refuses);
 *   - the mirror buffer-mode entries (render_do, render_do_ex) take no environment and are unaffected.
 * APT_ABI_VERSION is unchanged: callers detect the feature by its symbols.
 *
 * The arithmetic, in the terms of "per-sphere materials" and "Direct light sampling" above (fp32, every operation rounded on its own:
 * no FMA).  With an environment E a path carries one more flag, `sampled_sun`, false at its start, and the bounce changes in three
 * places:
 *     miss    a live path whose arg-min finds no sphere, along its direction d:
 *             t = d.y * 0.5f + 0.5f (mul, then add); t = t > 0 ? t : 0; t = t < 1 ? t : 1            (a NaN gives 0)
 *             sky_c = horizon_c + (zenith_c - horizon_c) * t;  L_c = L_c + T_c * sky_c                 per channel c
 *             then, if sun_omc > 0 and dot(d, sun_dir) >= 1.0f - sun_omc and not `sampled_sun`: L_c = L_c + T_c * sun_radiance_c.
 *             The path ends.
 *     light   at every hit sampled_sun = false, next to sampled = false.
 *     sun sample  at a DIFF hit when d + 1 < depth, E.flags & APT_ENV_SAMPLE_SUN and sun_omc > 0, after the DIFF direction is drawn and
 *             after the APT_FLAG_NEE / light-table sample if there is one.  "Direct light sampling"'s own arithmetic with w = sun_dir
 *             and omc = sun_omc (no d2, x, cmax or dl: the record holds both):
 *             skey = splitmix64(seed ^ splitmix64(path) ^ APT_ENV_SUN_SALT); (v1, v2) from skey exactly as (u1, u2) from mkey
 *             (one more stream: h = splitmix64(skey + 0x9E3779B97F4A7C15 * (d + 1)), the same 24-bit split)
 *             cos_a = 1 - v1 * omc; sin_a = sqrt(1 - cos_a * cos_a); (sin, cos) of 2*pi*v2 by DIFF's polynomial
 *             (t, bt) = the Duff basis of w; q = (t * (cos * sin_a) + bt * (sin * sin_a)) + w * cos_a per component
 *             l = q / sqrt(dot(q, q)); cosl = dot(l, nl); wgt = cosl * (2 * omc)
 *             sampled_sun = true, whatever follows.
 *             if cosl > 0: a shadow segment from h along l through the hit test, every sphere but this bounce's skip sphere.  The sun
 *             is visible iff that test finds NO sphere.  Visible: L_c = L_c + (T_c * sun_radiance_c) * wgt, T being the throughput
 *             after `T *= albedo` and before this bounce's roulette; it is added after the light's own contribution.
 *   There is NO sample at the last bounce (d + 1 == depth), for the reason given for APT_FLAG_NEE: the sample at bounce d stands for the
 *   sun a miss of segment d + 1 would add.  With this rule APT_ENV_SAMPLE_SUN changes the image by noise only, and at depth 1 by
 *   nothing.  The sun's shadow segment counts as a traced segment in the trace counter (and its cells / candidates in the grid
 *   statistics).  GLOSS, SPEC and REFR hits do not sample: a miss after them adds the sun in full.  The sun sample is independent of
 *   APT_FLAG_NEE and of a light table: it works with neither of them and with either (a launch has at most one of the two).  The cone test
 *   dot(d, sun_dir) >= 1.0f - sun_omc is an fp32 decision: the sampled cone (cos_a >= 1 - omc before q is normalised) and the tested
 *   cone differ by rounding at the rim, a relative solid angle of the order of 2^-23 / sun_omc.  A miss on the camera ray adds sky and
 *   sun like any other.  Roulette, APT_DEV_BAD_MATERIAL, the grid rules (a grid that is not the scene's: nothing written,
 *   APT_DEV_GRID_MISMATCH), APT_FLAG_GLOSS and the light rules are as above.
 * An environment whose radiances are all 0 and that has no sun (sun_omc = 0) adds exactly +0 at a miss: every image is the one without
 * an environment, bit for bit. */
enum { APT_ENV_SAMPLE_SUN = 1u };  /* apt_environment.flags: sample the sun directly at every diffuse hit */
#define APT_ENV_SUN_SALT 0x510E527FADE682D1ull   /* the sun sample's stream; differs from the bounce's, APT_FLAG_NEE's, the light table's, the lens's and roulette's (none) */
typedef struct apt_environment {
    uint32_t struct_size;       /* = sizeof(apt_environment)                                                */
    uint32_t flags;             /* APT_ENV_*                                                                */
    float horizon[3], zenith[3];/* sky radiance at d.y = -1 and d.y = +1                                    */
    float sun_dir[3];           /* unit, towards the sun                                                    */
    float sun_radiance[3];
    float sun_omc;              /* 1 - cos(half angle); 0 = no sun; <= 1                                    */
} apt_environment;

/* Host helpers: no GPU, nothing written unless APT_OK.
 * apt_environment_build_host: sun_dir of any length is normalised in float64, one operation at a time as apt_camera_build_host does
 *   (n = sqrt(fma(d2, d2, fma(d1, d1, d0*d0))), d[k] / n), then every field is rounded ONCE to fp32.  With sun_omc == 0 sun_dir may be
 *   anything finite (a zero vector is stored as it is).  APT_ERR_ARG: a NULL pointer, a non-finite input, a sun_dir shorter than 2^-30
 *   with sun_omc > 0, or a finished record apt_environment_check_host refuses.  APT_ERR_STRUCT when out->struct_size is not
 *   sizeof(apt_environment): the caller sets it.
 * apt_environment_check_host: APT_ERR_STRUCT for a wrong struct_size; APT_ERR_ARG for a NULL pointer, unknown flag bits, a radiance
 *   (horizon, zenith, sun_radiance) that is not finite or is negative, sun_omc outside [0, 1] or NaN, a non-finite sun_dir, and with
 *   sun_omc > 0 a sun_dir whose squared length (float64 from the fp32 fields) is further than 2^-20 from 1.
 * apt_context_set_environment: checked (the same refusals), copied, part of the snapshot every render call takes.  NULL removes it.  A
 *   refused record leaves the previous one in place.  apt_set_environment = the default context. */
int apt_environment_build_host(const double horizon[3], const double zenith[3], const double sun_dir[3] /* any length */,
                               const double sun_radiance[3], double sun_omc, uint32_t flags, apt_environment *out);
int apt_environment_check_host(const apt_environment *env);
int apt_context_set_environment(apt_context *ctx, const apt_environment *env_or_null);
int apt_set_environment(const apt_environment *env_or_null);

/* ---- film (EXTENSION: an unclipped float32 accumulation buffer for the material renderer, filled pass by pass, and its resolve) -------
 * The frame entries return the mean of ONE launch's samples, clipped to [0, 1] (data_visualization.py:54) and truncated to 8 bits.  A
 * film keeps what they clip: frame launches add to it pass by pass, and a resolve kernel turns it into a displayable image with an
 * exposure, a tone operator and a transfer curve.  APT_ABI_VERSION is unchanged: callers detect the feature by its symbols.
 *
 * Accumulate.  apt_render_frame_film / apt_context_render_frame_film:
 *   - film is a DEVICE buffer [3][pixel_count] float32, band-relative exactly as fb is.
 *   - The launch renders the pixel range exactly as apt_render_frame_lights would (lights_or_null == NULL: as apt_render_frame_materials
 *     would) with p->seed replaced by apt_film_pass_seed(p->seed, pass): flags, the context's camera and environment, the grid form
 *     behind `accel`, roulette, the status word, the trace counter, every refusal and the order of refusals are those entries' (a NULL
 *     `materials` is refused there already: there is no mirror film).  A film launch takes a pairwise-sum plan of at most 44 leaves
 *     whether or not a camera or an environment is set (every samples <= 4199 has one; APT_ERR_ARG otherwise), and without a camera set
 *     it renders from apt_camera_default_host's record (APT_ERR_ARG for an image shape that record refuses).  After those refusals the
 *     entry refuses a NULL `film` (APT_ERR_ARG), with nothing written.  An empty pixel range is APT_OK and launches nothing.
 *   - Per pixel and channel the kernel forms the same float64 v as the frame entries: the four sub-pixel np.means summed in float64,
 *     divided by 4 -- the value BEFORE :54's clip.  It does not clip.  r = (float)v.  pass == 0: film[c][pl] = r (a store: whatever the
 *     buffer held, NaN included, is gone).  pass > 0: film[c][pl] = film[c][pl] + r, one fp32 add.  No 8-bit image is written.
 *   - So after pass 0 alone clip(film, 0, 1) is the fb of the corresponding frame entry bit for bit (rounding to fp32 is monotone and 0
 *     and 1 are representable: clipping before or after it is the same), and after passes 0..K-1 the film is the sequential fp32 sum of
 *     K independent frames' (float)v.
 *   - apt_film_pass_seed(seed, 0) = seed; for pass > 0 it is splitmix64(seed ^ splitmix64((uint64_t)pass ^ APT_FILM_PASS_SALT)).  The
 *     salt keeps a pass seed from being the roulette key of path `pass` (splitmix64(seed ^ splitmix64(path))).  The seed is computed
 *     on the host: the kernel receives a seed as it always has.
 *   - Passes are the caller's loop; the entry keeps no state.  A caller may run bands, or resume a film another process wrote.
 *
 * List passes.  APT_FLAG_PIXEL_LIST in p->flags, read by the two film entries above and by nothing else:
 *   - pixel_begin carries the DEVICE address of a uint32_t list of image pixel indices (x-major, as everywhere), the way `accel`
 *     carries an address; pixel_count is the list's length.  film is a compact scratch [3][pixel_count] float32: word
 *     c * pixel_count + i receives entry i's pixel.
 *   - A lane derives its camera ray, its sub-pixel, its path indices and its roulette keys from the image pixel alone, so entry i
 *     receives EXACTLY the bits a launch over the whole image with the same `pass` computes for pixel list[i].
 *   - The launch always STORES that (float)v, whatever `pass` is: `pass` only selects the seed, apt_film_pass_seed(p->seed, pass).  A
 *     list launch has nothing of its own to add to; summing is render_mi355x_adaptive.h's apt_film_accumulate_list_*.
 *   - Everything else is the film entry's: flags, the context's camera and environment, the grid behind `accel`, roulette,
 *     APT_FLAG_MIS, the trace counter, the 44-leaf plan limit, every refusal and their order.  In the place of the pixel-range check:
 *     APT_ERR_ARG for a list address that is 0 or not 4-byte aligned, for pixel_count > width * height, and for
 *     width * height > 2^32; pixel_count == 0 is APT_OK with nothing launched.
 *   - An entry >= width * height makes its lanes invalid, exactly as lanes past the range are: they write nothing, so the entry's three
 *     scratch words are left untouched, and the kernel ORs APT_DEV_LIST_RANGE into the status word (without a status word such
 *     entries are skipped silently).  Lanes past the end of the list read list[0], never past the end.
 *   - A list may repeat an entry here: each slot has its own owner lane.
 *
 * Resolve.  apt_film_resolve_device (DEVICE pointers, asynchronous on `stream`) and apt_film_resolve_host (HOST pointers, the CPU twin:
 * the same operations, the same bits).  Every step is one IEEE fp32 operation (no FMA).  Per value s of the film:
 *     m = s / (float)passes                      (1 <= passes <= 2^24: the conversion is exact)
 *     x = m * exposure;  x = x > 0 ? x : 0       (a NaN and a negative value become 0)
 *     APT_TONEMAP_CLIP:      y = x < 1 ? x : 1
 *     APT_TONEMAP_REINHARD:  y = (x * (1 + x * inv_white2)) / (1 + x), with x == +inf giving 1 by a select before the divide (as does
 *                            an intermediate that overflows: a NaN quotient gives 1); then y = y < 1 ? y : 1.  inv_white2 = 0 is plain
 *                            Reinhard; inv_white2 = 1 / white^2 maps the radiance `white` to 1.
 *     out[c][i] = y                              (out_or_null: [3][pixel_count] float32)
 *     u8[i][c] = #{ k in 1..255 : table[k] <= y }  (u8_or_null: [pixel_count][3]; any byte alignment)
 *   The code is a search in a 256-entry table (table[0] is not read), numpy's searchsorted(table[1:], y, side="right") for an increasing
 *   table, done as 8 branch-free steps: code = 0; for b = 128, 64, ..., 1: if (table[code + b] <= y) code += b.  There is no pow on the
 *   device: the code is reproducible bit for bit.  For a table that is not increasing the code is what those 8 steps give.
 *   apt_film_curve_host fills table[0] = 0 and table[k] = (float)EOTF((k - 0.5) / 255) (float64, rounded once) for k = 1..255: the level
 *   boundaries of an encoding that is ROUNDED to the nearest of 256 levels, unlike the reference decode's truncation, which stays what it
 *   is in the frame entries.  APT_CURVE_LINEAR: EOTF(e) = e.  APT_CURVE_SRGB: e <= 0.04045 ? e / 12.92 : pow((e + 0.055) / 1.055, 2.4).
 *   APT_ERR_ARG for a NULL table or an unknown curve.
 *   Refusals of both resolve forms, nothing written: APT_ERR_ARG for a NULL r, film or table, both outputs NULL, passes == 0 or
 *   > 2^24, an unknown operator, an exposure or inv_white2 that is not finite or is negative; APT_ERR_STRUCT for a wrong struct_size.
 *   pixel_count == 0 is APT_OK.  The device form does not read the table on the host.
 * apt_write_pfm: a colour PFM ("PF\n<w> <h>\n-1.0\n", then little-endian float32 RGB, rows bottom to top) of HOST planes [3][W*H],
 *   x-major as fb (pixel (x, y) at x * H + y).  y counts upwards here, so file row r is y = r: apt_write_ppm flips, this does not. */
#define APT_FILM_PASS_SALT 0x9B05688C2B3E6C1Full   /* differs from every stream salt above */
enum { APT_TONEMAP_CLIP = 0, APT_TONEMAP_REINHARD = 1 };
enum { APT_CURVE_LINEAR = 0, APT_CURVE_SRGB = 1 };
typedef struct apt_film_resolve {
    uint32_t struct_size;       /* = sizeof(apt_film_resolve)                                               */
    uint32_t passes;            /* passes accumulated in the film, 1 .. 2^24                                */
    uint32_t tonemap;           /* APT_TONEMAP_*                                                            */
    uint32_t reserved;          /* not read                                                                 */
    float exposure;             /* finite, >= 0                                                             */
    float inv_white2;           /* APT_TONEMAP_REINHARD: 1 / white^2, finite, >= 0; 0 = plain Reinhard      */
} apt_film_resolve;
uint64_t apt_film_pass_seed(uint64_t seed, uint32_t pass);   /* host; pass 0 -> seed itself */
int apt_render_frame_film(const apt_render_params *p, void *stream, const float *spheres, const uint32_t *materials,
                          const void *lights_or_null, uint64_t pixel_begin, uint64_t pixel_count, float *film, uint32_t pass);
int apt_context_render_frame_film(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                                  const uint32_t *materials, const void *lights_or_null, uint64_t pixel_begin, uint64_t pixel_count,
                                  float *film, uint32_t pass);
int apt_film_curve_host(uint32_t curve, float table[256]);
int apt_film_resolve_device(const apt_film_resolve *r, void *stream, const float *film, uint64_t pixel_count, const float *table_dev,
                            float *out_or_null, uint8_t *u8_or_null);
int apt_film_resolve_host(const apt_film_resolve *r, const float *film, uint64_t pixel_count, const float *table, float *out_or_null,
                          uint8_t *u8_or_null);
int apt_write_pfm(const char *path, uint32_t width, uint32_t height, const float *planes_host);

/* ---- features (EXTENSION: first-hit feature planes of the material renderer's film: coverage, depth, normal, albedo) -----------------
 * What lies under each pixel, without light transport: the guides of an external denoiser, depth for compositing and fog, masks, a
 * look at a scene or a camera.  The planes describe the FIRST surface a camera ray meets: a mirror or a pane of glass is that surface,
 * nothing is followed through it.  One launch is one stored result; there is no per-pass accumulation.  APT_ABI_VERSION is unchanged:
 * callers detect the feature by its symbols.
 *
 * apt_render_frame_features / apt_context_render_frame_features:
 *   - features is a DEVICE buffer [APT_FEATURE_PLANES][pixel_count] float32, band-relative and x-major exactly as fb and the film are
 *     (pixel (x, y) of a whole image at x * height + y).  Plane APT_FEATURE_COVERAGE (0) is the coverage, APT_FEATURE_DEPTH (1) the
 *     depth, APT_FEATURE_NORMAL (2, 3, 4) the normal, APT_FEATURE_ALBEDO (5, 6, 7) the albedo.
 *   - Rays.  The paths of pixel P are [P * 4 * S, (P + 1) * 4 * S), S = samples, and their rays are the ones a material frame launch
 *     with the same width, height, samples, seed and context camera generates (without a camera: apt_camera_default_host's record):
 *     tent filter and thin lens included, so the planes are anti-aliased and carry the image's depth of field.
 *   - First hit.  render_do_ex's K-mode test of every sphere with p->eps, no sphere skipped, the lowest index on ties: the first
 *     segment of a material path.
 *   - Per path, on a hit of sphere k at tmin, every step one fp32 operation (no FMA), as in the bounce:
 *         c = 1;  t = tmin;  h = o + d * tmin;  nr = h - centre_k;  nu = nr / sqrt(dot(nr, nr));
 *         n = dot(d, nu) < 0 ? nu : -nu      (the bounce's nl; dot as ((0 + x) + y) + z)
 *         a = the sphere table's albedo, rows 7..9 of k
 *     On a miss all eight values are 0.
 *   - Per pixel, each of the eight values is summed over the pixel's paths in ascending path order in float64, the sum is divided by
 *     (double)(4 * S), and the quotient, rounded once to fp32, is STORED: whatever the buffer held, NaN included, is gone.  No clip;
 *     the mean normal is not renormalised.
 *   - Of *p the entry reads width, height, samples, seed, num_spheres, eps, and accel together with APT_FLAG_GRID_SLOTS (the grid
 *     form, as the material entries take it; the 8-sphere scene ignores a grid).  Every other flag and field is ignored, so the record
 *     of a film pass can be handed over as it is.  There is no material table.
 *   - Refusals, nothing written: the params record's own (NULL, struct_size, a zero width / height / samples / num_spheres, accel
 *     without APT_FLAG_GRID_SLOTS), then those of a film launch in its order -- a NULL `spheres`, the pixel range, the size of one
 *     launch, a pairwise-sum plan of more than 44 leaves (every samples <= 4199 has one), an image shape apt_camera_default_host
 *     refuses when no camera is set -- so that a film and its features accept the same calls; after them a NULL `features`
 *     (APT_ERR_ARG).  An empty pixel range is APT_OK and launches nothing.  A grid that is not the scene's leaves the buffer untouched
 *     and reports APT_DEV_GRID_MISMATCH through the status word. */
enum { APT_FEATURE_COVERAGE = 0, APT_FEATURE_DEPTH = 1, APT_FEATURE_NORMAL = 2, APT_FEATURE_ALBEDO = 5, APT_FEATURE_PLANES = 8 };
int apt_render_frame_features(const apt_render_params *p, void *stream, const float *spheres, uint64_t pixel_begin, uint64_t pixel_count,
                              float *features);
int apt_context_render_frame_features(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                                      uint64_t pixel_begin, uint64_t pixel_count, float *features);

/* ---- one process, several GPUs (the reference's 8-block split, src/render.cpp:9-10,24-27, across devices) ----
 * The frame's x-major pixel range is cut into num_bands*stripes contiguous stripes; band b renders stripes
 * b, b+num_bands, ... (stripes == 1: one contiguous band per device, the reference's split; stripes > 1
 * interleaves them, which balances APT_FLAG_RETIRE's uneven columns) on device_ids[b] with render_frame on a
 * stream of its own, and every stripe is copied straight into the full frame on the root device
 * (device_ids[0]) with hipMemcpyPeerAsync -- over xGMI each peer has its own link to the root, so the copies
 * of different bands run in parallel; a gather to one root needs no collective.  A device may appear more
 * than once in device_ids (several bands on one GPU).
 *   apt_multi_create   allocates per-band streams, the scene copy and stripe buffers (spheres_host: HOST table)
 *   apt_multi_render   renders one frame into fb_root [3][W*H] (+ u8_root [W*H][3] or NULL), DEVICE pointers on
 *                      the root device; synchronous (returns when the frame is complete);
 *                      band_kernel_ms: optional HOST float[num_bands], each band's kernel time (HIP events)
 * apt_render_params.accel is refused (a grid address belongs to one device).  One process per GPU with
 * torch.distributed (ascendpathtracing_amd/dist.py) is the other, equivalent way to shard. */
typedef struct apt_multi apt_multi;
int  apt_multi_create(const int *device_ids, uint32_t num_bands, uint32_t stripes, const apt_render_params *p,
                      const float *spheres_host, apt_multi **out);
int  apt_multi_render(apt_multi *m, float *fb_root, uint8_t *u8_root, float *band_kernel_ms);
void apt_multi_destroy(apt_multi *m);

/* First-hit debug mode, scripts/gen_data.py:134-188 test_scene: out [3][N] = emission of the
 * light sphere when it is the nearest hit, the hit sphere's colour otherwise, 0 on a miss
 * (test_scene's own arithmetic: float64-accumulated dot products). */
int apt_test_scene(const apt_render_params *p, void *stream, const float *rays,
                   const float *spheres, float *out);

/* Device gen_rays with the counter-based generator: writes rays [6][N] planes for paths
 * [path_begin, path_begin+path_count) of the full buffer (same rays render_frame traces). */
int apt_gen_rays_device(const apt_render_params *p, void *stream, float *rays);

/* Device gen_rays that is BIT-EXACT with scripts/gen_data.py:21-75 under np.random.seed(seed):
 * the MT19937 stream is regenerated on the device from host-made checkpoints (the raw 624-word
 * state every `stride` output blocks; one block = 624 words = 156 paths).
 *   apt_mt19937_checkpoints_host(seed, num_blocks, stride, states): states = HOST uint32
 *       [ceil(num_blocks/stride)][624]; num_blocks = ceil(N/156).  Sequential, done once per seed;
 *       a table made for a longer stream serves every shorter one.
 *   apt_gen_rays_mt_device(p, stream, checkpoints_dev, stride, num_checkpoints, rays): rays [6][N],
 *       paths [path_begin, path_begin+path_count).  p->seed is not used (the seed is in the table). */
int apt_mt19937_checkpoints_host(uint32_t seed, uint64_t num_blocks, uint32_t stride, uint32_t *states);
int apt_gen_rays_mt_device(const apt_render_params *p, void *stream, const uint32_t *checkpoints,
                           uint32_t stride, uint64_t num_checkpoints, float *rays);
/* Windowed forms, for frames whose whole stream is too long to tabulate at once (C3: 1.7e10 paths):
 *   apt_mt19937_checkpoints_window(state_in, seed, first_block, num_blocks, stride, states, state_out):
 *       checkpoints of output blocks first_block + k*stride, k < ceil(num_blocks/stride).  state_in = the raw
 *       624-word state of block first_block (from an earlier call's state_out, or a stored one), or NULL to twist
 *       there from the seed (first_block+1 sequential twists).  state_out (or NULL) receives the raw state of
 *       block first_block + num_blocks, so that windows chain.
 *   apt_gen_rays_mt_device_ex: as apt_gen_rays_mt_device with a table whose entry 0 is block first_block;
 *       the call's path range must lie inside the window; honours APT_FLAG_BAND_BUFFERS. */
int apt_mt19937_checkpoints_window(const uint32_t *state_in, uint32_t seed, uint64_t first_block, uint64_t num_blocks,
                                   uint32_t stride, uint32_t *states, uint32_t *state_out);
int apt_gen_rays_mt_device_ex(const apt_render_params *p, void *stream, const uint32_t *checkpoints, uint32_t stride,
                              uint64_t num_checkpoints, uint64_t first_block, float *rays);

/* The reference's EXACT pipeline in one launch (round 3; SURVEY 8(f)-1 "removes the rays.bin file/HBM boundary"):
 * MT19937 gen_rays (scripts/gen_data.py:21-75 under np.random.seed, :438) -> the render loop (src/render.cpp:104-207; in
 * APT_MODE_ORACLE the arithmetic of gen_data.py:246-429 test_soa) -> decode_color (scripts/data_visualization.py:36-57),
 * without the [6][N] ray buffer and the [3][N] colour buffer: bit-identical to apt_gen_rays_mt_device -> render_do_ex ->
 * apt_decode_color_device.  One workgroup per GROUP of 78 pixels (78 * 4 * samples paths = 2 * samples generator blocks of
 * 156 paths, for EVERY sample count): checkpoints[k] = the raw 624-word state of block (first_group + k) * 2 * samples,
 * i.e. apt_mt19937_checkpoints_window(state_in, seed, first_group * 2 * samples, groups * 2 * samples, 2 * samples, ...).  Renders
 * pixels [pixel_begin, pixel_begin + pixel_count) into fb [3][pixel_count] (+ fb_u8 [pixel_count][3] or NULL); the table must
 * cover groups pixel_begin / 78 .. (pixel_begin + pixel_count - 1) / 78.  The 8-sphere scene, no APT_FLAG_RR; any sample count that has a
 * pairwise-sum plan (every count <= 7688; since round 4 -- before: 8, 16, ..., 256 only -- incl. the reference's own default, 16 x 16 with
 * samples = 1, src/common.h:4-6).  Enqueues on `stream`, allocates nothing. */
int apt_render_frame_mt(const apt_render_params *p, void *stream, const uint32_t *checkpoints, uint64_t num_checkpoints,
                        uint64_t first_group, const float *spheres, uint64_t pixel_begin, uint64_t pixel_count,
                        float *fb, uint8_t *fb_u8);

/* Device decode_color: colors [3][N] -> fb float32 [3][W*H] (+ fb_u8 [W*H][3] or NULL),
 * same arithmetic as scripts/data_visualization.py:20-59. */
int apt_decode_color_device(const apt_render_params *p, void *stream, const float *colors,
                            float *fb, uint8_t *fb_u8);

/* The same for a band: colors_band = float32 [3][pixel_count*4*S] holding the paths of pixel_count consecutive
 * pixels (APT_FLAG_BAND_BUFFERS layout) -> fb [3][pixel_count] (+ fb_u8 [pixel_count][3] or NULL).  decode_color
 * does not depend on where in the image the pixels lie. */
int apt_decode_color_band(const apt_render_params *p, void *stream, const float *colors_band, uint64_t pixel_count,
                          float *fb, uint8_t *fb_u8);

/* ---- host-side helpers (no GPU) -------------------------------------------------------
 * Host gen_rays, bit-exact with scripts/gen_data.py:21-75 under np.random.seed(seed)
 * (MT19937 legacy stream).  rays = HOST float32 [6][N]. */
int apt_gen_rays_host(uint32_t width, uint32_t height, uint32_t samples, uint32_t seed,
                      float *rays);

/* Host gen_spheres (scripts/gen_data.py:92-132): writes the 128-float / 512-byte table. */
int apt_gen_spheres_host(float *spheres128);

/* Build-defined large scene (BASELINE config 4; the reference has no generator):
 * spheres 0..5 the six walls, 6..Ns-2 random small spheres, Ns-1 the light.
 * Writes [10][Ns] planes zero padded to a multiple of 128 floats; *out_floats receives the
 * padded length.  Pass spheres == NULL to query the length. */
int apt_gen_scene_host(uint32_t num_spheres, uint64_t seed, float *spheres,
                       size_t *out_floats);

/* Acceleration structure for scenes far larger than LDS (num_spheres != 8): a uniform grid over the
 * small spheres plus an always-tested list of the large ones (walls, light).  Built on the HOST from
 * the same [10][Ns] table the kernels read; the caller copies the `*out_bytes` bytes to the device and
 * passes that address in apt_render_params.accel.  Pass grid == NULL to query the size.  Rendering
 * with it is bit-identical to rendering without: every candidate goes through the reference's exact
 * intersection arithmetic, the traversal only skips spheres that provably cannot be hit, and ties keep
 * the lowest sphere index.  The buffer holds two forms of the lists: item ranges (the nested walk of buffer
 * mode and of samples < 8) and, since round 3, pair-slot tables (two candidates per 32-byte slot, one word per
 * cell) for the frame kernel's per-lane walk; apt_render_frame picks the kernel from what the buffer carries,
 * on the device. */
int apt_build_grid_host(const float *spheres_host, uint32_t num_spheres, void *grid, size_t *out_bytes);

/* The flags a built grid earns for a scene of `num_spheres` spheres, from the first 128 bytes of the buffer (HOST memory: the
 * buffer apt_build_grid_host filled, or a copy of the head of a device-built one): APT_FLAG_GRID_SLOTS when it is a grid for that
 * sphere count with pair-slot tables, else 0.  OR the result into apt_render_params.flags next to `accel`. */
uint32_t apt_grid_flags(const void *grid_head_host, uint32_t num_spheres);

/* The same grid built ON THE DEVICE from the [10][Ns] table in device memory: byte-identical to what
 * apt_build_grid_host writes for that scene (radix-select median, scans and atomics in kernels; the scalar header
 * arithmetic is the host's own).  grid_dev = DEVICE buffer of `capacity` bytes, or NULL to query the size
 * (*out_bytes).  Synchronous on `stream` (two small read-backs size the buffer) and allocates its workspace: a
 * build step, not capture-safe.  Up to 512 cells per axis (round 1: 128). */
int apt_build_grid_device(const float *spheres_dev, uint32_t num_spheres, void *stream, void *grid_dev,
                          size_t capacity, size_t *out_bytes);

/* P3 writer of scripts/data_visualization.py:11-17 from a [pixel][3] uint8 image in
 * x-major pixel order (q = i*H + j, y not flipped). */
int apt_write_ppm(const char *path, uint32_t width, uint32_t height, const uint8_t *fb_u8);

/* ---- diagnostics ------------------------------------------------------------------- */
/* Optional DEVICE uint64[4] statistics block.  [0] += ray segments actually traced by every
 * render launch (== paths*depth unless APT_FLAG_RETIRE); [1], [2] += lane-slots (64 per wave-level
 * execution) spent in bounce / ray-generate by the refill loop of render_frame; [3] += wave-level
 * exact re-runs of a bounce (full-trace Ns = 8 loop).  NULL disables it.
 * The caller zeroes it; process-wide. */
int apt_set_trace_counter(uint64_t *device_counter);

/* Self-test of the hot loop's fast correctly-rounded sqrt: compares it with sqrtf() for every
 * float whose bit pattern lies in [first_bits, first_bits+count) (count = 2^32 covers all).
 * variant 0 = neighbour check (shade), 1..3 = FMA-correction candidates; the intersect loop uses 2.
 * device_result2[0] += number of mismatches, device_result2[1] = min(first mismatching bits);
 * the caller initialises them to 0 and ~0. */
int apt_selftest_sqrt(int variant, void *stream, uint64_t first_bits, uint64_t count,
                      uint64_t *device_result2);

/* Self-test of the shared-reciprocal divide of the shading step against the plain `/` on
 * `count` hashed operand sets starting at counter `first`.  device_result3[0] += mismatches,
 * [1] = min(first mismatching counter), [2] += sets inside the accepted operand range.
 * Initialise to 0, ~0, 0. */
int apt_selftest_div3(void *stream, uint64_t first, uint64_t count, uint64_t *device_result3);

/* Self-test of the two-path bounce's divide (csrc/pt_core.h div3_seeded_packed2: the reciprocal refined from the square
 * root's v_rsq_f32 seed by two Newton steps, one residual round per quotient, a flag for the one divisor family whose
 * reciprocal may not converge) against the plain `/`.
 *   part 0: the operand sets [first, first + count) of apt_selftest_div3's generator;
 *   part 1: every len2 whose bit pattern lies in [first, first + count), d = sqrtf(len2), four numerator triples each;
 *   part 2: the divisor with bit pattern `first`, numerator mantissa i & 0x7fffff at exponent class i >> 23 for
 *           i in [0, count), count <= 3 * 2^23, from the v_rsq_f32 seed of every len2 next to d * d whose sqrtf() is d and from
 *           RN(1/d) - 1, + 0, + 1 ulp.
 * device_result8: [0] += accepted sets with a wrong quotient (must stay 0), [1] = min(first such index), [2] += accepted
 * sets, [3] += sets in range whose flag is raised (they take the exact form in the renderer), [4] += of those, the ones whose
 * divisor mantissa is NOT all ones (must stay 0), [5] += sets inside the operand range of the bounce's validity chain,
 * [6] += (part 0) sets the scalar form's own flags accept -- [5] + [6] is what apt_selftest_div3 reports as accepted on the
 * same range --, [7] += accepted sets whose refined reciprocal is not RN(1/d).  Initialise to 0, ~0, 0, 0, 0, 0, 0, 0. */
int apt_selftest_div3_seeded(void *stream, int part, uint64_t first, uint64_t count, uint64_t *device_result8);

/* Self-test of ray-generate's direction: the device makes d / |d| in float32 from one refined reciprocal square root and accepts a
 * component only where that provably rounds like the reference's float64 sqrt and divisions (csrc/pt_core.h fast_direction); a ray
 * with a rejected component is redone in the exact form.  d3 = `count` vectors (d0, d1, d2), float64.  result5: [0] += vectors
 * accepted, [1] += vectors rejected, [2] += accepted components whose float32 differs from the exact form's (must stay 0),
 * [3] += vectors rejected by the ray-level part of the rule (operand range, certificate), [4] = max(bits of |certificate|) -- the
 * caller zeroes all five.  flags (or NULL): per vector, bit k = component k accepted, bit 3 + k = component k differs, bit 6 = the
 * ray-level part passes.
 * apt_selftest_direction: DEVICE buffers, the real v_rsq_f64, against the device's sqrt() and `/`.
 * apt_selftest_direction_host: HOST buffers, no GPU; (1/sqrt(n2)) * (1 + rsq_rel_error), |rsq_rel_error| <= 2^-20, stands in for the
 * instruction. */
int apt_selftest_direction(void *stream, const double *d3, uint64_t count, uint64_t *device_result5, uint8_t *device_flags);
int apt_selftest_direction_host(const double *d3, uint64_t count, double rsq_rel_error, uint64_t *result5, uint8_t *flags);

/* Self-test (host, no GPU) of the generator states render_frame's two-paths-per-lane kernel forms by addition -- one base state per
 * lane, plus a multiple of the per-path stride that is the same for a whole wave -- for every lane of pixels [pixel_begin,
 * pixel_begin + pixel_count) and every pair of samples of the frame's summation plan, against the counter generator's definition
 * (the two 64-bit outputs of path (pixel * 4 + sub-pixel) * samples + k).  result3: [0] += samples checked, [1] += samples whose
 * outputs differ (must stay 0), [2] += samples the kernel traces one at a time, from the definition itself; the caller zeroes them. */
int apt_selftest_chain_states_host(uint32_t samples, uint64_t seed, uint64_t pixel_begin, uint64_t pixel_count, uint64_t *result3);

/* Self-test (host, no GPU) of the tent filter made straight from the generator's bits (csrc/pt_core.h tent_e_from_bits, tent_e: the
 * ray-generate of render_frame's two-paths-per-lane kernel) against the form from the uniform itself (tent_t(unit_from_bits(z))), for
 * the 64-bit generator outputs z[0 .. count).  result2: [0] += outputs whose square-root arguments differ in their bits, [1] += outputs
 * whose results differ other than in the sign of a zero (both must stay 0); the caller zeroes them. */
int apt_selftest_tent_bits_host(const uint64_t *z, uint64_t count, uint64_t *result2);

/* Tuning knob of the APT_FLAG_RETIRE compaction in render_frame: a wave runs its (expensive,
 * float64) ray-generate when at least `lanes` of its 64 lanes have an empty ray slot (default
 * 32).  Speed only: results are bit-identical for every value.  Default context. */
int apt_set_refill_lanes(uint32_t lanes);

int         apt_abi_version(void);
const char *apt_last_error(void);       /* this thread's last call: "" when it succeeded */
int         apt_last_status(void);      /* this thread's last call: APT_OK or APT_ERR_* (how a caller of the void
                                           render_do learns the outcome) */
int         apt_device_count(void);     /* number of HIP devices, 0 when none */

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif /* RENDER_MI355X_H */
