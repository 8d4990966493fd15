// render_kernels.hip -- the one translation unit of the device side of librender_mi355x.so: host-side
// launch logic and the C-ABI (include/render_mi355x.h) on top of
//     pt_core.h     the reference's arithmetic, shared with the host helpers
//     pt_trace.h    scene access + bounce loops (8-sphere SGPR path, LDS tiles, grid walk)
//     pt_kernels.h  the __global__ kernels
// What the host code acquires from HIP -- device memory, streams, events, the current device -- it holds through hip_own.h's owners.
// One lane = one path; the whole bounce loop lives in registers (the reference moves 64-ray tiles through
// a 16 KB scratch buffer with a free-list allocator, src/allocator.h -- no counterpart here).  No MFMA:
// this is branchy fp32 VALU work whose separately rounded mul/add an MFMA chain could not reproduce.
// Built with -ffp-contract=off -fno-slp-vectorize (Makefile); see DESIGN.md sections 2 and 4.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <new>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/render_mi355x.h"
#include "apt_host.h"
#include "apt_materials.h"
#include "hip_own.h"
#include "pt_core.h"
#include "pt_dispatch.h"

#include "pt_kernels.h"
#include "pt_grid_build.h"

namespace {

// ---- host side ----------------------------------------------------------------------------
using apt::clear_error;
int fail(int code, const char *fmt, const char *detail = "") { return apt::set_error(code, fmt, detail); }
int hip_fail(hipError_t e) { return fail(APT_ERR_DEVICE, "HIP: %s", hipGetErrorString(e)); }
// a HIP call whose failure ends the entry: APT_ERR_DEVICE "HIP: ...", and the owners release what the entry holds
#define HIP_TRY(call) do { if (hipError_t e_ = (call); e_ != hipSuccess) return hip_fail(e_); } while (0)
int launched() { HIP_TRY(hipGetLastError()); return APT_OK; }   // the outcome of the launches just made

// Run-time settings -> template arguments: with_mode / with_flag, pt_dispatch.h.

int no_leaf_plan() { return fail(APT_ERR_ARG, "samples too large: its pairwise-sum plan needs more than 64 leaves (every count <= 7688 fits, and 8192)%s"); }
int make_leaf_prog(uint32_t samples, LeafProg &lp) { return make_leaf_plan(samples, lp) ? APT_OK : no_leaf_plan(); }   // the plan itself: pt_leaf.h

// The workgroups of one launch as a grid size, or the entry's own refusal `msg` when one launch does not take that many.
int one_launch(uint64_t blocks, const char *msg, unsigned *grid = nullptr) {
    if (blocks > 0x7fffffffull) return fail(APT_ERR_ARG, msg);
    if (grid) *grid = (unsigned)blocks;
    return APT_OK;
}

// What of the record an entry reads, and so checks: the mirror entries all of it, the *_materials entries not light_index with
// APT_FLAG_EMISSION (include/render_mi355x.h), the feature planes neither mode nor light_index.
enum class Reads { All, Materials, Features };
int check_params(const apt_render_params *p, Reads reads = Reads::All) {
    if (!p) return fail(APT_ERR_ARG, "params is null%s");
    if (p->struct_size != sizeof(apt_render_params)) return fail(APT_ERR_STRUCT, "apt_render_params.struct_size mismatch%s");
    if (!p->width || !p->height || !p->samples) return fail(APT_ERR_ARG, "width/height/samples must be non-zero%s");
    if (reads != Reads::Features && p->mode > APT_MODE_ORACLE) return fail(APT_ERR_ARG, "unknown mode%s");
    if (p->num_spheres == 0) return fail(APT_ERR_SCENE, "num_spheres is 0%s");
    if (reads == Reads::Features) return APT_OK;
    if (p->light_index >= (int32_t)p->num_spheres) return fail(APT_ERR_SCENE, "light_index out of range%s");
    if (reads == Reads::All && (p->flags & APT_FLAG_EMISSION) && p->light_index < 0) return fail(APT_ERR_SCENE, "APT_FLAG_EMISSION needs a light_index >= 0%s");
    return APT_OK;
}

// What the material entries refuse on top of check_params (after it, before any pointer or range check of the entry itself).
// lights: a *_lights entry, which reads neither APT_FLAG_NEE nor light_index.
int check_materials(const apt_render_params *p, const uint32_t *materials, bool lights = false) {
    if (!materials) return fail(APT_ERR_ARG, "materials must be non-null%s");
    if (p->mode != APT_MODE_KERNEL) return fail(APT_ERR_ARG, "materials need APT_MODE_KERNEL (O-mode restates test_soa, which has none)%s");
    // a grid only on the caller's word that it is this scene's (apt_grid_flags): the material kernels are one launch, never a second one beside it
    if (p->accel && !(p->flags & APT_FLAG_GRID_SLOTS)) return fail(APT_ERR_ARG, "materials: accel (grid) needs APT_FLAG_GRID_SLOTS (apt_grid_flags of the built grid)%s");
    if (!lights && (p->flags & APT_FLAG_NEE) && p->light_index < 0) return fail(APT_ERR_SCENE, "APT_FLAG_NEE samples the sphere light_index: it needs a light_index >= 0%s");
    return APT_OK;
}

// A context's camera (include/render_mi355x.h "camera") serves the material frame entries only.  The mirror frame entries have exactly the
// reference's camera and refuse, after their own checks, rather than render a frame from a viewpoint the caller did not ask for.
// The same holds for a context's environment ("environment"): the mirror renderer has none, and refuses with the same status.
int refuse_camera(const apt_context::Values &cv, const char *entry) {
    if (cv.has_env) return fail(APT_ERR_ARG, "%s: the context has an environment set (apt_context_set_environment), which the mirror frame entries do not take: unset it, or use the material entries", entry);
    return cv.has_camera ? fail(APT_ERR_ARG, "%s: the context has a camera set (apt_context_set_camera), which the mirror frame entries do not take: unset it, or use apt_gen_rays_camera_device + render_do_ex + apt_decode_color_device", entry) : APT_OK;
}

// A material entry's own arguments: which entry it is, and what it was given.  lights: with_lights entries only (device light table).
struct MatArgs {
    const uint32_t *materials = nullptr;
    bool with_lights = false;
    const void *lights = nullptr;
    apt::MatFilm film = apt::MatFilm::None;   // the film entries ("film" in the header): fb is a film, fb_u8 null
    bool list = false;                        // APT_FLAG_PIXEL_LIST on a film entry: pixel_begin is a device list's address, pixel_count its length
};
// check_materials, then what the *_lights entries refuse on top of it.
int check_mat_args(const apt_render_params *p, const MatArgs &m) {
    int rc = check_materials(p, m.materials, m.with_lights);
    if (rc) return rc;
    if (m.with_lights && !m.lights) return fail(APT_ERR_ARG, "lights must be non-null (a device light table: apt_build_lights_host)%s");
    return APT_OK;
}
// A light table names spheres by index, and the kernel that finds it is not this scene's can only say so through the status word.
// Without one the call is refused here rather than launched on trust.
int check_lights_status(const MatArgs &m, const uint32_t *status) {
    if (m.with_lights && !status) return fail(APT_ERR_DEVICE, "lights: the context has no device status word here (its first launch on this device is inside a stream capture, or the device index is beyond its table)%s");
    return APT_OK;
}

// The device status word of `ctx` on the current device (include/render_mi355x.h "Device-side failure channel"), made on the
// context's first launch there: one allocation of apt::kFirstPlanAllocWords words (8256 bytes), once.  Null -- the kernels then report
// nothing -- when it does not exist yet and cannot be made now (the stream is being captured, or the allocation failed).
// Behind the word, in the same allocation, the slots of the first-bounce plan records (pt_first_plan.h, kFirstPlanBase: layout, tickets and
// why a record is never read as another launch's).  The ticket count is one for the process, not one per context: a ticket only has to
// differ from every other launch's that may write the same memory, and a count no two launches share does that for every context at once.
std::atomic<uint64_t> g_plan_ticket{1};
// (A frame wider or higher than 2^24 gets no ticket either: its record would be the all-zero one, and first_plan_cond() compares in int32,
// where a width or height from 2^31 on turns "the last 0 columns" into every column -- pt_first_plan.h.)
uint64_t plan_ticket(uint32_t *status, uint32_t width, uint32_t height) {   // 0: no allocation (the capture-first case above), the frame kernel skips nothing
#ifdef APT_TEST_NO_FIRST_PLAN   // test build only (make variant ... EXTRA=-DAPT_TEST_NO_FIRST_PLAN): no plan at all, to tell a rule's fault from the kernel's
    return 0u;
#endif
    if (width > apt::kFirstPlanMaxSide || height > apt::kFirstPlanMaxSide) return 0u;
    return status ? g_plan_ticket.fetch_add(1u, std::memory_order_relaxed) : 0u;
}
uint32_t *status_word(apt_context &ctx, hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (dev < 0 || dev >= apt::kMaxStatusDevices) return nullptr;   // beyond the table: no word (and no allocation per launch)
    if (uint32_t *w = ctx.status_lookup(dev)) return w;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (cs != hipStreamCaptureStatusNone) return nullptr;
    apt::DeviceBuffer<uint32_t> fresh;
    if (fresh.alloc(apt::kFirstPlanAllocWords) != hipSuccess || hipMemset(fresh.get(), 0, apt::kFirstPlanAllocWords * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    uint32_t *spare = nullptr;
    uint32_t *w = ctx.status_adopt(dev, fresh.release(), &spare);
    apt::DeviceBuffer<uint32_t> loser(spare);   // another thread was first (or the device index is beyond the table)
    return w;
}

// What a render call needs from its context: one consistent copy of the values and the status word of the current device.
struct Launch { apt_context::Values cv; uint32_t *status; };
Launch launch_state(apt_context &ctx, void *stream) { return Launch{ctx.snapshot(), status_word(ctx, (hipStream_t)stream)}; }

TraceArgs make_trace_args(const apt_render_params *p, const Launch &ls) {
    const apt_context::Values &cv = ls.cv;
    TraceArgs ta;
    ta.ns = p->num_spheres; ta.depth = p->depth; ta.light = p->light_index;
    ta.eps = p->eps; ta.gain = p->gain; ta.traced = cv.trace_counter;
    ta.status = ls.status;
    ta.refill_lanes = cv.refill_lanes;
    ta.grid = (p->num_spheres != 8) ? reinterpret_cast<const uint32_t *>((uintptr_t)p->accel) : nullptr;   // (8 spheres: null, or the two-path frame kernel's plan ticket -- pt_trace.h first_plan_ticket)
    ta.grid_walk = 0;
    ta.emission = (p->flags & APT_FLAG_EMISSION) ? 1u : 0u;
    ta.rr_start = (p->flags & APT_FLAG_RR) ? (p->rr_start ? p->rr_start : 3u) : 0u;
    ta.seed = p->seed;
    return ta;
}

apt::MatTrace make_mat_trace(const apt_render_params *p, const Launch &ls, const MatArgs &m) {
    const TraceArgs ta = make_trace_args(p, ls);
    // The grid form reports a grid that breaks the caller's promise through the status word and renders nothing.  Without a word (a
    // context's first launch inside a stream capture, a device index beyond the context's table) it would do so silently: the tile
    // form, which needs no promise, renders the same image then.  (ta.grid is null for the 8-sphere scene: make_trace_args.)
    // A light table stands for APT_FLAG_NEE and light_index, which its entries do not read.
    // APT_FLAG_MIS is read only next to APT_FLAG_GLOSS and a light mode (the flag or a table); everywhere else the bit is ignored.
    const uint32_t *lights = m.with_lights ? static_cast<const uint32_t *>(m.lights) : nullptr;
    const bool nee = !lights && (p->flags & APT_FLAG_NEE) != 0, gloss = (p->flags & APT_FLAG_GLOSS) != 0;
    return apt::MatTrace{ta.ns, ta.depth, ta.rr_start, ta.light, nee, ta.eps, ta.seed, ta.status ? ta.grid : nullptr, ta.status, ta.traced, lights,
                         gloss, (p->flags & APT_FLAG_MIS) != 0 && gloss && (nee || lights)};
}

// The path range [b, b + c) of a buffer-mode call (path_count 0: to the end of the image) among the image's n_image paths.  With
// APT_FLAG_BAND_BUFFERS the caller's buffers are planes of c floats holding the range only: plane() is their length either way, and
// base() shifts such a buffer so that path p sits at index p, the indexing of a whole-image buffer.
struct PathRange {
    uint64_t n_image, b, c;
    bool band;
    unsigned grid = 0;   // workgroups of one lane per path: paths_launch_range
    uint64_t plane() const { return band ? c : n_image; }
    template <class T> T *base(T *buf) const { return band ? buf - b : buf; }
};
// -> APT_OK with r.c == 0 for an empty range: the call is a no-op, the caller returns APT_OK without launching anything
int path_range(const apt_render_params *p, PathRange &r) {
    r.n_image = (uint64_t)p->width * p->height * 4u * p->samples;
    r.b = p->path_begin;
    if (r.b > r.n_image) return fail(APT_ERR_ARG, "path_begin beyond the image%s");
    r.c = p->path_count ? p->path_count : r.n_image - r.b;
    if (r.b + r.c > r.n_image) return fail(APT_ERR_ARG, "path range beyond the image%s");
    r.band = p->flags & APT_FLAG_BAND_BUFFERS;
    return APT_OK;
}
// The pixel range of a frame launch among the image's pixels.
int pixel_range(const apt_render_params *p, uint64_t pixel_begin, uint64_t pixel_count) {
    const uint64_t npix = (uint64_t)p->width * p->height;
    return (pixel_begin > npix || pixel_count > npix - pixel_begin) ? fail(APT_ERR_ARG, "pixel range beyond the image%s") : APT_OK;
}

// The pixel list of a list pass ("List passes" in the header) in the range's place: its address and its length.
int pixel_list(const apt_render_params *p, uint64_t list_address, uint64_t list_count) {
    const uint64_t npix = (uint64_t)p->width * p->height;
    if (list_address == 0 || (list_address & 3u)) return fail(APT_ERR_ARG, "pixel list: pixel_begin must carry a non-null, 4-byte aligned device address%s");
    if (list_count > npix) return fail(APT_ERR_ARG, "pixel list: more entries than the image has pixels%s");
    return npix > (1ull << 32) ? fail(APT_ERR_ARG, "pixel list: an image of more than 2^32 pixels has no 32-bit pixel indices%s") : APT_OK;
}

FrameArgs make_frame_args(const apt_render_params *p, uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    FrameArgs fa;
    camera_init(fa.cam, p->width, p->height);
    fa.width = p->width; fa.height = p->height; fa.samples = p->samples; fa.seed = p->seed;
    fa.pixel_begin = pixel_begin; fa.pixel_count = pixel_count; fa.fb = fb; fa.fb_u8 = fb_u8;
    return fa;
}

// bytes of the zero-padded [10][Ns] sphere table (a 512-byte multiple, gen_data.py:120-127)
size_t sphere_table_bytes(uint32_t num_spheres) { return ((size_t)num_spheres * 10 + 127) / 128 * 128 * sizeof(float); }

// Buffer mode takes the two-paths-per-lane kernel from this many paths on: below it the one-path kernel's twice as many workgroups fill the
// chip better (C1, the reference's own CPU-runnable configuration, is 262 144 paths = 1024 workgroups of it: launch-bound either way).
constexpr uint64_t kTwoPathBufferMin = 1ull << 20;

// What a launch of one lane per path checks after its params: pointers (`pointers`: the entry's are non-null, `which` names them), the
// path range, the size of one launch (r.grid).  -> APT_OK with r.c == 0 for an empty range, as path_range.
int paths_launch_range(const apt_render_params *p, bool pointers, PathRange &r, const char *which = "rays/spheres/colors must be non-null%s") {
    if (!pointers) return fail(APT_ERR_ARG, which);
    if (int rc = path_range(p, r); rc || r.c == 0) return rc;
    return one_launch((r.c + kBlock - 1) / kBlock, "path_count too large for one launch; shard it%s", &r.grid);
}

// The same for a frame launch: pointers (`pointers`: the entry's are non-null), the pixel range, the plan, the size of one launch.
// -> APT_OK with an all-zero fs (fs.blocks == 0) for an empty range: the call is a no-op, the caller returns APT_OK without launching
int frame_launch_shape(const apt_render_params *p, bool pointers, uint64_t pixel_begin, uint64_t pixel_count, FrameShape &fs, bool list = false) {
    if (!pointers) return fail(APT_ERR_ARG, "spheres/fb must be non-null%s");
    if (int rc = list ? pixel_list(p, pixel_begin, pixel_count) : pixel_range(p, pixel_begin, pixel_count)) return rc;
    fs = FrameShape{};
    if (pixel_count == 0) return APT_OK;
    if (!frame_shape(p->samples, pixel_count, fs)) return no_leaf_plan();
    return one_launch(fs.blocks, "pixel_count too large for one launch; shard it%s");
}

// ---- the two mirror render launches, on an explicit snapshot of a context's values ---------
int do_render_paths(const Launch &ls, const apt_render_params *p, void *stream, const float *rays,
                    const float *spheres, float *colors) {
    int rc = check_params(p);
    if (rc) return rc;
    PathRange r;
    if ((rc = paths_launch_range(p, rays && spheres && colors, r)) || r.c == 0) return rc;
    const uint64_t n = r.plane(), b = r.b, c = r.c;
    hipStream_t st = (hipStream_t)stream;
    const bool ns8 = p->num_spheres == 8;
    const TraceArgs ta = make_trace_args(p, ls);
    const bool retire = p->flags & APT_FLAG_RETIRE;
    const dim3 grid(r.grid);
    rays = r.base(rays);
    colors = r.base(colors);
    with_mode(p->mode, [&](auto m) {
        if (ns8 && !retire && ta.rr_start == 0 && c >= kTwoPathBufferMin) {   // a large range of the reference scene, every segment traced: two paths per lane
            const uint64_t per_block = 2ull * kBlock * kPaths2Pairs;
            const dim3 grid2((unsigned)((c + per_block - 1) / per_block));
            hipLaunchKernelGGL((render_paths2_kernel<m>), grid2, dim3(kBlock), 0, st, rays, spheres, colors, n, b, c, ta);
        } else if (ns8 && retire) { // wave-level queue: one wave per kQueueChunk consecutive paths
            const uint64_t waves = (c + kQueueChunk - 1) / kQueueChunk;
            const dim3 qgrid((unsigned)((waves + kBlock / 64 - 1) / (kBlock / 64)));
            hipLaunchKernelGGL((render_paths_queue_kernel<m>), qgrid, dim3(kBlock), 0, st, rays, spheres, colors, n, b, c, ta);
        } else if (ns8) {
            hipLaunchKernelGGL((render_paths_kernel<m, kScene8, false>), grid, dim3(kBlock), 0, st, rays, spheres, colors, n, b, c, ta);
        } else {
            with_flag(ta.grid != nullptr, [&](auto gr) { with_flag(retire, [&](auto rt) {
                hipLaunchKernelGGL((render_paths_kernel<m, gr ? kSceneGrid : kSceneTiles, rt>), grid, dim3(kBlock), 0, st, rays, spheres, colors, n, b, c, ta);
            }); });
        }
    });
    return launched();
}

// The sample-queue kernels' launch shape (pt_queue.h): colour buffers, pixels per wave, dynamic LDS, one wave per workgroup.
struct QueueShape { QueueArgs qa; unsigned waves; size_t lds; };
int queue_launch_shape(const apt::Debug &dbg, const LeafProg &lp, bool rr, bool grid, uint64_t pixel_count, bool retire, QueueShape &q) {
    QueueArgs &qa = q.qa;
    // a unit = one pairwise leaf of a pixel (8-sphere form) or of half a pixel (grid form); buffers for ~512 resp. ~384 items in flight
    const uint32_t subs = queue_unit_subs(grid), unit_items = subs * lp.maxleaf, window = subs == 4u ? 512u : 384u;
    qa.nbuf = dbg.queue_nbuf ? dbg.queue_nbuf : std::max(2u, std::min(16u, (window + unit_items - 1u) / unit_items));
    qa.buf_bytes = queue_buf_bytes(lp.maxleaf, subs);
    qa.retire = retire ? 1u : 0u;
    // pixels per wave: 16 at C2 (lane efficiency 0.98; 8 / 16 / 24 measured within 0.5 % of each other, 2 costs 6 %), fewer only
    // for frames too small to fill the chip's ~3800 wave slots a few times over
    const uint64_t ppw = dbg.queue_ppw ? dbg.queue_ppw : std::max<uint64_t>(4, std::min<uint64_t>(16, pixel_count / 8192u));
    qa.ppw = (uint32_t)ppw;
    q.lds = queue_lds_bytes(queue_pool_entries(grid), rr, qa.nbuf, lp.nleaves > 1, qa.buf_bytes, subs) + dbg.queue_lds_pad;   // the pad: experiments only, lowers the occupancy
    return one_launch((pixel_count + ppw - 1) / ppw, "pixel_count too large for one launch; shard it%s", &q.waves);
}

int do_render_frame(const Launch &ls, const apt_render_params *p, void *stream, const float *spheres,
                    uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    int rc = check_params(p);
    if (rc) return rc;
    FrameShape fs;
    if ((rc = frame_launch_shape(p, spheres && fb, pixel_begin, pixel_count, fs)) || fs.blocks == 0) return rc;
    const LeafProg &lp = fs.lp;
    const int group = fs.group;
    const apt::Debug &dbg = ls.cv.debug;
    if ((rc = refuse_camera(ls.cv, "render_frame"))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool ns8 = p->num_spheres == 8;
    TraceArgs ta = make_trace_args(p, ls);
    const FrameArgs fa = make_frame_args(p, pixel_begin, pixel_count, fb, fb_u8);
    const bool retire = p->flags & APT_FLAG_RETIRE, rrk = ta.rr_start != 0;
    if (retire && ns8 && group == 8 && p->depth > 0) {
        // 8-sphere scene with compaction: one wave per workgroup, a stream of `ppw` pixels per wave (pt_queue.h)
        QueueShape q;
        if ((rc = queue_launch_shape(dbg, lp, rrk, false, pixel_count, true, q))) return rc;
        with_mode(p->mode, [&](auto m) { with_flag(rrk, [&](auto rr) {
            hipLaunchKernelGGL((render_frame_queue8_kernel<m, rr>), dim3(q.waves), dim3(64), q.lds, st, spheres, fa, ta, lp, q.qa);
        }); });
        return launched();
    }
    if (!ns8 && ta.grid && group == 8 && p->depth > 0 && dbg.grid_walk != 1u) {
        // A scene behind a grid: the sample-queue kernel's grid form (pt_queue.h run_grid), with or without APT_FLAG_RETIRE.  Whether
        // the grid carries the pair-slot tables that form needs is written in the buffer on the DEVICE: rather than reading it back in
        // the launch path, both kernels are launched and each asks grid_queue_usable() -- the one not chosen returns at once.
        // (apt_set_debug("grid_walk", 1): measurement knob, the nested item walk of render_frame_kernel only.)
        QueueShape q;
        if ((rc = queue_launch_shape(dbg, lp, rrk, true, pixel_count, retire, q))) return rc;
        // APT_FLAG_GRID_SLOTS: the caller vouches for the grid (apt_grid_flags): this launch is the frame's only one, and a grid that does not
        // keep the promise is reported through the status word (grid_walk == 3 tells the kernel to report instead of returning silently)
        // (Only with a status word to report through: without one -- a context's first launch inside a stream capture, a device index beyond
        // the context's table -- a grid that breaks the promise would render nothing and say nothing, so the two-launch form is kept then.)
        const bool vouched = (p->flags & APT_FLAG_GRID_SLOTS) && eps_allows_rootkey(p->eps) && ta.status != nullptr;
        TraceArgs ta_q = ta;
        ta_q.grid_walk = vouched ? 3u : 0u;
        // (the walk statistics behind apt_set_trace_counter are a template flag: a frame without a counter does not carry them)
        with_mode(p->mode, [&](auto m) { with_flag(rrk, [&](auto rr) { with_flag(ta.traced != nullptr, [&](auto stats) {
            hipLaunchKernelGGL((render_frame_queue8_kernel<m, rr, kSceneGrid, stats>), dim3(q.waves), dim3(64), q.lds, st, spheres, fa, ta_q, lp, q.qa);
        }); }); });
        if ((rc = launched()) || vouched) return rc;
        ta.grid_walk = 2;
    }
    size_t lds = fs.lds;
    if (retire && !ns8 && !ta.grid && group == 8) lds += (size_t)(kBlock / 64) * 3 * 8 * lp.maxleaf * sizeof(float); // colour queue of the LDS-tile form
    const dim3 grid((unsigned)fs.blocks);
    with_mode(p->mode, [&](auto m) {
        if (ns8 && group == 8) {
            // With APT_FLAG_RETIRE these frames belong to the sample-queue kernel (above); what arrives here with the flag set is depth 0,
            // where there is nothing to retire.  The headline case -- >= 16 samples, every segment traced, no roulette -- runs two paths per lane.
            if (!retire && !rrk && p->samples >= 16) {
                // its first-bounce plan, made on the device in front of it (the table lives there), every call; without a record: skip nothing
                uint64_t ticket = plan_ticket(ls.status, fa.width, fa.height);
                if (ticket && !apt::launch_first_plan(st, spheres, fa.cam, fa.width, fa.height, ta.eps, ls.status, ticket)) ticket = 0;
                TraceArgs ta2 = ta;
                set_first_plan_ticket(ta2, ticket);   // (in ta.grid's slot, null for every 8-sphere launch: make_trace_args, pt_trace.h)
                hipLaunchKernelGGL((render_frame_kernel<m, kScene8, 8, false, true>), grid, dim3(kBlock), lds, st, spheres, fa, ta2, lp);
            } else {
                hipLaunchKernelGGL((render_frame_kernel<m, kScene8, 8, false>), grid, dim3(kBlock), lds, st, spheres, fa, ta, lp);
            }
        } else if (ns8) {
            with_flag(retire, [&](auto rt) {
                hipLaunchKernelGGL((render_frame_kernel<m, kScene8, 1, rt>), grid, dim3(kBlock), lds, st, spheres, fa, ta, lp);
            });
        } else {
            with_flag(ta.grid != nullptr, [&](auto gr) { with_flag(group == 8, [&](auto g8) { with_flag(retire, [&](auto rt) {
                hipLaunchKernelGGL((render_frame_kernel<m, gr ? kSceneGrid : kSceneTiles, g8 ? 8 : 1, rt>), grid, dim3(kBlock), lds, st, spheres, fa, ta, lp);
            }); }); });
        }
    });
    return launched();
}

// contiguous near-equal split of [0,total) into `parts`: part r -> (begin, count); the first total%parts get one more
void split_range(uint64_t total, uint64_t r, uint64_t parts, uint64_t &begin, uint64_t &count) {
    const uint64_t base = total / parts, extra = total % parts;
    begin = r * base + (r < extra ? r : extra);
    count = base + (r < extra ? 1 : 0);
}

// ---- the material entries (include/render_mi355x.h "per-sphere materials"): which kernels serve a call is apt_materials.h's to decide.
// check_params and check_mat_args run before the context's launch state is taken: the one place the other entries touch HIP before
// their checks.
int do_mat_paths(apt_context *ctx, const apt_render_params *p, void *stream, const float *rays, const float *spheres, const MatArgs &ma,
                 float *colors) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    int rc = check_params(p, Reads::Materials);
    if (rc || (rc = check_mat_args(p, ma))) return rc;
    const Launch ls = launch_state(*ctx, stream);
    PathRange r;
    if ((rc = paths_launch_range(p, rays && spheres && colors, r)) || r.c == 0) return rc;
    if ((rc = check_lights_status(ma, ls.status))) return rc;
    apt::mat_render_paths(apt::MatPathsCall{make_mat_trace(p, ls, ma), r.base(rays), spheres, ma.materials, r.base(colors), r.plane(), r.b, r.c,
                                            stream, ls.cv.has_env ? &ls.cv.env : nullptr});
    return launched();
}
int do_mat_frame(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres, const MatArgs &ma, uint64_t pixel_begin,
                 uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    int rc = check_params(p, Reads::Materials);
    if (rc || (rc = check_mat_args(p, ma))) return rc;
    const Launch ls = launch_state(*ctx, stream);
    const bool film = ma.film != apt::MatFilm::None;   // (its null film is refused last: by mat_render_frame)
    FrameShape fs;
    if ((rc = frame_launch_shape(p, spheres && (fb || film), pixel_begin, pixel_count, fs, ma.list)) || fs.blocks == 0) return rc;
    if ((rc = check_lights_status(ma, ls.status))) return rc;
    if ((ls.cv.has_camera || ls.cv.has_env || film) && !apt::mat_camera_fits(p->samples)) return fail(APT_ERR_ARG, "camera / environment: a frame with a camera or an environment set takes a pairwise-sum plan of at most 44 leaves (every samples <= 4199 has one)%s");
    // (a list call: the range starts at 0 and the list's address travels on its own)
    if ((rc = apt::mat_render_frame(apt::MatFrameCall{make_mat_trace(p, ls, ma), spheres, ma.materials, p->width, p->height, p->samples,
                                                      ma.list ? 0 : pixel_begin, pixel_count, fb, fb_u8, stream,
                                                      ls.cv.has_camera ? &ls.cv.camera : nullptr, ls.cv.has_env ? &ls.cv.env : nullptr, ma.film,
                                                      ma.list ? reinterpret_cast<const uint32_t *>((uintptr_t)pixel_begin) : nullptr})))
        return rc;
    return launched();
}

// The feature planes ("features" in the header).  Of the params record only what the entry reads is checked; from the pointers on,
// the refusals are do_mat_frame's for a film, in its order, so that a film and its features accept the same calls: the launch shape is
// the film's (a features launch has fewer workgroups), the last two refusals are mat_render_features'.
int do_features(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres, uint64_t pixel_begin, uint64_t pixel_count,
                float *features) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    int rc = check_params(p, Reads::Features);
    if (rc) return rc;
    if (p->accel && !(p->flags & APT_FLAG_GRID_SLOTS)) return fail(APT_ERR_ARG, "features: accel (grid) needs APT_FLAG_GRID_SLOTS (apt_grid_flags of the built grid)%s");
    const Launch ls = launch_state(*ctx, stream);
    FrameShape fs;
    if ((rc = frame_launch_shape(p, spheres != nullptr, pixel_begin, pixel_count, fs)) || fs.blocks == 0) return rc;
    if (!apt::mat_camera_fits(p->samples)) return fail(APT_ERR_ARG, "features: the frame takes a pairwise-sum plan of at most 44 leaves, as a film's does (every samples <= 4199 has one)%s");
    // the grid only with a status word to report a broken promise through, and never for the 8-sphere scene (make_mat_trace)
    const uint32_t *grid = (p->num_spheres != 8 && ls.status) ? reinterpret_cast<const uint32_t *>((uintptr_t)p->accel) : nullptr;
    if ((rc = apt::mat_render_features(apt::FeaturesCall{spheres, p->num_spheres, p->eps, p->seed, grid, ls.status, p->width, p->height, p->samples,
                                                         pixel_begin, pixel_count, features, stream, ls.cv.has_camera ? &ls.cv.camera : nullptr})))
        return rc;
    return launched();
}

} // namespace

// ---- one process, several GPUs (include/render_mi355x.h: apt_multi_*) ---------------------------
// The frame is cut into `bands * stripes` contiguous stripes of x-major pixels; band b renders stripes
// b, b+bands, b+2*bands, ... on its own device and stream, and every stripe is copied straight into the full
// framebuffer on the root device with hipMemcpyPeerAsync (xGMI: each peer has its own link to the root, so the
// copies of different bands run in parallel; no ring, no collective needed for a gather to one root).
struct apt_multi {
    struct Band {
        int device = 0;
        apt::Stream stream;
        apt::Event start, stop;
        apt::DeviceBuffer<float> sph;  // the scene table on this device
        apt::DeviceBuffer<float> fb;   // [3][max stripe] per stripe, stripes back to back
        apt::DeviceBuffer<uint8_t> u8;
    };
    std::vector<Band> bands;           // the bands set up so far
    apt_render_params params;
    uint32_t stripes = 1;
    uint64_t max_stripe = 0;
    int root = 0;
    // Sets up the next band, on `device`, which it leaves current.  What a failure leaves half made goes with the handle.
    hipError_t add_band(int device, const float *spheres_host, size_t sph_bytes) {
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) return e;
        Band &bd = bands.emplace_back();
        bd.device = device;
        int can = 0;   // let the root's copy engine read this device (no-op if already on)
        if (device != root && hipDeviceCanAccessPeer(&can, device, root) == hipSuccess && can && hipDeviceEnablePeerAccess(root, 0) != hipSuccess) (void)hipGetLastError();
        if ((e = bd.stream.create(hipStreamNonBlocking)) != hipSuccess) return e;
        if ((e = bd.start.create()) != hipSuccess || (e = bd.stop.create()) != hipSuccess) return e;
        if ((e = bd.sph.alloc(sph_bytes / sizeof(float))) != hipSuccess) return e;
        if ((e = hipMemcpy(bd.sph.get(), spheres_host, sph_bytes, hipMemcpyHostToDevice)) != hipSuccess) return e;
        if ((e = bd.fb.alloc((size_t)stripes * 3 * max_stripe)) != hipSuccess) return e;
        return bd.u8.alloc((size_t)stripes * 3 * max_stripe);
    }
    // every band's stream, events and memory go with the band's own device current; the root device is left current
    ~apt_multi() {
        apt::DeviceScope to_root(root);
        for (; !bands.empty(); bands.pop_back()) (void)hipSetDevice(bands.back().device);
    }
};

extern "C" {

int apt_abi_version(void) { return APT_ABI_VERSION; }

int apt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

// ---- contexts ---------------------------------------------------------------------------------------
apt_context *apt_context_create(void) { clear_error(); return new (std::nothrow) apt_context(); }
void apt_context_destroy(apt_context *ctx) {
    clear_error();
    if (!ctx) return;
    uint32_t *words[apt::kMaxStatusDevices];
    ctx->status_release(words);
    {
        apt::DeviceScope back;
        for (int d = 0; d < apt::kMaxStatusDevices; ++d)
            if (words[d] && hipSetDevice(d) == hipSuccess) { apt::DeviceBuffer<uint32_t> freed(words[d]); }   // with its device current
    }
    (void)hipGetLastError();
    delete ctx;
}

int apt_context_set_debug(apt_context *ctx, const char *key, double value) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    return ctx->set_debug(key, value);
}

int apt_context_get_debug(apt_context *ctx, const char *key, double *value) {
    clear_error();
    if (!ctx || !value) return fail(APT_ERR_ARG, "context/value is null%s");
    return ctx->get_debug(key, value);
}

// Reads and clears the status word of the current device (see the header).  Synchronises `stream` first.
int apt_context_check(apt_context *ctx, void *stream) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    uint32_t *w = status_word(*ctx, (hipStream_t)stream);
    if (!w) return APT_OK;                       // no word could be made: nothing was ever reported into it
    uint32_t bits = 0;
    HIP_TRY(hipMemcpy(&bits, w, sizeof bits, hipMemcpyDeviceToHost));
    if (!bits) return APT_OK;
    if (hipMemset(w, 0, sizeof bits) != hipSuccess) (void)hipGetLastError();
    std::string what;
    if (bits & APT_DEV_QUEUE_GUARD) what += " queue-loop-bound";
    if (bits & APT_DEV_GRID_TURNS) what += " grid-walk-bound";
    if (bits & APT_DEV_LDS_BASE) what += " lds-base";
    if (bits & APT_DEV_GRID_MISMATCH) what += " grid-mismatch";
    if (bits & APT_DEV_BAD_MATERIAL) what += " bad-material";
    if (bits & APT_DEV_LIGHTS_MISMATCH) what += " lights-mismatch";
    if (bits & APT_DEV_LIST_RANGE) what += " list-range";
    if (bits & ~(uint32_t)(APT_DEV_QUEUE_GUARD | APT_DEV_GRID_TURNS | APT_DEV_LDS_BASE | APT_DEV_GRID_MISMATCH | APT_DEV_BAD_MATERIAL | APT_DEV_LIGHTS_MISMATCH | APT_DEV_LIST_RANGE)) what += " unknown-bits";
    return fail(APT_ERR_DEVICE, "a kernel reported a failure through the device status word:%s (the frame it wrote is incomplete)", what.c_str());
}

int apt_context_set_params(apt_context *ctx, const apt_render_params *p) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    int rc = check_params(p);
    if (rc) return rc;
    ctx->set_params(*p);
    return APT_OK;
}

int apt_context_set_trace_counter(apt_context *ctx, uint64_t *device_counter) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    ctx->set_trace_counter((unsigned long long *)device_counter);
    return APT_OK;
}

int apt_context_set_refill_lanes(apt_context *ctx, uint32_t lanes) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    if (lanes < 1 || lanes > 64) return fail(APT_ERR_ARG, "refill lanes: 1..64%s");
    ctx->set_refill_lanes(lanes);
    return APT_OK;
}

void apt_context_render_do(apt_context *ctx, uint32_t blockDim, void *l2ctrl, void *stream, uint8_t *rays,
                           uint8_t *spheres, uint8_t *colors) {
    clear_error();
    (void)blockDim; // the reference's 8-way partition (render.cpp:9-10,24): results do not depend on it
    (void)l2ctrl;
    if (!ctx) { (void)fail(APT_ERR_ARG, "context is null%s"); return; }
    const Launch ls = launch_state(*ctx, stream);
    (void)do_render_paths(ls, &ls.cv.params, stream, (const float *)rays, (const float *)spheres, (float *)colors);
}

int apt_context_render_do_ex(apt_context *ctx, const apt_render_params *p, void *stream, const float *rays,
                             const float *spheres, float *colors) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    return do_render_paths(launch_state(*ctx, stream), p, stream, rays, spheres, colors);
}

int apt_context_render_frame(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                             uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    clear_error();
    if (!ctx) return fail(APT_ERR_ARG, "context is null%s");
    return do_render_frame(launch_state(*ctx, stream), p, stream, spheres, pixel_begin, pixel_count, fb, fb_u8);
}

// Per-sphere materials: do_mat_frame, do_mat_paths.
int apt_context_render_frame_materials(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                                       const uint32_t *materials, uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    return do_mat_frame(ctx, p, stream, spheres, MatArgs{materials}, pixel_begin, pixel_count, fb, fb_u8);
}

int apt_context_render_paths_materials(apt_context *ctx, const apt_render_params *p, void *stream, const float *rays,
                                       const float *spheres, const uint32_t *materials, float *colors) {
    return do_mat_paths(ctx, p, stream, rays, spheres, MatArgs{materials}, colors);
}

int apt_render_frame_materials(const apt_render_params *p, void *stream, const float *spheres, const uint32_t *materials,
                               uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    return apt_context_render_frame_materials(&apt::default_context(), p, stream, spheres, materials, pixel_begin, pixel_count, fb, fb_u8);
}

int apt_render_paths_materials(const apt_render_params *p, void *stream, const float *rays, const float *spheres,
                               const uint32_t *materials, float *colors) {
    return apt_context_render_paths_materials(&apt::default_context(), p, stream, rays, spheres, materials, colors);
}

// The material entries with a light table ("several lights" in the header): the same checks, then lights == NULL.
int apt_context_render_frame_lights(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                                    const uint32_t *materials, const void *lights, uint64_t pixel_begin, uint64_t pixel_count, float *fb,
                                    uint8_t *fb_u8) {
    return do_mat_frame(ctx, p, stream, spheres, MatArgs{materials, true, lights}, pixel_begin, pixel_count, fb, fb_u8);
}

int apt_context_render_paths_lights(apt_context *ctx, const apt_render_params *p, void *stream, const float *rays, const float *spheres,
                                    const uint32_t *materials, const void *lights, float *colors) {
    return do_mat_paths(ctx, p, stream, rays, spheres, MatArgs{materials, true, lights}, colors);
}

// The film entries ("film" in the header): the frame entry the caller's `lights` selects, rendered with the pass's seed into a film.
int apt_context_render_frame_film(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres,
                                  const uint32_t *materials, const void *lights, uint64_t pixel_begin, uint64_t pixel_count, float *film,
                                  uint32_t pass) {
    // APT_FLAG_PIXEL_LIST ("List passes" in the header): the launch stores whatever `pass` is, which then only selects the seed
    const bool list = p && p->struct_size == sizeof(apt_render_params) && (p->flags & APT_FLAG_PIXEL_LIST) != 0;
    const MatArgs ma{materials, lights != nullptr, lights, pass && !list ? apt::MatFilm::Add : apt::MatFilm::Store, list};
    apt_render_params q;
    if (p && p->struct_size == sizeof q) {   // (anything else is check_params' to refuse)
        q = *p;
        q.seed = apt_film_pass_seed(p->seed, pass);
        p = &q;
    }
    return do_mat_frame(ctx, p, stream, spheres, ma, pixel_begin, pixel_count, film, nullptr);
}

int apt_render_frame_film(const apt_render_params *p, void *stream, const float *spheres, const uint32_t *materials, const void *lights,
                          uint64_t pixel_begin, uint64_t pixel_count, float *film, uint32_t pass) {
    return apt_context_render_frame_film(&apt::default_context(), p, stream, spheres, materials, lights, pixel_begin, pixel_count, film, pass);
}

// The feature planes ("features" in the header): do_features.
int apt_context_render_frame_features(apt_context *ctx, const apt_render_params *p, void *stream, const float *spheres, uint64_t pixel_begin,
                                      uint64_t pixel_count, float *features) {
    return do_features(ctx, p, stream, spheres, pixel_begin, pixel_count, features);
}

int apt_render_frame_features(const apt_render_params *p, void *stream, const float *spheres, uint64_t pixel_begin, uint64_t pixel_count,
                              float *features) {
    return do_features(&apt::default_context(), p, stream, spheres, pixel_begin, pixel_count, features);
}

int apt_film_resolve_device(const apt_film_resolve *r, void *stream, const float *film, uint64_t pixel_count, const float *table_dev,
                            float *out, uint8_t *u8) {
    clear_error();
    int rc = apt::film_resolve_check(r, film, table_dev, out, u8, "apt_film_resolve_device");
    if (rc || pixel_count == 0) return rc;
    if ((rc = one_launch((pixel_count + kBlock - 1) / kBlock, "pixel_count too large for one launch; shard it%s"))) return rc;
    apt::film_resolve(*r, stream, film, pixel_count, table_dev, out, u8);
    return launched();
}

int apt_render_frame_lights(const apt_render_params *p, void *stream, const float *spheres, const uint32_t *materials, const void *lights,
                            uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    return apt_context_render_frame_lights(&apt::default_context(), p, stream, spheres, materials, lights, pixel_begin, pixel_count, fb, fb_u8);
}

int apt_render_paths_lights(const apt_render_params *p, void *stream, const float *rays, const float *spheres, const uint32_t *materials,
                            const void *lights, float *colors) {
    return apt_context_render_paths_lights(&apt::default_context(), p, stream, rays, spheres, materials, lights, colors);
}

// ---- the context-free forms: the process-wide default context -----------------------------------------
int apt_set_default_params(const apt_render_params *p) { return apt_context_set_params(&apt::default_context(), p); }
int apt_set_refill_lanes(uint32_t lanes) { return apt_context_set_refill_lanes(&apt::default_context(), lanes); }
int apt_set_trace_counter(uint64_t *device_counter) { return apt_context_set_trace_counter(&apt::default_context(), device_counter); }
int apt_set_debug(const char *key, double value) { return apt_context_set_debug(&apt::default_context(), key, value); }
int apt_get_debug(const char *key, double *value) { return apt_context_get_debug(&apt::default_context(), key, value); }
int apt_check(void *stream) { return apt_context_check(&apt::default_context(), stream); }

int render_do_ex(const apt_render_params *p, void *stream, const float *rays, const float *spheres, float *colors) {
    return apt_context_render_do_ex(&apt::default_context(), p, stream, rays, spheres, colors);
}

void render_do(uint32_t blockDim, void *l2ctrl, void *stream, uint8_t *rays, uint8_t *spheres, uint8_t *colors) {
    apt_context_render_do(&apt::default_context(), blockDim, l2ctrl, stream, rays, spheres, colors);
}

// The same function under a name a C++ translation unit can bind next to its own C++-linkage render_do
// (render_do_cxx.cpp: the reference declares render_do WITHOUT extern "C", src/main.cpp:9-10).
void apt_render_do(uint32_t blockDim, void *l2ctrl, void *stream, uint8_t *rays, uint8_t *spheres, uint8_t *colors) {
    apt_context_render_do(&apt::default_context(), blockDim, l2ctrl, stream, rays, spheres, colors);
}

int render_frame(const apt_render_params *p, void *stream, const float *spheres, uint64_t pixel_begin,
                 uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    return apt_context_render_frame(&apt::default_context(), p, stream, spheres, pixel_begin, pixel_count, fb, fb_u8);
}

// The CPU-simulator shape of the boundary (src/main.cpp:21-44: ICPU_RUN_KF(render, blockDim, rays, spheres,
// colors) on HOST buffers, synchronous): copies in, renders with the default context's parameters, copies out.
int apt_render_host(uint32_t blockDim, const uint8_t *rays, const uint8_t *spheres, uint8_t *colors) {
    clear_error();
    if (!rays || !spheres || !colors) return fail(APT_ERR_ARG, "rays/spheres/colors must be non-null%s");
    const Launch ls = launch_state(apt::default_context(), nullptr);
    const apt_render_params &p = ls.cv.params;
    const size_t n = (size_t)p.width * p.height * 4u * p.samples;
    // The reference's call renders the whole ray array (src/main.cpp:18-25); with a STRICT path sub-range in the default parameters the
    // colours outside it would be copied back from memory no kernel wrote.  (path_begin 0 with path_count 0 or N is the whole frame.)
    if (p.path_begin != 0 || (p.path_count != 0 && p.path_count != n)) return fail(APT_ERR_ARG, "apt_render_host: the default parameters carry a path sub-range; it renders whole frames only%s");
    const size_t sph_bytes = sphere_table_bytes(p.num_spheres);
    apt::DeviceBuffer<float> d_rays, d_sph, d_col;
    HIP_TRY(d_rays.alloc(n * 6)); HIP_TRY(d_sph.alloc(sph_bytes / sizeof(float))); HIP_TRY(d_col.alloc(n * 3));
    HIP_TRY(hipMemcpy(d_rays.get(), rays, n * 24, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_sph.get(), spheres, sph_bytes, hipMemcpyHostToDevice));
    (void)blockDim;
    if (int rc = do_render_paths(ls, &p, nullptr, d_rays.get(), d_sph.get(), d_col.get())) return rc;
    HIP_TRY(hipMemcpy(colors, d_col.get(), n * 12, hipMemcpyDeviceToHost)); // synchronises the null stream
    return apt_context_check(&apt::default_context(), nullptr);   // a kernel may have reported a failure (clears and sets the error record itself)
}

// ---- one process, several GPUs ---------------------------------------------------------------------------
void apt_multi_destroy(apt_multi *m) { clear_error(); delete m; }

int apt_multi_create(const int *device_ids, uint32_t num_bands, uint32_t stripes, const apt_render_params *p,
                     const float *spheres_host, apt_multi **out) {
    clear_error();
    if (!device_ids || !num_bands || !stripes || !spheres_host || !out) return fail(APT_ERR_ARG, "apt_multi_create: bad arguments%s");
    int rc = check_params(p);
    if (rc) return rc;
    if (p->accel) return fail(APT_ERR_ARG, "apt_multi_create: accel is a single-device address; not supported here%s");
    if ((rc = refuse_camera(apt::default_context().snapshot(), "apt_multi_create"))) return rc;   // apt_multi_render renders through the default context
    const int ndev = apt_device_count();
    for (uint32_t b = 0; b < num_bands; ++b)
        if (device_ids[b] < 0 || device_ids[b] >= ndev) return fail(APT_ERR_DEVICE, "apt_multi_create: device id out of range%s");
    const uint64_t npix = (uint64_t)p->width * p->height, parts = (uint64_t)num_bands * stripes;
    if (parts > npix) return fail(APT_ERR_ARG, "apt_multi_create: more stripes than pixels%s");
    apt_multi *m = new (std::nothrow) apt_multi();
    if (!m) return fail(APT_ERR_DEVICE, "out of host memory%s");
    m->params = *p; m->stripes = stripes; m->root = device_ids[0];
    uint64_t b0, c0;
    split_range(npix, 0, parts, b0, c0);
    m->max_stripe = c0;
    m->bands.reserve(num_bands);
    const size_t sph_bytes = sphere_table_bytes(p->num_spheres);
    hipError_t e = hipSuccess;
    {
        apt::DeviceScope to_root(m->root);
        for (uint32_t b = 0; b < num_bands && e == hipSuccess; ++b) e = m->add_band(device_ids[b], spheres_host, sph_bytes);
    }
    if (e != hipSuccess) { delete m; return fail(APT_ERR_DEVICE, "apt_multi_create: HIP: %s", hipGetErrorString(e)); }
    *out = m;
    return APT_OK;
}

int apt_multi_render(apt_multi *m, float *fb_root, uint8_t *u8_root, float *band_kernel_ms) {
    clear_error();
    if (!m || !fb_root) return fail(APT_ERR_ARG, "apt_multi_render: handle/fb must be non-null%s");
    if (int crc = refuse_camera(apt::default_context().snapshot(), "apt_multi_render")) return crc;
    const uint64_t npix = (uint64_t)m->params.width * m->params.height;
    const uint64_t nb = m->bands.size(), parts = nb * m->stripes;
    int rc = APT_OK;
    hipError_t e = hipSuccess;
    apt::DeviceScope to_root(m->root);
    for (uint64_t b = 0; b < nb && rc == APT_OK && e == hipSuccess; ++b) {
        apt_multi::Band &bd = m->bands[b];
        e = hipSetDevice(bd.device);
        if (e != hipSuccess) break;
        Launch ls = launch_state(apt::default_context(), bd.stream.get());   // (the status word is per device: taken with the band's device current)
        // the statistics block of the default context is an address on ITS device: only bands on the root device may count into it
        if (bd.device != m->root) ls.cv.trace_counter = nullptr;
        e = hipEventRecord(bd.start.get(), bd.stream.get());
        for (uint32_t s = 0; s < m->stripes && rc == APT_OK && e == hipSuccess; ++s) {
            uint64_t begin, count;
            split_range(npix, (uint64_t)s * nb + b, parts, begin, count);   // interleaved: stripe s*nb + b belongs to band b
            float *fb = bd.fb.get() + (size_t)s * 3 * m->max_stripe;
            uint8_t *u8 = bd.u8.get() + (size_t)s * 3 * m->max_stripe;
            rc = do_render_frame(ls, &m->params, bd.stream.get(), bd.sph.get(), begin, count, fb, u8_root ? u8 : nullptr);
            if (rc != APT_OK) break;
            if (s + 1 == m->stripes) e = hipEventRecord(bd.stop.get(), bd.stream.get());  // kernels only: the copies follow
        }
        for (uint32_t s = 0; s < m->stripes && rc == APT_OK && e == hipSuccess; ++s) {
            uint64_t begin, count;
            split_range(npix, (uint64_t)s * nb + b, parts, begin, count);
            const float *fb = bd.fb.get() + (size_t)s * 3 * m->max_stripe;
            const uint8_t *u8 = bd.u8.get() + (size_t)s * 3 * m->max_stripe;
            for (int ch = 0; ch < 3 && e == hipSuccess; ++ch)   // band-local planes [3][count] -> planes of the full frame
                e = hipMemcpyPeerAsync(fb_root + (size_t)ch * npix + begin, m->root, fb + (size_t)ch * count, bd.device,
                                       count * sizeof(float), bd.stream.get());
            if (u8_root && e == hipSuccess)
                e = hipMemcpyPeerAsync(u8_root + begin * 3, m->root, u8, bd.device, count * 3, bd.stream.get());
        }
    }
    for (auto &bd : m->bands)   // wait for every band (also after an error: nothing may still be writing)
        if (hipSetDevice(bd.device) == hipSuccess) { hipError_t se = hipStreamSynchronize(bd.stream.get()); if (e == hipSuccess) e = se; }
    if (band_kernel_ms && rc == APT_OK && e == hipSuccess)
        for (uint64_t b = 0; b < nb; ++b) {
            (void)hipSetDevice(m->bands[b].device);
            if (hipEventElapsedTime(&band_kernel_ms[b], m->bands[b].start.get(), m->bands[b].stop.get()) != hipSuccess) band_kernel_ms[b] = -1.0f;
        }
    int dev_rc = APT_OK;
    std::string dev_msg;
    if (rc == APT_OK && e == hipSuccess)   // the device status words of every device that rendered (each check clears its word)
        for (auto &bd : m->bands)
            if (hipSetDevice(bd.device) == hipSuccess && apt_context_check(&apt::default_context(), bd.stream.get()) != APT_OK && dev_rc == APT_OK) {
                dev_rc = apt_last_status();
                dev_msg = apt_last_error();
            }
    if (rc != APT_OK) return rc;             // (the error record still describes the launch that failed: no check ran after it)
    if (e != hipSuccess) return hip_fail(e);
    return dev_rc == APT_OK ? APT_OK : fail(dev_rc, "apt_multi_render: %s", dev_msg.c_str());
}

int apt_build_grid_device(const float *spheres_dev, uint32_t ns, void *stream, void *grid_dev, size_t capacity,
                          size_t *out_bytes) {
    clear_error();
    if (!spheres_dev || ns == 0 || !out_bytes) return fail(APT_ERR_ARG, "apt_build_grid_device: spheres/out_bytes must be non-null, num_spheres non-zero%s");
    hipStream_t st = (hipStream_t)stream;
    // The workspace (a build step, not a render call) is released on return: after the stream's last synchronise, or on a failure path
    // by a release that itself waits for the device.
    apt::DeviceBuffer<float> rad;
    apt::DeviceBuffer<uint32_t> large, small, count, cursor, sums, long_count;
    apt::DeviceBuffer<uint2> long_cells;
    apt::DeviceBuffer<GridBuildStats> stats_d;
    // classify: radii, the two ordered lists, statistics
    HIP_TRY(rad.alloc(ns)); HIP_TRY(large.alloc(ns)); HIP_TRY(small.alloc(ns)); HIP_TRY(stats_d.alloc(1));
    hipLaunchKernelGGL(grid_classify_kernel, dim3(1), dim3(kGB), 0, st, spheres_dev, ns, rad.get(), large.get(), small.get(), stats_d.get());
    GridBuildStats stt;
    HIP_TRY(hipMemcpyAsync(&stt, stats_d.get(), sizeof stt, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    GridHeader h;   // header
    grid_header_from_stats(ns, stt.nsmall, stt.nlarge, stt.lo, stt.hi, stt.scale, apt::grid_spheres_per_cell(), h);
    // count and scan: where each cell's list starts, and the item count
    const uint64_t nc1 = (uint64_t)h.ncells + 1, nblk = (nc1 + kGB - 1) / kGB;
    HIP_TRY(count.alloc(nc1)); HIP_TRY(cursor.alloc(h.ncells)); HIP_TRY(sums.alloc(nblk));
    HIP_TRY(hipMemsetAsync(count.get(), 0, nc1 * 4, st)); HIP_TRY(hipMemsetAsync(cursor.get(), 0, (size_t)h.ncells * 4, st));
    if (stt.nsmall) hipLaunchKernelGGL(grid_count_kernel, dim3((stt.nsmall + 255) / 256), dim3(256), 0, st, h, spheres_dev, rad.get(), small.get(), stt.nsmall, count.get());
    hipLaunchKernelGGL(scan_blocks_kernel, dim3((unsigned)nblk), dim3(kGB), 0, st, count.get(), nc1, sums.get());
    hipLaunchKernelGGL(scan_sums_kernel, dim3(1), dim3(kGB), 0, st, sums.get(), (uint32_t)nblk);
    hipLaunchKernelGGL(scan_add_kernel, dim3((unsigned)nblk), dim3(kGB), 0, st, count.get(), nc1, sums.get());
    uint32_t nitems = 0;
    HIP_TRY(hipMemcpyAsync(&nitems, count.get() + h.ncells, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const size_t words = grid_header_offsets(h, nitems);
    *out_bytes = words * 4;
    if (!grid_dev) return APT_OK;                                             // size query
    if (capacity < words * 4) return fail(APT_ERR_ARG, "apt_build_grid_device: capacity too small (see *out_bytes)%s");
    uint32_t *w = (uint32_t *)grid_dev;   // fill
    HIP_TRY(hipMemsetAsync(w, 0, words * 4, st));
    HIP_TRY(hipMemcpyAsync(w, &h, sizeof h, hipMemcpyHostToDevice, st));
    if (h.nlarge) HIP_TRY(hipMemcpyAsync(w + h.off_large, large.get(), (size_t)h.nlarge * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(w + h.off_cells, count.get(), nc1 * 4, hipMemcpyDeviceToDevice, st));
    if (stt.nsmall) hipLaunchKernelGGL(grid_fill_kernel, dim3((stt.nsmall + 255) / 256), dim3(256), 0, st, h, spheres_dev, rad.get(), small.get(), stt.nsmall, count.get(), cursor.get(), w + h.off_items);
    // sort: short cell lists on the device, long ones (clustered scenes) reported and sorted here
    HIP_TRY(long_cells.alloc(nitems / (kGridSortInline + 1u) + 1u)); HIP_TRY(long_count.alloc(1));
    HIP_TRY(hipMemsetAsync(long_count.get(), 0, 4, st));
    hipLaunchKernelGGL(grid_sort_cells_kernel, dim3((h.ncells + 255) / 256), dim3(256), 0, st, h.ncells, count.get(), w + h.off_items, long_count.get(), long_cells.get());
    uint32_t nlong = 0;
    HIP_TRY(hipMemcpyAsync(&nlong, long_count.get(), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (nlong) {
        std::vector<uint2> cells(nlong);
        std::vector<uint32_t> host_items(nitems);
        HIP_TRY(hipMemcpy(cells.data(), long_cells.get(), (size_t)nlong * sizeof(uint2), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(host_items.data(), w + h.off_items, (size_t)nitems * 4, hipMemcpyDeviceToHost));
        for (const uint2 &c : cells) std::sort(host_items.begin() + c.x, host_items.begin() + c.y);
        // only the long cells go back: the short ones were sorted in place by the kernel above (the copy out saw them sorted already)
        HIP_TRY(hipMemcpy(w + h.off_items, host_items.data(), (size_t)nitems * 4, hipMemcpyHostToDevice));
    }
    const uint32_t ng = ns > nitems ? ns : nitems;   // geometry, pair slots
    hipLaunchKernelGGL(grid_geom_kernel, dim3((ng + 255) / 256), dim3(256), 0, st, spheres_dev, ns, w + h.off_items, nitems,
                       reinterpret_cast<float4 *>(w + h.off_geom), reinterpret_cast<float4 *>(w + h.off_item_geom));
    if (h.off_cellslot) hipLaunchKernelGGL(grid_slots_kernel, dim3((std::max(apt::grid_bordered_cells(h.n) + 1u, ns) + 255u) / 256u), dim3(256), 0, st, w, h, spheres_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return APT_OK;
}

int apt_selftest_sqrt(int variant, void *stream, uint64_t first_bits, uint64_t count, uint64_t *device_result2) {
    clear_error();
    if (!device_result2 || variant < 0 || variant > 3) return fail(APT_ERR_ARG, "apt_selftest_sqrt: bad arguments%s");
    if (first_bits + count > (1ull << 32)) return fail(APT_ERR_ARG, "apt_selftest_sqrt: range beyond 2^32%s");
    if (count == 0) return APT_OK;
    hipLaunchKernelGGL(selftest_sqrt_kernel, dim3(256 * 16), dim3(kBlock), 0, (hipStream_t)stream, variant, first_bits,
                       count, (unsigned long long *)device_result2);
    return launched();
}

int apt_selftest_div3(void *stream, uint64_t first, uint64_t count, uint64_t *device_result3) {
    clear_error();
    if (!device_result3) return fail(APT_ERR_ARG, "apt_selftest_div3: bad arguments%s");
    if (count == 0) return APT_OK;
    hipLaunchKernelGGL(selftest_div3_kernel, dim3(256 * 16), dim3(kBlock), 0, (hipStream_t)stream, first, count,
                       (unsigned long long *)device_result3);
    return launched();
}

int apt_selftest_direction(void *stream, const double *d3, uint64_t count, uint64_t *device_result5, uint8_t *device_flags) {
    clear_error();
    if (!d3 || !device_result5) return fail(APT_ERR_ARG, "apt_selftest_direction: bad arguments%s");
    if (count == 0) return APT_OK;
    apt::selftest_direction(stream, d3, count, device_result5, device_flags);
    return launched();
}

int apt_test_scene(const apt_render_params *p, void *stream, const float *rays, const float *spheres, float *out) {
    clear_error();
    int rc = check_params(p);
    if (rc) return rc;
    if (!rays || !spheres || !out) return fail(APT_ERR_ARG, "rays/spheres/out must be non-null%s");
    const uint64_t n = (uint64_t)p->width * p->height * 4u * p->samples;
    unsigned blocks;
    if ((rc = one_launch((n + kBlock - 1) / kBlock, "image too large for one launch%s", &blocks))) return rc;
    hipLaunchKernelGGL(test_scene_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, rays, spheres,
                       out, n, p->num_spheres, p->light_index, p->eps);
    return launched();
}

int apt_gen_rays_device(const apt_render_params *p, void *stream, float *rays) {
    clear_error();
    int rc = check_params(p);
    if (rc) return rc;
    PathRange r;
    if ((rc = paths_launch_range(p, rays != nullptr, r, "rays must be non-null%s")) || r.c == 0) return rc;
    Camera cam;
    camera_init(cam, p->width, p->height);
    hipLaunchKernelGGL(gen_rays_kernel, dim3(r.grid), dim3(kBlock), 0, (hipStream_t)stream, cam, p->width,
                       p->height, p->samples, p->seed, r.plane(), r.b, r.c, r.base(rays));
    return launched();
}

int apt_gen_rays_camera_device(const apt_render_params *p, const apt_camera *cam, void *stream, float *rays) {
    clear_error();
    int rc = check_params(p);
    if (rc) return rc;
    if ((rc = apt_camera_check_host(cam))) return rc;      // (clears and sets the error record itself)
    PathRange r;
    if ((rc = paths_launch_range(p, rays != nullptr, r, "rays must be non-null%s")) || r.c == 0) return rc;
    apt::mat_gen_rays_camera(apt::CamRaysCall{cam, p->width, p->height, p->samples, p->seed, r.base(rays), r.plane(), r.b, r.c, stream});
    return launched();
}

int apt_gen_rays_mt_device_ex(const apt_render_params *p, void *stream, const uint32_t *checkpoints, uint32_t stride,
                              uint64_t num_checkpoints, uint64_t first_block, float *rays) {
    clear_error();
    int rc = check_params(p);
    if (rc) return rc;
    if (!rays || !checkpoints || stride == 0) return fail(APT_ERR_ARG, "rays/checkpoints must be non-null, stride > 0%s");
    PathRange r;
    if ((rc = path_range(p, r)) || r.c == 0) return rc;
    const uint64_t b = r.b, c = r.c;
    const uint64_t num_blocks = (r.n_image + kPathsPerBlock - 1) / kPathsPerBlock;   // of the whole stream
    const uint64_t blk_lo = b / kPathsPerBlock, blk_hi = (b + c + kPathsPerBlock - 1) / kPathsPerBlock; // blocks the range touches
    if (blk_lo < first_block) return fail(APT_ERR_ARG, "path range starts before the checkpoint window%s");
    const uint64_t cp_lo = (blk_lo - first_block) / stride, cp_hi = (blk_hi - first_block + stride - 1) / stride;
    if (cp_hi > num_checkpoints) return fail(APT_ERR_ARG, "not enough MT19937 checkpoints for this path range%s");
    unsigned grid;
    if ((rc = one_launch(cp_hi - cp_lo, "too many checkpoints for one launch%s", &grid))) return rc;
    Camera cam;
    camera_init(cam, p->width, p->height);
    // one workgroup per checkpoint the range touches (workgroups of untouched checkpoints would only skip)
    hipLaunchKernelGGL(gen_rays_mt_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)stream,
                       checkpoints + cp_lo * kMtN, stride, first_block + cp_lo * stride, num_blocks, cam, p->width, p->height,
                       p->samples, r.plane(), b, b + c, r.base(rays));
    return launched();
}

int apt_gen_rays_mt_device(const apt_render_params *p, void *stream, const uint32_t *checkpoints, uint32_t stride,
                           uint64_t num_checkpoints, float *rays) {
    return apt_gen_rays_mt_device_ex(p, stream, checkpoints, stride, num_checkpoints, 0, rays);
}

int apt_render_frame_mt(const apt_render_params *p, void *stream, const uint32_t *checkpoints, uint64_t num_checkpoints,
                        uint64_t first_group, const float *spheres, uint64_t pixel_begin, uint64_t pixel_count, float *fb, uint8_t *fb_u8) {
    clear_error();
    int rc = check_params(p);
    if (rc) return rc;
    if (!checkpoints || !spheres || !fb) return fail(APT_ERR_ARG, "apt_render_frame_mt: checkpoints/spheres/fb must be non-null%s");
    if (p->num_spheres != 8) return fail(APT_ERR_SCENE, "apt_render_frame_mt: the 8-sphere scene only%s");
    if (p->flags & APT_FLAG_RR) return fail(APT_ERR_ARG, "apt_render_frame_mt: APT_FLAG_RR is not part of the reference's pipeline%s");
    uint32_t log2_s = 0;
    while ((1u << log2_s) < p->samples) ++log2_s;
    // 78 pixels are 2 * samples generator blocks for every sample count; samples in {8, 16, ..., 256} take the kernel whose sums are a
    // fixed 24 lanes per run, every other count (1, 2, 4 -- the reference's default is 1 --, non-powers of two, > 256) the general one
    const bool pow2_kernel = (1u << log2_s) == p->samples && p->samples >= 8 && p->samples <= 256;
    LeafProg lp;
    if ((rc = make_leaf_prog(p->samples, lp))) return rc;
    if ((rc = pixel_range(p, pixel_begin, pixel_count)) || pixel_count == 0) return rc;
    const uint64_t g_lo = pixel_begin / kMtGroupPixels, g_hi = (pixel_begin + pixel_count + kMtGroupPixels - 1) / kMtGroupPixels;
    if (g_lo < first_group || g_hi - first_group > num_checkpoints) return fail(APT_ERR_ARG, "apt_render_frame_mt: the checkpoint table does not cover the pixel range%s");
    unsigned groups;
    if ((rc = one_launch(g_hi - g_lo, "pixel_count too large for one launch; shard it%s", &groups))) return rc;
    if ((rc = refuse_camera(apt::default_context().snapshot(), "apt_render_frame_mt"))) return rc;
    const TraceArgs ta = make_trace_args(p, launch_state(apt::default_context(), stream));
    const FrameArgs fa = make_frame_args(p, pixel_begin, pixel_count, fb, fb_u8);
    MtFrameArgs ma;
    ma.checkpoints = checkpoints + (g_lo - first_group) * 624; ma.first_group = g_lo; ma.log2_s = log2_s;
    const dim3 grid(groups);
    hipStream_t st = (hipStream_t)stream;
    with_mode(p->mode, [&](auto m) {
        if (pow2_kernel) hipLaunchKernelGGL((render_frame_mt_kernel<m>), grid, dim3(kBlock), 0, st, spheres, fa, ta, ma);
        else hipLaunchKernelGGL((render_frame_mt_any_kernel<m>), grid, dim3(kBlock), 0, st, spheres, fa, ta, ma, lp);
    });
    return launched();
}

int apt_decode_color_band(const apt_render_params *p, void *stream, const float *colors, uint64_t pixel_count, float *fb,
                          uint8_t *fb_u8) {
    clear_error();
    int rc = check_params(p);
    if (rc) return rc;
    if (!colors || !fb) return fail(APT_ERR_ARG, "colors/fb must be non-null%s");
    if (pixel_count == 0) return APT_OK;
    LeafProg lp;
    if ((rc = make_leaf_prog(p->samples, lp))) return rc;
    const uint64_t npix = pixel_count;                    // the band is decoded like an image of pixel_count pixels
    const bool wide = p->samples >= 8;                    // 8 lanes per sub-pixel row: coalesced loads
    // few samples: 2 lanes per row with float4 loads (decode_color_kernel4); every row then starts at a multiple of 16 bytes from `colors`.
    // decode_color_kernel4 adds ONE leaf and relies on lp.nleaves == 1 (which every count <= 128 has)
    const bool quad = wide && p->samples <= 8u * kDecode4Blocks && lp.nleaves == 1 && p->samples % 4 == 0 && ((uintptr_t)colors & 15u) == 0;
    const uint64_t lanes = npix * 3 * 4 * (quad ? 2 : (wide ? 8 : 1));
    unsigned blocks;
    if ((rc = one_launch((lanes + kBlock - 1) / kBlock, "band too large for one launch%s", &blocks))) return rc;
    // grid caps measured on the C2 buffer (profiles/microbench/decode_rates.hip): 8-lane form 4.9 / 5.4 / 6.1 / 5.5 TB/s at 256 x 64 / 256 / 1024 /
    // one round for S = 64 (S = 256: 5.1 / 5.5 / 5.6 / 5.7; below 64 samples the smaller grid wins); float4 form 4.3 / 6.1 / 4.6 TB/s at S = 8 / 16 / 32 with its cap of 256 x 256 (8-lane form: 1.2 / 2.3 / 4.1)
    if (quad)
        hipLaunchKernelGGL(decode_color_kernel4, dim3(std::min(blocks, 256u * 256u)), dim3(kBlock), 0, (hipStream_t)stream, colors,
                           p->samples, npix, lp, fb, fb_u8);
    else if (wide)
        hipLaunchKernelGGL(decode_color_kernel8, dim3(std::min(blocks, p->samples >= 64 ? 256u * 1024u : 256u * 256u)), dim3(kBlock), 0, (hipStream_t)stream, colors,
                           p->samples, npix, lp, fb, fb_u8);
    else
        hipLaunchKernelGGL(decode_color_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, colors,
                           p->samples, npix, lp, fb, fb_u8);
    return launched();
}

int apt_decode_color_device(const apt_render_params *p, void *stream, const float *colors, float *fb, uint8_t *fb_u8) {
    clear_error();
    if (!p) return fail(APT_ERR_ARG, "params is null%s");
    return apt_decode_color_band(p, stream, colors, (uint64_t)p->width * p->height, fb, fb_u8);
}

} // extern "C"

