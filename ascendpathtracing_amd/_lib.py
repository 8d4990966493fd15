"""ctypes binding of librender_mi355x.so (include/render_mi355x.h).  Loading fails loudly:
there is no Python or CPU fallback for the compute path."""
import ctypes
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# APT_LIB_PATH: another build of the same library (A/B timing of kernel variants); still no fallback
LIB_PATH = os.environ.get("APT_LIB_PATH") or os.path.join(_HERE, "librender_mi355x.so")

APT_OK = 0
APT_MODE_KERNEL, APT_MODE_ORACLE = 0, 1
APT_FLAG_RETIRE = 1
APT_FLAG_RR = 2
APT_FLAG_EMISSION = 4
APT_FLAG_BAND_BUFFERS = 8
APT_FLAG_GRID_SLOTS = 16
APT_FLAG_NEE = 32
APT_FLAG_GLOSS = 64
APT_FLAG_MIS = 128                      # with APT_FLAG_GLOSS and a light mode (APT_FLAG_NEE or a light table): GLOSS hits sample the lights too
APT_FLAG_PIXEL_LIST = 256               # apt_render_frame_film only: pixel_begin carries the device address of a uint32 pixel list ("List passes")
APT_ERR_DEVICE = 4
APT_DEV_QUEUE_GUARD, APT_DEV_GRID_TURNS, APT_DEV_LDS_BASE, APT_DEV_GRID_MISMATCH = 1, 2, 4, 8      # bits of the device status word (apt_context_check)
APT_DEV_BAD_MATERIAL = 16
APT_DEV_LIGHTS_MISMATCH = 32
APT_DEV_LIST_RANGE = 64                 # a list pass: an entry of the pixel list is beyond the image
APT_ENV_SAMPLE_SUN = 1                  # apt_environment.flags: DIFF hits sample the sun directly
APT_TONEMAP_CLIP, APT_TONEMAP_REINHARD = 0, 1   # apt_film_resolve.tonemap
APT_CURVE_LINEAR, APT_CURVE_SRGB = 0, 1         # apt_film_curve_host
APT_FILM_PASS_SALT = 0x9B05688C2B3E6C1F
# planes of apt_render_frame_features' buffer [APT_FEATURE_PLANES][count]: coverage, depth, normal (3 planes from 2), albedo (3 from 5)
APT_FEATURE_COVERAGE, APT_FEATURE_DEPTH, APT_FEATURE_NORMAL, APT_FEATURE_ALBEDO, APT_FEATURE_PLANES = 0, 1, 2, 5, 8
MAT_GLOSS = 3                           # with APT_FLAG_GLOSS: gen_data.gloss(alpha) makes the word (APT_MAT_GLOSS_WORD)
MAT_SPEC, MAT_DIFF, MAT_REFR = 0, 1, 2  # material codes of the *_materials entries (include/render_mi355x.h APT_MAT_*)

# the reference declares render_do with C++ linkage (src/main.cpp:9-10): the mangled symbol is exported too
CXX_RENDER_DO = "_Z9render_dojPvS_PhS0_S0_"
ABI_VERSION = 3

# The prototypes of include/render_mi355x.h, one line per symbol in the header's order: name -> (restype, [argtypes]).  lib() sets them
# on the loaded library, so a bare Python int arrives at its full width and a value of the wrong kind raises instead of being
# reinterpreted.  A new entry is declared HERE; tests/test_abi_prototypes.py holds the table to the header.  uint32_t U32, uint64_t U64,
# int I, double D, size_t SZ, const char * S; every other pointer or array parameter is P (c_void_p also for pointers to records: it
# takes None, an address, byref(...), arrays and typed pointers alike); a void return is None.
P, U32, U64, I, D, SZ, S = (ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int, ctypes.c_double, ctypes.c_size_t,
                            ctypes.c_char_p)
PROTOTYPES = {
    "apt_default_params": (None, [P]),
    "render_do": (None, [U32, P, P, P, P, P]),
    "apt_render_do": (None, [U32, P, P, P, P, P]),
    "apt_set_default_params": (I, [P]),
    "apt_render_host": (I, [U32, P, P, P]),
    "apt_context_create": (P, []),
    "apt_context_destroy": (None, [P]),
    "apt_context_set_params": (I, [P, P]),
    "apt_context_set_trace_counter": (I, [P, P]),
    "apt_context_set_refill_lanes": (I, [P, U32]),
    "apt_context_check": (I, [P, P]),
    "apt_check": (I, [P]),
    "apt_context_set_debug": (I, [P, S, D]),
    "apt_set_debug": (I, [S, D]),
    "apt_context_get_debug": (I, [P, S, P]),
    "apt_get_debug": (I, [S, P]),
    "apt_context_render_do": (None, [P, U32, P, P, P, P, P]),
    "apt_context_render_do_ex": (I, [P, P, P, P, P, P]),
    "apt_context_render_frame": (I, [P, P, P, P, U64, U64, P, P]),
    "render_do_ex": (I, [P, P, P, P, P]),
    "render_frame": (I, [P, P, P, U64, U64, P, P]),
    "apt_render_frame_materials": (I, [P, P, P, P, U64, U64, P, P]),
    "apt_context_render_frame_materials": (I, [P, P, P, P, P, U64, U64, P, P]),
    "apt_render_paths_materials": (I, [P, P, P, P, P, P]),
    "apt_context_render_paths_materials": (I, [P, P, P, P, P, P, P]),
    "apt_lights_bytes": (SZ, [U32, U32]),
    "apt_build_lights_host": (I, [P, U32, P, U32, P, SZ, P]),
    "apt_render_frame_lights": (I, [P, P, P, P, P, U64, U64, P, P]),
    "apt_context_render_frame_lights": (I, [P, P, P, P, P, P, U64, U64, P, P]),
    "apt_render_paths_lights": (I, [P, P, P, P, P, P, P]),
    "apt_context_render_paths_lights": (I, [P, P, P, P, P, P, P, P]),
    "apt_gen_spheres_materials_host": (I, [P, P]),
    "apt_gen_scene_materials_host": (I, [U32, U64, P]),
    "apt_materials_flags_host": (U32, [P, U32]),
    "apt_camera_default_host": (I, [U32, U32, P]),
    "apt_camera_build_host": (I, [P, P, P, D, D, D, D, U32, U32, P]),
    "apt_camera_check_host": (I, [P]),
    "apt_context_set_camera": (I, [P, P]),
    "apt_set_camera": (I, [P]),
    "apt_gen_rays_camera_device": (I, [P, P, P, P]),
    "apt_environment_build_host": (I, [P, P, P, P, D, U32, P]),
    "apt_environment_check_host": (I, [P]),
    "apt_context_set_environment": (I, [P, P]),
    "apt_set_environment": (I, [P]),
    "apt_film_pass_seed": (U64, [U64, U32]),
    "apt_render_frame_film": (I, [P, P, P, P, P, U64, U64, P, U32]),
    "apt_context_render_frame_film": (I, [P, P, P, P, P, P, U64, U64, P, U32]),
    "apt_film_curve_host": (I, [U32, P]),
    "apt_film_resolve_device": (I, [P, P, P, U64, P, P, P]),
    "apt_film_resolve_host": (I, [P, P, U64, P, P, P]),
    "apt_write_pfm": (I, [S, U32, U32, P]),
    "apt_render_frame_features": (I, [P, P, P, U64, U64, P]),
    "apt_context_render_frame_features": (I, [P, P, P, P, U64, U64, P]),
    "apt_multi_create": (I, [P, U32, U32, P, P, P]),
    "apt_multi_render": (I, [P, P, P, P]),
    "apt_multi_destroy": (None, [P]),
    "apt_test_scene": (I, [P, P, P, P, P]),
    "apt_gen_rays_device": (I, [P, P, P]),
    "apt_mt19937_checkpoints_host": (I, [U32, U64, U32, P]),
    "apt_gen_rays_mt_device": (I, [P, P, P, U32, U64, P]),
    "apt_mt19937_checkpoints_window": (I, [P, U32, U64, U64, U32, P, P]),
    "apt_gen_rays_mt_device_ex": (I, [P, P, P, U32, U64, U64, P]),
    "apt_render_frame_mt": (I, [P, P, P, U64, U64, P, U64, U64, P, P]),
    "apt_decode_color_device": (I, [P, P, P, P, P]),
    "apt_decode_color_band": (I, [P, P, P, U64, P, P]),
    "apt_gen_rays_host": (I, [U32, U32, U32, U32, P]),
    "apt_gen_spheres_host": (I, [P]),
    "apt_gen_scene_host": (I, [U32, U64, P, P]),
    "apt_build_grid_host": (I, [P, U32, P, P]),
    "apt_grid_flags": (U32, [P, U32]),
    "apt_build_grid_device": (I, [P, U32, P, P, SZ, P]),
    "apt_write_ppm": (I, [S, U32, U32, P]),
    "apt_set_trace_counter": (I, [P]),
    "apt_selftest_sqrt": (I, [I, P, U64, U64, P]),
    "apt_selftest_div3": (I, [P, U64, U64, P]),
    "apt_selftest_div3_seeded": (I, [P, I, U64, U64, P]),
    "apt_selftest_direction": (I, [P, P, U64, P, P]),
    "apt_selftest_direction_host": (I, [P, U64, D, P, P]),
    "apt_selftest_chain_states_host": (I, [U32, U64, U64, U64, P]),
    "apt_selftest_tent_bits_host": (I, [P, U64, P]),
    "apt_set_refill_lanes": (I, [U32]),
    "apt_abi_version": (I, []),
    "apt_last_error": (S, []),
    "apt_last_status": (I, []),
    "apt_device_count": (I, []),
    CXX_RENDER_DO: (None, [U32, P, P, P, P, P]),
}
# every symbol include/render_mi355x.h declares
ABI_SYMBOLS = [name for name in PROTOTYPES if name != CXX_RENDER_DO]

# The film stages: six libraries of their own beside librender_mi355x.so, lib<stage>_mi355x.so with include/render_mi355x_<stage>.h.
# Their prototypes by the same rules, each table in its header's order (a float parameter is F32); tests/test_<stage>_cpu.py holds a
# table to its header and to the library's exports.  STAGES below is the one table of the stages.
F32 = ctypes.c_float
DENOISE_PROTOTYPES = {
    "apt_film_accumulate_device": (I, [P, P, U64, P, P, U32]),
    "apt_film_accumulate_host": (I, [P, U64, P, P, U32]),
    "apt_film_denoise_default_host": (I, [P, U32]),
    "apt_film_denoise_work_floats": (U64, [U32, U32]),
    "apt_film_denoise_device": (I, [P, P, P, P, P, U32, U32, P, P]),
    "apt_film_denoise_host": (I, [P, P, P, P, U32, U32, P, P]),
    "apt_film_denoise_last_error": (S, []),
}

ADAPTIVE_PROTOTYPES = {
    "apt_film_select_default_host": (I, [P, U32]),
    "apt_film_select_work_words": (U64, [U64]),
    "apt_film_select_device": (I, [P, P, P, P, U64, P, P, P]),
    "apt_film_select_host": (I, [P, P, P, U64, P, P, P]),
    "apt_film_accumulate_list_device": (I, [P, P, P, U64, U64, P, P, P]),
    "apt_film_accumulate_list_host": (I, [P, P, U64, U64, P, P, P]),
    "apt_film_mean_device": (I, [P, P, P, U32, U64, P]),
    "apt_film_mean_host": (I, [P, P, U32, U64, P]),
    "apt_film_adaptive_last_error": (S, []),
}

HISTORY_PROTOTYPES = {
    "apt_film_history_default_host": (I, [P]),
    "apt_film_history_device": (I, [P, P, P, P, P, P, P, P, U32, U32, P]),
    "apt_film_history_host": (I, [P, P, P, P, P, P, P, U32, U32, P]),
    "apt_film_history_export_device": (I, [P, P, U64, P, P]),
    "apt_film_history_export_host": (I, [P, U64, P, P]),
    "apt_film_history_last_error": (S, []),
}

APT_METER_BINS, APT_METER_WORDS = 256, 257
POST_PROTOTYPES = {
    "apt_film_meter_default_host": (I, [P, U32]),
    "apt_film_meter_work_words": (U64, [U64]),
    "apt_film_meter_device": (I, [P, P, P, U64, P, P]),
    "apt_film_meter_host": (I, [P, P, U64, P]),
    "apt_film_exposure_host": (I, [P, P, F32, P]),
    "apt_film_bloom_default_host": (I, [P, U32]),
    "apt_film_bloom_work_floats": (U64, [U32, U32, U32]),
    "apt_film_bloom_device": (I, [P, P, P, U32, U32, P, P]),
    "apt_film_bloom_host": (I, [P, P, U32, U32, P, P]),
    "apt_film_post_last_error": (S, []),
}

APT_COMPARE_WORDS, APT_SSIM_WORDS, APT_SSIM_TAPS = 8, 2, 11
METRICS_PROTOTYPES = {
    "apt_film_compare_default_host": (I, [P, U32, U32]),
    "apt_film_compare_work_doubles": (U64, [U64]),
    "apt_film_compare_device": (I, [P, P, P, P, U64, P, P, P]),
    "apt_film_compare_host": (I, [P, P, P, U64, P, P]),
    "apt_film_ssim_weights_host": (I, [P]),
    "apt_film_ssim_work_bytes": (U64, [U32, U32]),
    "apt_film_ssim_device": (I, [P, P, P, P, U32, U32, P, P, P]),
    "apt_film_ssim_host": (I, [P, P, P, U32, U32, P, P]),
    "apt_film_metrics_last_error": (S, []),
}

UPSCALE_PROTOTYPES = {
    "apt_film_upscale_default_host": (I, [P]),
    "apt_film_upscale_work_floats": (U64, [U32, U32]),
    "apt_film_upscale_device": (I, [P, P, P, P, U32, U32, P, U32, U32, P, P, P]),
    "apt_film_upscale_host": (I, [P, P, P, U32, U32, P, U32, U32, P, P, P]),
    "apt_film_upscale_patch_device": (I, [P, P, P, U64, U32, U64, P]),
    "apt_film_upscale_patch_host": (I, [P, P, U64, U32, U64, P]),
    "apt_film_upscale_last_error": (S, []),
}


class Stage:
    """One film stage: where its library is (APT_<STAGE>_LIB_PATH: another build of it, as APT_LIB_PATH), its prototype table, the
    name of its public header under include/, the symbol of its error record, and the loaded library once stage_lib() has loaded it."""

    def __init__(self, name, prototypes):
        self.name, self.prototypes = name, prototypes
        self.built_path = os.path.join(_HERE, f"lib{name}_mi355x.so")        # what the build makes
        self.lib_path = os.environ.get(f"APT_{name.upper()}_LIB_PATH") or self.built_path
        self.header = f"render_mi355x_{name}.h"
        self.last_error = f"apt_film_{name}_last_error"
        self.handle = None


# in the order the stages were added: build_id() hashes their headers in it
STAGES = {st.name: st for st in (Stage("denoise", DENOISE_PROTOTYPES), Stage("adaptive", ADAPTIVE_PROTOTYPES),
                                 Stage("history", HISTORY_PROTOTYPES), Stage("post", POST_PROTOTYPES),
                                 Stage("metrics", METRICS_PROTOTYPES), Stage("upscale", UPSCALE_PROTOTYPES))}
DENOISE_LIB_PATH, ADAPTIVE_LIB_PATH, HISTORY_LIB_PATH, POST_LIB_PATH, METRICS_LIB_PATH, UPSCALE_LIB_PATH = (st.lib_path for st in STAGES.values())


class AptError(RuntimeError):
    pass


class RenderParams(ctypes.Structure):
    """apt_render_params: run-time form of the reference's compile-time constants
    (src/common.h:4-14, src/render.cpp:141,194-196)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("samples", ctypes.c_uint32), ("depth", ctypes.c_uint32), ("num_spheres", ctypes.c_uint32),
                ("light_index", ctypes.c_int32), ("eps", ctypes.c_float), ("gain", ctypes.c_float),
                ("mode", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("rr_start", ctypes.c_uint32),
                ("path_begin", ctypes.c_uint64), ("path_count", ctypes.c_uint64), ("seed", ctypes.c_uint64),
                ("accel", ctypes.c_uint64)]

    @property
    def num_paths(self):
        return self.width * self.height * 4 * self.samples

    def copy(self, **kw):
        p = RenderParams.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(p, k, v)
        return p


class ApCamera(ctypes.Structure):
    """apt_camera (include/render_mi355x.h "camera"): the frame pos / g / cx / cy, the segment's start `offset`, and the thin lens.
    Made by gen_data.default_camera / gen_data.camera; a record filled in by hand goes through apt_camera_check_host when it is set."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("pos", ctypes.c_double * 3), ("g", ctypes.c_double * 3),
                ("cx", ctypes.c_double * 3), ("cy", ctypes.c_double * 3), ("offset", ctypes.c_double), ("aperture", ctypes.c_double),
                ("focus", ctypes.c_double), ("lens_u", ctypes.c_double * 3), ("lens_v", ctypes.c_double * 3),
                ("offset_over_focus", ctypes.c_double)]

    def copy(self, **kw):
        c = ApCamera.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(c, k, (ctypes.c_double * 3)(*v) if isinstance(v, (tuple, list)) else v)
        return c


class ApEnvironment(ctypes.Structure):
    """apt_environment (include/render_mi355x.h "environment"): the sky's two radiances, the sun's direction, radiance and cone
    (sun_omc = 1 - cos(half angle), 0 = no sun), APT_ENV_* flags.  Made by gen_data.environment; a record filled in by hand goes
    through apt_environment_check_host when it is set."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("horizon", ctypes.c_float * 3), ("zenith", ctypes.c_float * 3),
                ("sun_dir", ctypes.c_float * 3), ("sun_radiance", ctypes.c_float * 3), ("sun_omc", ctypes.c_float)]

    def copy(self, **kw):
        e = ApEnvironment.from_buffer_copy(bytes(self))
        for k, v in kw.items():
            setattr(e, k, (ctypes.c_float * 3)(*v) if isinstance(v, (tuple, list)) else v)
        return e


class ApFilmResolve(ctypes.Structure):
    """apt_film_resolve (include/render_mi355x.h "film"): passes in the film, the tone operator, exposure and 1 / white^2."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("passes", ctypes.c_uint32), ("tonemap", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("exposure", ctypes.c_float), ("inv_white2", ctypes.c_float)]


def film_resolve_record(passes, exposure=1.0, tonemap=APT_TONEMAP_CLIP, inv_white2=0.0):
    return ApFilmResolve(ctypes.sizeof(ApFilmResolve), passes, tonemap, 0, exposure, inv_white2)


class ApFilmDenoise(ctypes.Structure):
    """apt_film_denoise (include/render_mi355x_denoise.h): passes in the film and its moments, a-trous iterations, the five edge-stopping
    sigmas (normal, depth, coverage, albedo, luminance) and the albedo floor."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("passes", ctypes.c_uint32), ("iterations", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("sigma_n", ctypes.c_float), ("sigma_z", ctypes.c_float), ("sigma_c", ctypes.c_float), ("sigma_a", ctypes.c_float),
                ("sigma_l", ctypes.c_float), ("albedo_floor", ctypes.c_float)]


def _replace_fields(rec, what, fields, permitted):
    """`rec` with each of `fields` set; one that is not `permitted` is refused in the name of the helper `what`."""
    for k, v in fields.items():
        if k not in permitted:
            raise AptError(f"{what}: unknown field {k!r}")
        setattr(rec, k, v)
    return rec


def film_denoise_record(passes, iterations=None, **fields):
    """apt_film_denoise_default_host's record for `passes`, with `iterations` and any of sigma_n, sigma_z, sigma_c, sigma_a, sigma_l,
    albedo_floor replaced."""
    rec = ApFilmDenoise()
    denoise_check(denoise_lib().apt_film_denoise_default_host(ctypes.byref(rec), passes), "apt_film_denoise_default_host")
    if iterations is not None:
        rec.iterations = iterations
    return _replace_fields(rec, "film_denoise_record", fields, ("sigma_n", "sigma_z", "sigma_c", "sigma_a", "sigma_l", "albedo_floor"))


class ApFilmSelect(ctypes.Structure):
    """apt_film_select (include/render_mi355x_adaptive.h): the uniform passes in the film, the pass counts below which a pixel is always
    and from which it is never selected, the relative error that is enough and the luminance floor under it."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("base_passes", ctypes.c_uint32), ("min_passes", ctypes.c_uint32),
                ("max_passes", ctypes.c_uint32), ("threshold", ctypes.c_float), ("floor", ctypes.c_float)]


def film_select_record(base_passes, **fields):
    """apt_film_select_default_host's record for `base_passes`, with any of min_passes, max_passes, threshold, floor replaced."""
    rec = ApFilmSelect()
    adaptive_check(adaptive_lib().apt_film_select_default_host(ctypes.byref(rec), base_passes), "apt_film_select_default_host")
    return _replace_fields(rec, "film_select_record", fields, ("min_passes", "max_passes", "threshold", "floor"))


class ApFilmHistory(ctypes.Structure):
    """apt_film_history (include/render_mi355x_history.h): the clamp of the history length, the plane and normal tolerances of a
    reprojected tap and the least accepted bilinear weight of a valid pixel."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("max_history", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("tol_plane", ctypes.c_float), ("tol_normal", ctypes.c_float), ("min_weight", ctypes.c_float)]


def film_history_record(**fields):
    """apt_film_history_default_host's record, with any of max_history, tol_plane, tol_normal, min_weight replaced."""
    rec = ApFilmHistory()
    history_check(history_lib().apt_film_history_default_host(ctypes.byref(rec)), "apt_film_history_default_host")
    return _replace_fields(rec, "film_history_record", fields, ("max_history", "tol_plane", "tol_normal", "min_weight"))


class ApFilmMeter(ctypes.Structure):
    """apt_film_meter (include/render_mi355x_post.h): passes in the film, the metered percentile range in 1/65536, the key luminance,
    the exposure's clamps and the share of the way from the last frame's exposure to the metered one."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("passes", ctypes.c_uint32), ("low_q", ctypes.c_uint32), ("high_q", ctypes.c_uint32),
                ("key", ctypes.c_float), ("min_exposure", ctypes.c_float), ("max_exposure", ctypes.c_float), ("adapt", ctypes.c_float)]


def film_meter_record(passes, **fields):
    """apt_film_meter_default_host's record for `passes`, with any of low_q, high_q, key, min_exposure, max_exposure, adapt replaced."""
    rec = ApFilmMeter()
    post_check(post_lib().apt_film_meter_default_host(ctypes.byref(rec), passes), "apt_film_meter_default_host")
    return _replace_fields(rec, "film_meter_record", fields, ("low_q", "high_q", "key", "min_exposure", "max_exposure", "adapt"))


class ApFilmBloom(ctypes.Structure):
    """apt_film_bloom (include/render_mi355x_post.h): passes in the film, pyramid levels, the luminance threshold, the per-channel cap,
    the weight of each coarser level and the weight of the glare in the output."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("passes", ctypes.c_uint32), ("levels", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("threshold", ctypes.c_float), ("cap", ctypes.c_float), ("spread", ctypes.c_float), ("intensity", ctypes.c_float)]


def film_bloom_record(passes, **fields):
    """apt_film_bloom_default_host's record for `passes`, with any of levels, threshold, cap, spread, intensity replaced."""
    rec = ApFilmBloom()
    post_check(post_lib().apt_film_bloom_default_host(ctypes.byref(rec), passes), "apt_film_bloom_default_host")
    return _replace_fields(rec, "film_bloom_record", fields, ("levels", "threshold", "cap", "spread", "intensity"))


class ApFilmCompare(ctypes.Structure):
    """apt_film_compare (include/render_mi355x_metrics.h): the passes in the film and in the reference, the exposure of the clipped
    error and of SSIM, and what the relative error adds to the squared reference."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("passes_a", ctypes.c_uint32), ("passes_b", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
                ("exposure", ctypes.c_float), ("eps", ctypes.c_float)]


def film_compare_record(passes_a, passes_b=1, **fields):
    """apt_film_compare_default_host's record for the two pass counts, with any of exposure, eps replaced."""
    rec = ApFilmCompare()
    metrics_check(metrics_lib().apt_film_compare_default_host(ctypes.byref(rec), passes_a, passes_b), "apt_film_compare_default_host")
    return _replace_fields(rec, "film_compare_record", fields, ("exposure", "eps"))


class ApFilmUpscale(ctypes.Structure):
    """apt_film_upscale (include/render_mi355x_upscale.h): the edge-stopping sigmas of the guided sum (normal, depth, coverage, albedo),
    the floor under a demodulating albedo and the least guided weight of a resolved pixel."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("sigma_n", ctypes.c_float), ("sigma_z", ctypes.c_float),
                ("sigma_c", ctypes.c_float), ("sigma_a", ctypes.c_float), ("albedo_floor", ctypes.c_float), ("min_weight", ctypes.c_float)]


def film_upscale_record(**fields):
    """apt_film_upscale_default_host's record, with any of sigma_n, sigma_z, sigma_c, sigma_a, albedo_floor, min_weight replaced."""
    rec = ApFilmUpscale()
    upscale_check(upscale_lib().apt_film_upscale_default_host(ctypes.byref(rec)), "apt_film_upscale_default_host")
    return _replace_fields(rec, "film_upscale_record", fields, ("sigma_n", "sigma_z", "sigma_c", "sigma_a", "albedo_floor", "min_weight"))


_lib = None


def lib():
    """The loaded library; raises AptError when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AptError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C ascendpathtracing_amd/csrc` (there is no CPU fallback)")
        # One HIP runtime per process: torch's wheel bundles its own libamdhip64 (soname
        # libamdhip64.so.7) and asks for it by file name, so it must be loaded BEFORE this
        # library, which then binds to the already-loaded soname instead of /opt/rocm's copy.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            h = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # e.g. libamdhip64 not found
            raise AptError(f"cannot load {LIB_PATH}: {e}") from e
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(h, name)       # every symbol resolves, or AttributeError names the missing one
            fn.restype, fn.argtypes = restype, argtypes
        if h.apt_abi_version() != ABI_VERSION:
            raise AptError("librender_mi355x.so ABI version mismatch")
        _lib = h
    return _lib


def stage_lib(name):
    """The loaded library of the film stage `name`; raises AptError when it has not been built.  As lib(): no fallback."""
    st = STAGES[name]
    if st.handle is None:
        if not os.path.exists(st.lib_path):
            raise AptError(f"{st.lib_path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "or `make -C ascendpathtracing_amd/csrc` (there is no CPU fallback)")
        lib()                           # the one HIP runtime of the process is loaded first, as lib() arranges it
        try:
            h = ctypes.CDLL(st.lib_path)
        except OSError as e:
            raise AptError(f"cannot load {st.lib_path}: {e}") from e
        for symbol, (restype, argtypes) in st.prototypes.items():
            fn = getattr(h, symbol)
            fn.restype, fn.argtypes = restype, argtypes
        st.handle = h
    return st.handle


def stage_check(name, rc, what):
    if rc != APT_OK:
        raise AptError(f"{what} failed ({rc}): {getattr(stage_lib(name), STAGES[name].last_error)().decode()}")


denoise_lib, adaptive_lib, history_lib, post_lib, metrics_lib, upscale_lib = (functools.partial(stage_lib, name) for name in STAGES)
denoise_check, adaptive_check, history_check, post_check, metrics_check, upscale_check = (functools.partial(stage_check, name) for name in STAGES)


def public_headers():
    """The public headers under include/: librender_mi355x.so's, then the stages' in the table's order."""
    include = os.path.join(os.path.dirname(_HERE), "include")
    return [os.path.join(include, h) for h in ["render_mi355x.h"] + [st.header for st in STAGES.values()]]


def build_id():
    """Identifies the build of the library by its SOURCES (sha256 over ascendpathtracing_amd/csrc/*.{h,hip,cpp}, the Makefile and the
    public headers, first 16 hex digits): what profiles/summarize.py stamps the recorded PMC traffic with and bench.py compares
    before it reports that traffic for the library it is running."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.h")) + glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")))
    files += [os.path.join(csrc, "Makefile"), os.path.join(csrc, "apt_exports.map")] + public_headers()
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def check(rc, what):
    if rc != APT_OK:
        raise AptError(f"{what} failed ({rc}): {lib().apt_last_error().decode()}")


def default_params():
    p = RenderParams()
    lib().apt_default_params(ctypes.byref(p))
    return p


def make_params(width=16, height=16, samples=1, depth=5, num_spheres=8, light_index=None, eps=1e-4, gain=12.0,
                mode=APT_MODE_KERNEL, flags=0, path_begin=0, path_count=0, seed=0, rr_start=0, accel=0):
    p = default_params()
    p.width, p.height, p.samples, p.depth = width, height, samples, depth
    p.num_spheres = num_spheres
    p.light_index = num_spheres - 1 if light_index is None else light_index
    p.eps, p.gain, p.mode, p.flags, p.rr_start = eps, gain, mode, flags, rr_start
    p.path_begin, p.path_count, p.seed, p.accel = path_begin, path_count, seed, accel
    return p


def require_gpu():
    if lib().apt_device_count() < 1:
        raise AptError("no HIP device visible: the render path needs an MI355X (no CPU fallback)")
