"""The render boundary, mirroring the reference host interface (src/main.cpp:9-10,74;
src/render.cpp:262-266) on top of the C-ABI.  Tensors are torch CUDA(HIP) tensors used only
as device buffers; the stream is a torch stream (or None = torch's current stream)."""
import ctypes

import torch

from . import _lib
from ._lib import MAT_DIFF, MAT_REFR, MAT_SPEC, RenderParams, check, lib, require_gpu  # noqa: F401  (MAT_*: the materials= codes)


def _stream_handle(stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    return stream if isinstance(stream, int) else stream.cuda_stream


def _torch_stream(stream):
    """The same stream as a torch object, for work that torch itself enqueues."""
    if stream is None:
        return torch.cuda.current_stream()
    return torch.cuda.ExternalStream(stream) if isinstance(stream, int) else stream


def _dev_f32(t, name, numel=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise _lib.AptError(f"{name} must be a contiguous float32 tensor on the GPU")
    if numel is not None and t.numel() != numel:
        raise _lib.AptError(f"{name} has {t.numel()} elements, expected {numel}")
    return t.data_ptr()


def _buffer_paths(params):
    """Paths per plane of the ray / colour buffers of a buffer-mode call: the whole image, or the range alone with band-relative buffers."""
    if params.flags & _lib.APT_FLAG_BAND_BUFFERS:
        return params.path_count or (params.num_paths - params.path_begin)   # path_count 0: to the end of the image (path_range)
    return params.num_paths


def _dev_materials(t, num_spheres):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise _lib.AptError("materials must be a contiguous int32 tensor on the GPU")
    if t.numel() != num_spheres:
        raise _lib.AptError(f"materials has {t.numel()} elements, expected num_spheres = {num_spheres}")
    return t.data_ptr()


def _dev_u32(t, name, numel=None):
    """uint32 words travel in int32 tensors, as the material words do."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise _lib.AptError(f"{name} must be a contiguous int32 tensor on the GPU (it holds uint32 words)")
    if numel is not None and t.numel() != numel:
        raise _lib.AptError(f"{name} has {t.numel()} elements, expected {numel}")
    return t.data_ptr()


def _dev_pixel_list(t):
    if not (isinstance(t, torch.Tensor) and t.numel() >= 1):
        raise _lib.AptError("pixel_list must hold at least one entry")
    return _dev_u32(t, "pixel_list")


def _dev_lights(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= 16):
        raise _lib.AptError("lights must be a contiguous int32 tensor on the GPU holding a light table (gen_data.build_lights)")
    return t.data_ptr()


# The C entries by their context-free names, as the header pairs them (the pairs are irregular, so they are listed, not derived).
# _MATERIAL_FORMS: the *_materials and *_lights forms of the two entries that take materials= / lights=.
# _CONTEXT_ENTRY: the apt_context_* form of each, which takes the context's handle in front.
_MATERIAL_FORMS = {"render_do_ex": ("apt_render_paths_materials", "apt_render_paths_lights"),
                   "render_frame": ("apt_render_frame_materials", "apt_render_frame_lights")}
_CONTEXT_ENTRY = {"apt_set_default_params": "apt_context_set_params", "apt_set_refill_lanes": "apt_context_set_refill_lanes",
                  "apt_set_trace_counter": "apt_context_set_trace_counter", "apt_set_camera": "apt_context_set_camera",
                  "apt_set_environment": "apt_context_set_environment", "apt_set_debug": "apt_context_set_debug",
                  "apt_get_debug": "apt_context_get_debug", "apt_check": "apt_context_check",
                  "render_do": "apt_context_render_do", "render_do_ex": "apt_context_render_do_ex",
                  "render_frame": "apt_context_render_frame",
                  "apt_render_paths_materials": "apt_context_render_paths_materials",
                  "apt_render_frame_materials": "apt_context_render_frame_materials",
                  "apt_render_paths_lights": "apt_context_render_paths_lights",
                  "apt_render_frame_lights": "apt_context_render_frame_lights",
                  "apt_render_frame_film": "apt_context_render_frame_film",
                  "apt_render_frame_features": "apt_context_render_frame_features"}


def _material_args(entry, params, materials, lights):
    """-> (the entry to call, its extra arguments after `spheres`): the entry itself, its *_materials form, or its *_lights form."""
    if lights is not None and materials is None:
        raise _lib.AptError("lights needs materials: the light table belongs to the material renderer")
    if materials is None:
        return entry, ()
    mat = (_dev_materials(materials, params.num_spheres),)
    if lights is None:
        return _MATERIAL_FORMS[entry][0], mat
    return _MATERIAL_FORMS[entry][1], mat + (_dev_lights(lights),)


def sphere_floats(num_spheres):
    """Length of the zero-padded [10][Ns] table (512-byte multiple, gen_data.py:120-127)."""
    return (num_spheres * 10 + 127) // 128 * 128


class Context:
    """apt_context: private settings for render_do / render_do_ex / render_frame (instead of the process-wide
    default context); safe to use from several threads, one context per thread needs no coordination at all."""
    _private = True     # False in one object only: `_default` below, the process-wide default context, which has no handle

    def __init__(self, params=None):
        self._h = lib().apt_context_create()
        if not self._h:
            raise _lib.AptError("apt_context_create failed")
        if params is not None:
            self.set_params(params)

    def close(self):
        if self._h:
            lib().apt_context_destroy(self._h)
            self._h = None

    __del__ = close

    def _call(self, name, *args):
        """Every entry's crossing of the boundary.  `name` is the context-free entry: the default context calls it, a private one
        its apt_context_* form with the handle in front.  A failure is reported under the name of the entry that was called."""
        entry, args = (_CONTEXT_ENTRY[name], (self._h,) + args) if self._private else (name, args)
        rc = getattr(lib(), entry)(*args)
        # render_do is void like the reference (rc None): the outcome of THIS call, on this thread, is apt_last_status()
        check(lib().apt_last_status() if rc is None else rc, entry)

    def set_params(self, params):
        self._call("apt_set_default_params", ctypes.byref(params))

    def set_refill_lanes(self, lanes):
        self._call("apt_set_refill_lanes", lanes)

    def set_trace_counter(self, tensor_or_none):
        self._call("apt_set_trace_counter", None if tensor_or_none is None else tensor_or_none.data_ptr())

    def set_camera(self, cam):
        """apt_context_set_camera: this context's material frames render from `cam` (gen_data.camera / default_camera; None: the
        reference's camera again), its mirror frame entries refuse while one is set."""
        self._call("apt_set_camera", None if cam is None else ctypes.byref(cam))

    def set_environment(self, env):
        """apt_context_set_environment: this context's material and light-table entries, frame and buffer mode, gather `env`'s sky and
        sun where a path leaves the scene (gen_data.environment; None: no environment, every image as before); its mirror frame
        entries refuse while one is set."""
        self._call("apt_set_environment", None if env is None else ctypes.byref(env))

    def set_debug(self, key, value):
        self._call("apt_set_debug", key.encode(), value)

    def get_debug(self, key):
        v = ctypes.c_double(0)
        self._call("apt_get_debug", key.encode(), ctypes.byref(v))
        return v.value

    def check(self, stream=None):
        """apt_context_check: waits for `stream`, raises AptError when a kernel of this context reported a failure through the
        device status word (the reference asserts inside its kernel, src/render.cpp:68-73)."""
        self._call("apt_check", _stream_handle(stream))

    def render_do(self, blockDim, l2ctrl, stream, rays, spheres, colors):
        require_gpu()
        self._call("render_do", blockDim, None, _stream_handle(stream), _dev_f32(rays, "rays"), _dev_f32(spheres, "spheres"),
                   _dev_f32(colors, "colors"))

    # materials (int32 tensor of num_spheres codes, MAT_*): the entry's *_materials form; None: the entry itself, untouched.
    # lights (int32 tensor, a light table: gen_data.build_lights), with materials only: the entry's *_lights form.
    def render_do_ex(self, params, stream, rays, spheres, colors, materials=None, lights=None):
        require_gpu()
        n = _buffer_paths(params)
        entry, mat = _material_args("render_do_ex", params, materials, lights)
        self._call(entry, ctypes.byref(params), _stream_handle(stream), _dev_f32(rays, "rays", 6 * n),
                   _dev_f32(spheres, "spheres", sphere_floats(params.num_spheres)), *mat, _dev_f32(colors, "colors", 3 * n))

    def render_frame(self, params, spheres, pixel_begin=0, pixel_count=None, stream=None, fb=None, fb_u8=None, materials=None,
                     lights=None):
        require_gpu()
        npix = params.width * params.height
        if pixel_count is None:
            pixel_count = npix - pixel_begin
        if fb is None:
            fb = torch.empty((3, pixel_count), dtype=torch.float32, device=spheres.device)
        if fb_u8 is None:
            fb_u8 = torch.empty((pixel_count, 3), dtype=torch.uint8, device=spheres.device)
        entry, mat = _material_args("render_frame", params, materials, lights)
        self._call(entry, ctypes.byref(params), _stream_handle(stream), _dev_f32(spheres, "spheres", sphere_floats(params.num_spheres)),
                   *mat, pixel_begin, pixel_count, _dev_f32(fb, "fb", 3 * pixel_count), fb_u8.data_ptr())
        return fb, fb_u8

    def render_frame_film(self, params, spheres, materials, film=None, pass_index=0, lights=None, pixel_begin=0, pixel_count=None,
                          stream=None, pixel_list=None):
        require_gpu()
        if pixel_list is not None:       # a list pass (APT_FLAG_PIXEL_LIST): the list's address travels in pixel_begin
            if pixel_begin != 0:
                raise _lib.AptError("render_frame_film: pixel_list takes no pixel_begin")
            if pixel_count is None:
                pixel_count = pixel_list.numel()
            if pixel_count > pixel_list.numel():
                raise _lib.AptError(f"pixel_list has {pixel_list.numel()} entries, fewer than pixel_count = {pixel_count}")
            pixel_begin = _dev_pixel_list(pixel_list)
            params = params.copy(flags=params.flags | _lib.APT_FLAG_PIXEL_LIST)
        elif params.flags & _lib.APT_FLAG_PIXEL_LIST:
            raise _lib.AptError("render_frame_film: APT_FLAG_PIXEL_LIST is set by pixel_list=, which holds the list")
        if pixel_count is None:
            pixel_count = params.width * params.height - pixel_begin
        if film is None:
            film = torch.empty((3, pixel_count), dtype=torch.float32, device=spheres.device)
        self._call("apt_render_frame_film", ctypes.byref(params), _stream_handle(stream),
                   _dev_f32(spheres, "spheres", sphere_floats(params.num_spheres)), _dev_materials(materials, params.num_spheres),
                   None if lights is None else _dev_lights(lights), pixel_begin, pixel_count, _dev_f32(film, "film", 3 * pixel_count),
                   pass_index)
        return film

    def render_frame_features(self, params, spheres, features=None, pixel_begin=0, pixel_count=None, stream=None):
        require_gpu()
        if pixel_count is None:
            pixel_count = params.width * params.height - pixel_begin
        if features is None:
            features = torch.empty((_lib.APT_FEATURE_PLANES, pixel_count), dtype=torch.float32, device=spheres.device)
        self._call("apt_render_frame_features", ctypes.byref(params), _stream_handle(stream),
                   _dev_f32(spheres, "spheres", sphere_floats(params.num_spheres)), pixel_begin, pixel_count,
                   _dev_f32(features, "features", _lib.APT_FEATURE_PLANES * pixel_count))
        return features


# the process-wide default context as an object of the same class: the module-level functions below forward to it
_default = object.__new__(Context)
_default._h, _default._private = None, False


def render_do(blockDim, l2ctrl, stream, rays, spheres, colors):
    """void render_do(blockDim, l2ctrl, stream, rays, spheres, colors) -- src/main.cpp:9-10,74.
    Asynchronous on `stream`; uses the process-wide defaults (apt_set_default_params)."""
    _default.render_do(blockDim, l2ctrl, stream, rays, spheres, colors)


def render_host(blockDim, rays, spheres, colors):
    """The CPU-simulator shape of the boundary (src/main.cpp:21-44, ICPU_RUN_KF(render, ...)): HOST numpy float32
    buffers in, colours out, synchronous.  Uses the default context's parameters (set_default_params)."""
    import numpy as np
    require_gpu()
    for a, name in ((rays, "rays"), (spheres, "spheres"), (colors, "colors")):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous):
            raise _lib.AptError(f"{name} must be a C-contiguous float32 numpy array")
    check(lib().apt_render_host(blockDim, rays.ctypes.data, spheres.ctypes.data, colors.ctypes.data), "apt_render_host")


class MultiGpu:
    """apt_multi: one process, several GPUs.  Band b of the frame renders on device_ids[b]; with stripes > 1 the
    bands are interleaved stripes.  The frame is assembled on device_ids[0] by peer copies (no collective)."""

    def __init__(self, params, spheres_host, device_ids, stripes=1):
        import numpy as np
        require_gpu()
        sph = np.ascontiguousarray(spheres_host, dtype=np.float32)
        if sph.size != sphere_floats(params.num_spheres):
            raise _lib.AptError("spheres_host has the wrong length")
        ids = (ctypes.c_int * len(device_ids))(*device_ids)
        self._h = ctypes.c_void_p()
        check(lib().apt_multi_create(ids, len(device_ids), stripes, ctypes.byref(params), sph.ctypes.data, ctypes.byref(self._h)),
              "apt_multi_create")
        self.params, self.device_ids, self.stripes = params, list(device_ids), stripes
        self.band_kernel_ms = [0.0] * len(device_ids)

    def render(self, fb=None, fb_u8=None):
        """-> (fb [3][W*H] float32, u8 [W*H][3]) on device_ids[0]; synchronous."""
        npix = self.params.width * self.params.height
        dev = torch.device("cuda", self.device_ids[0])
        if fb is None:
            fb = torch.empty((3, npix), dtype=torch.float32, device=dev)
        if fb_u8 is None:
            fb_u8 = torch.empty((npix, 3), dtype=torch.uint8, device=dev)
        ms = (ctypes.c_float * len(self.device_ids))()
        check(lib().apt_multi_render(self._h, fb.data_ptr(), fb_u8.data_ptr(), ms), "apt_multi_render")
        self.band_kernel_ms = list(ms)
        return fb, fb_u8

    def close(self):
        if getattr(self, "_h", None):
            lib().apt_multi_destroy(self._h)
            self._h = None

    __del__ = close


def set_default_params(params):
    _default.set_params(params)


def set_camera(cam):
    """apt_set_camera: the default context's camera (gen_data.camera / default_camera), or None for the reference's.  render_frame with
    materials= then renders from it; render_frame without materials refuses while it is set (gen_rays_camera + render_paths +
    decode_color_device gives the mirror renderer a camera)."""
    _default.set_camera(cam)


def set_environment(env):
    """apt_set_environment: the default context's environment (gen_data.environment), or None for none.  render_frame / render_do_ex
    with materials= (and lights=) then light every path that leaves the scene with its sky and sun; render_frame without materials
    refuses while it is set.  dist.py and MultiGpu render mirrors only: they take neither materials nor an environment."""
    _default.set_environment(env)


def set_debug(key, value):
    """Measurement knob of the default context (include/render_mi355x.h apt_context_set_debug): "queue_ppw", "queue_nbuf",
    "queue_lds_pad", "grid_walk" (1 = nested item walk), "grid_spheres_per_cell"; 0 = the library's own choice."""
    _default.set_debug(key, value)


def get_debug(key):
    """The knob's current value in the default context (apt_get_debug)."""
    return _default.get_debug(key)


class debug_knob:
    """with debug_knob("grid_walk", 1): ...  -- sets a knob of the default context and puts back the value it FOUND on the way out
    (an initial value from the environment, or an enclosing debug_knob's), also after an exception (tests select kernels this way,
    never through the process environment)."""

    def __init__(self, key, value):
        self.key, self.value, self.before = key, value, 0

    def __enter__(self):
        self.before = get_debug(self.key)
        set_debug(self.key, self.value)
        return self

    def __exit__(self, *exc):
        set_debug(self.key, self.before)


def check_device_status(stream=None):
    """apt_check: waits for `stream` (None = torch's current stream) and raises AptError when a kernel launched through the default
    context reported a failure through the device status word since the last check (a tripped loop bound: the frame is incomplete)."""
    require_gpu()
    _default.check(stream)


def render_do_ex(params: RenderParams, stream, rays, spheres, colors, materials=None, lights=None):
    """Run-time-parameter form of render_do: rays [6][N], spheres [10][Ns] padded, colors [3][N] (with APT_FLAG_BAND_BUFFERS: planes of
    path_count floats holding only the range).  materials: contiguous int32 CUDA tensor of num_spheres MAT_* codes -> per-path radiance
    of the material renderer (apt_render_paths_materials); None: the mirror renderer.  With materials, params.accel (a built grid)
    is taken only together with APT_FLAG_GRID_SLOTS (gen_data.grid_flags of that grid): the same colours, found by walking the grid.
    APT_FLAG_NEE in params.flags (materials only): every diffuse hit samples the sphere params.light_index directly -- the same
    expectation at the same depth, less noise for a small light; it needs light_index >= 0.
    lights (materials only): a light table on the GPU (gen_data.build_lights, as a contiguous int32 CUDA tensor) -> every diffuse hit
    samples ONE of the listed spheres (apt_render_paths_lights); APT_FLAG_NEE and light_index are not read then.  A table that is not
    this scene's renders nothing and check_device_status() raises lights-mismatch.
    APT_FLAG_MIS in params.flags (gen_data.materials_flags(table, mis=True)): read only next to APT_FLAG_GLOSS and a light mode
    (APT_FLAG_NEE or lights) -- the rough-metal hits then sample the light too, weighted against their own sampler by the balance
    heuristic: the same expectation at the same depth, far less noise in the highlight of a small lamp.  Every other launch ignores the bit."""
    _default.render_do_ex(params, stream, rays, spheres, colors, materials, lights)


def render_paths(params: RenderParams, rays, spheres, stream=None, materials=None, lights=None):
    """Convenience: allocate colours, launch, return the [3][N] tensor (not synchronised)."""
    colors = torch.empty(3 * params.num_paths, dtype=torch.float32, device=rays.device)
    render_do_ex(params, stream, rays, spheres, colors, materials, lights)
    return colors.view(3, -1)


def render_frame(params: RenderParams, spheres, pixel_begin=0, pixel_count=None, stream=None, fb=None, fb_u8=None, materials=None,
                 lights=None):
    """Fused ray-generate + trace + decode for pixels [pixel_begin, pixel_begin+pixel_count).
    Returns (fb float32 [3][count], fb_u8 uint8 [count][3]); not synchronised.  materials: as render_do_ex (apt_render_frame_materials),
    its rule for params.accel included: a grid needs APT_FLAG_GRID_SLOTS, changes which spheres are tested and never the image; a grid
    that is not this scene's renders nothing and check_device_status() raises grid-mismatch.  APT_FLAG_NEE, lights, APT_FLAG_MIS: as
    render_do_ex (apt_render_frame_lights)."""
    return _default.render_frame(params, spheres, pixel_begin, pixel_count, stream, fb, fb_u8, materials, lights)


def render_frame_film(params: RenderParams, spheres, materials, film=None, pass_index=0, lights=None, pixel_begin=0, pixel_count=None,
                      stream=None, pixel_list=None):
    """apt_render_frame_film: one pass of a film.  The pixel range rendered as render_frame(materials=, lights=) would with the seed
    apt_film_pass_seed(params.seed, pass_index), unclipped, stored in `film` (float32 [3][count]; None: a new tensor) for pass 0 and
    added to it for a later pass.  Returns the film; not synchronised.  The flags travel in params.flags, APT_FLAG_MIS among them.
    pixel_list (an int32 device tensor of image pixel indices; pixel_count: how many of them, None: all): a list pass
    (APT_FLAG_PIXEL_LIST) -- `film` is then a compact scratch [3][count] whose word c * count + i is STORED with what pass
    `pass_index` over the whole image gives pixel pixel_list[i]; an entry beyond the image leaves its slot untouched and
    check_device_status() raises list-range."""
    return _default.render_frame_film(params, spheres, materials, film, pass_index, lights, pixel_begin, pixel_count, stream, pixel_list)


def film_select(record, moments, extra, work=None, pixel_list=None, count=None, stream=None):
    """apt_film_select_device (libadaptive_mi355x.so, include/render_mi355x_adaptive.h): the pixels of a film -- moments float32 [2][N],
    extra int32 [N] -- that `record` (_lib.film_select_record) sends another pass to, in ascending order -> (pixel_list int32 [N], of
    which the first `count` are written, count int32 [1]), both on the device; not synchronised.  work: int32, at least
    apt_film_select_work_words(N) elements.  None: new tensors."""
    require_gpu()
    n = moments.numel() // 2
    L = _lib.adaptive_lib()
    words = L.apt_film_select_work_words(n)
    if work is None:
        work = torch.empty(words, dtype=torch.int32, device=moments.device)
    if work.numel() < words:
        raise _lib.AptError(f"work has {work.numel()} elements, fewer than apt_film_select_work_words = {words}")
    if pixel_list is None:
        pixel_list = torch.empty(n, dtype=torch.int32, device=moments.device)
    if count is None:
        count = torch.empty(1, dtype=torch.int32, device=moments.device)
    _lib.adaptive_check(L.apt_film_select_device(ctypes.byref(record), _stream_handle(stream), _dev_f32(moments, "moments", 2 * n),
                                                 _dev_u32(extra, "extra", n), n, _dev_u32(work, "work"), _dev_u32(pixel_list, "pixel_list", n),
                                                 _dev_u32(count, "count", 1)), "apt_film_select_device")
    return pixel_list, count


def film_accumulate_list(pass_planes, pixel_list, list_count, film, moments, extra, stream=None):
    """apt_film_accumulate_list_device: the compact planes of ONE list pass (the first 3 * list_count floats of `pass_planes`) added
    to the pixels the first list_count entries of pixel_list name: film [3][N], moments [2][N], extra [N] += 1.  Not synchronised."""
    require_gpu()
    n = film.numel() // 3
    if pass_planes.numel() < 3 * list_count or pixel_list.numel() < list_count:
        raise _lib.AptError("film_accumulate_list: pass_planes or pixel_list is shorter than list_count asks")
    _lib.adaptive_check(_lib.adaptive_lib().apt_film_accumulate_list_device(
        _stream_handle(stream), _dev_f32(pass_planes, "pass_planes"), _dev_u32(pixel_list, "pixel_list"), list_count, n,
        _dev_f32(film, "film", 3 * n), _dev_f32(moments, "moments", 2 * n), _dev_u32(extra, "extra", n)), "apt_film_accumulate_list_device")
    return film, moments, extra


def film_mean(film, base_passes, extra=None, out=None, stream=None):
    """apt_film_mean_device: film [3][N] over each pixel's own number of passes, base_passes + extra[p] (extra None: base_passes
    everywhere) -> out float32 [3][N] (None: a new tensor), which Film.resolve takes as a source.  Not synchronised."""
    require_gpu()
    n = film.numel() // 3
    if out is None:
        out = torch.empty((3, n), dtype=torch.float32, device=film.device)
    _lib.adaptive_check(_lib.adaptive_lib().apt_film_mean_device(
        _stream_handle(stream), _dev_f32(film, "film", 3 * n), None if extra is None else _dev_u32(extra, "extra", n), base_passes, n,
        _dev_f32(out, "out", 3 * n)), "apt_film_mean_device")
    return out


def render_frame_features(params: RenderParams, spheres, features=None, pixel_begin=0, pixel_count=None, stream=None):
    """apt_render_frame_features: the first-hit feature planes of the pixel range -- coverage, depth, normal, albedo (APT_FEATURE_*),
    each the mean over the pixel's camera rays, the ones render_frame(materials=) traces with these params -- stored in `features`
    (float32 [APT_FEATURE_PLANES][count]; None: a new tensor).  Reads no material table and no flag but APT_FLAG_GRID_SLOTS with
    params.accel.  Returns the tensor; not synchronised."""
    return _default.render_frame_features(params, spheres, features, pixel_begin, pixel_count, stream)


def film_accumulate(pass_planes, film, moments, pass_index, stream=None):
    """apt_film_accumulate_device (libdenoise_mi355x.so, include/render_mi355x_denoise.h): ONE pass's planes (float32 [3][count]) stored in (pass_index 0) or added to `film` [3][count], its
    luminance and squared luminance to `moments` [2][count].  Returns (film, moments); not synchronised."""
    require_gpu()
    count = pass_planes.numel() // 3
    _lib.denoise_check(_lib.denoise_lib().apt_film_accumulate_device(_stream_handle(stream), _dev_f32(pass_planes, "pass_planes", 3 * count), count,
                                           _dev_f32(film, "film", 3 * count), _dev_f32(moments, "moments", 2 * count), pass_index),
          "apt_film_accumulate_device")
    return film, moments


def film_denoise(record, film, moments, features, width, height, work=None, out=None, stream=None):
    """apt_film_denoise_device: the a-trous filter of `record` (_lib.film_denoise_record) over a whole width x height image -- film
    [3][W*H], moments [2][W*H], features [APT_FEATURE_PLANES][W*H] -> `out` float32 [3][W*H], the denoised MEAN radiance (None: a new
    tensor).  work: a float32 tensor of apt_film_denoise_work_floats elements (None: a new one).  Not synchronised."""
    require_gpu()
    n = width * height
    if work is None:
        work = torch.empty(_lib.denoise_lib().apt_film_denoise_work_floats(width, height), dtype=torch.float32, device=film.device)
    if out is None:
        out = torch.empty((3, n), dtype=torch.float32, device=film.device)
    _lib.denoise_check(_lib.denoise_lib().apt_film_denoise_device(ctypes.byref(record), _stream_handle(stream), _dev_f32(film, "film", 3 * n),
                                        _dev_f32(moments, "moments", 2 * n), _dev_f32(features, "features", _lib.APT_FEATURE_PLANES * n),
                                        width, height, _dev_f32(work, "work", 16 * n), _dev_f32(out, "out", 3 * n)),
          "apt_film_denoise_device")
    return out


def film_history(record, cur, cur_features, cur_cam, out_hist, prev=None, stream=None):
    """apt_film_history_device (libhistory_mi355x.so, include/render_mi355x_history.h): the history of the previous frame -- prev =
    (prev_hist float32 [6][N], prev_features [APT_FEATURE_PLANES][N], prev_cam), None: the first frame -- reprojected to the surfaces
    the current camera `cur_cam` (an ApCamera) sees and blended with `cur`, the current frame's MEAN radiance [3][N], by `record`
    (_lib.film_history_record) -> out_hist float32 [6][N], a (width, height) image given by out_hist's shape (6, width, height).
    Returns out_hist; not synchronised."""
    require_gpu()
    if not (isinstance(out_hist, torch.Tensor) and out_hist.dim() == 3 and out_hist.shape[0] == 6):
        raise _lib.AptError("out_hist must have the shape (6, width, height)")
    width, height = int(out_hist.shape[1]), int(out_hist.shape[2])
    n = width * height
    p_hist, p_feat, p_cam = (None, None, None) if prev is None else prev
    _lib.history_check(_lib.history_lib().apt_film_history_device(
        ctypes.byref(record), _stream_handle(stream), ctypes.byref(cur_cam), None if p_cam is None else ctypes.byref(p_cam),
        _dev_f32(cur, "cur", 3 * n), _dev_f32(cur_features, "cur_features", _lib.APT_FEATURE_PLANES * n),
        None if p_feat is None else _dev_f32(p_feat, "prev_features", _lib.APT_FEATURE_PLANES * n),
        None if p_hist is None else _dev_f32(p_hist, "prev_hist", 6 * n), width, height, _dev_f32(out_hist, "out_hist", 6 * n)),
        "apt_film_history_device")
    return out_hist


def film_history_export(hist, film=None, moments=None, stream=None):
    """apt_film_history_export_device: a history buffer [6][N] as the (film [3][N], moments [2][N]) pair that film_denoise takes with a
    record of passes = 2 (None: new tensors).  Not synchronised."""
    require_gpu()
    n = hist.numel() // 6
    if film is None:
        film = torch.empty((3, n), dtype=torch.float32, device=hist.device)
    if moments is None:
        moments = torch.empty((2, n), dtype=torch.float32, device=hist.device)
    _lib.history_check(_lib.history_lib().apt_film_history_export_device(
        _stream_handle(stream), _dev_f32(hist, "hist", 6 * n), n, _dev_f32(film, "film", 3 * n), _dev_f32(moments, "moments", 2 * n)),
        "apt_film_history_export_device")
    return film, moments


def film_meter(record, film, work=None, hist=None, stream=None):
    """apt_film_meter_device (libpost_mi355x.so, include/render_mi355x_post.h): the luminance histogram of `film`, float32 [3][count]
    (a whole image or a band) divided by record.passes (_lib.film_meter_record) -> `hist`, an int32 tensor of APT_METER_WORDS uint32
    words (None: a new one), stored.  work: an int32 tensor of at least apt_film_meter_work_words(count) words (None: a new one).
    Returns hist; not synchronised."""
    require_gpu()
    count = film.numel() // 3
    words = _lib.post_lib().apt_film_meter_work_words(count)
    if work is None:
        work = torch.empty(max(words, 1), dtype=torch.int32, device=film.device)
    if hist is None:
        hist = torch.empty(_lib.APT_METER_WORDS, dtype=torch.int32, device=film.device)
    if work.numel() < words:
        raise _lib.AptError(f"work has {work.numel()} words, expected at least {words}")
    _lib.post_check(_lib.post_lib().apt_film_meter_device(ctypes.byref(record), _stream_handle(stream), _dev_f32(film, "film", 3 * count), count,
                                                          _dev_u32(work, "work"), _dev_u32(hist, "hist", _lib.APT_METER_WORDS)),
                    "apt_film_meter_device")
    return hist


def film_exposure(record, hist, prev=1.0):
    """apt_film_exposure_host: the exposure that `record` derives from the histogram `hist` (what film_meter returned, or a host array of
    APT_METER_WORDS uint32 words) and the exposure `prev` of the frame before -> float.  A device tensor is READ BACK (257 words): this
    synchronises torch's current stream; a meter enqueued on another stream must have been waited for."""
    import numpy as np
    words = hist.cpu().numpy() if isinstance(hist, torch.Tensor) else np.asarray(hist)
    if words.dtype not in (np.dtype(np.int32), np.dtype(np.uint32)):
        raise _lib.AptError("hist must hold 32-bit integer words")
    words = np.ascontiguousarray(words).view(np.uint32)
    if words.size != _lib.APT_METER_WORDS:
        raise _lib.AptError(f"hist has {words.size} words, expected {_lib.APT_METER_WORDS}")
    out = ctypes.c_float(0.0)
    _lib.post_check(_lib.post_lib().apt_film_exposure_host(ctypes.byref(record), words.ctypes.data, prev, ctypes.byref(out)),
                    "apt_film_exposure_host")
    return out.value


def film_bloom(record, film, width, height, work=None, out=None, stream=None):
    """apt_film_bloom_device: the bloom of `record` (_lib.film_bloom_record) over a whole width x height image -- film float32 [3][W*H]
    divided by record.passes -> `out` float32 [3][W*H], the MEAN radiance plus the glare (None: a new tensor; never `film` itself).
    work: a float32 tensor of apt_film_bloom_work_floats(width, height, record.levels) elements (None: a new one).  Not synchronised."""
    require_gpu()
    n = width * height
    floats = _lib.post_lib().apt_film_bloom_work_floats(width, height, record.levels)
    if work is None:
        work = torch.empty(max(floats, 4), dtype=torch.float32, device=film.device)
    if out is None:
        out = torch.empty((3, n), dtype=torch.float32, device=film.device)
    if work.numel() < floats:
        raise _lib.AptError(f"work has {work.numel()} elements, expected at least {floats}")
    _lib.post_check(_lib.post_lib().apt_film_bloom_device(ctypes.byref(record), _stream_handle(stream), _dev_f32(film, "film", 3 * n), width, height,
                                                          _dev_f32(work, "work"), _dev_f32(out, "out", 3 * n)), "apt_film_bloom_device")
    return out


def _dev_words(t, name, dtype, numel=None):
    """64-bit words: uint64 results travel in int64 tensors, the rows of a reduction in float64 ones."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise _lib.AptError(f"{name} must be a contiguous {dtype} tensor on the GPU")
    if numel is not None and t.numel() != numel:
        raise _lib.AptError(f"{name} has {t.numel()} elements, expected {numel}")
    return t.data_ptr()


def film_compare(record, a, b, work=None, result=None, err_map=None, stream=None):
    """apt_film_compare_device (libmetrics_mi355x.so, include/render_mi355x_metrics.h): film `a`, float32 [3][n] over record.passes_a,
    against the reference `b` over record.passes_b (_lib.film_compare_record) -> `result`, an int64 tensor of APT_COMPARE_WORDS uint64
    words (None: a new one), stored: the bits of the float64 tree sums of the squared, clipped squared, relative squared and absolute
    error, the key of the largest difference, the bad pixels, n, 0.  work: a float64 tensor of at least
    apt_film_compare_work_doubles(n) elements (None: a new one).  err_map: None, or float32 [n] that receives each pixel's squared
    error.  Returns result; not synchronised.  compare_summary turns the words into numbers."""
    require_gpu()
    n = a.numel() // 3
    doubles = _lib.metrics_lib().apt_film_compare_work_doubles(n)
    if work is None:
        work = torch.empty(max(doubles, 1), dtype=torch.float64, device=a.device)
    if result is None:
        result = torch.empty(_lib.APT_COMPARE_WORDS, dtype=torch.int64, device=a.device)
    if work.numel() < doubles:
        raise _lib.AptError(f"work has {work.numel()} elements, expected at least {doubles}")
    _lib.metrics_check(_lib.metrics_lib().apt_film_compare_device(
        ctypes.byref(record), _stream_handle(stream), _dev_f32(a, "a", 3 * n), _dev_f32(b, "b", 3 * n), n,
        _dev_words(work, "work", torch.float64), _dev_words(result, "result", torch.int64, _lib.APT_COMPARE_WORDS),
        None if err_map is None else _dev_f32(err_map, "err_map", n)), "apt_film_compare_device")
    return result


def film_ssim(record, a, b, width, height, work=None, result=None, ssim_map=None, stream=None):
    """apt_film_ssim_device: the SSIM of the display luminances of the whole width x height images `a` and `b` (float32 [3][W*H], over
    record.passes_a and record.passes_b, times record.exposure, clipped) -> `result`, an int64 tensor of APT_SSIM_WORDS uint64 words
    (None: a new one), stored: the bits of the float64 tree sum of the windows' s, and the window count.  work: a float64 tensor of at
    least apt_film_ssim_work_bytes(width, height) / 8 elements (None: a new one).  ssim_map: None, or float32
    [(W - 10) * (H - 10)] that receives s.  Returns result; not synchronised."""
    require_gpu()
    n = width * height
    doubles = (_lib.metrics_lib().apt_film_ssim_work_bytes(width, height) + 7) // 8
    if work is None:
        work = torch.empty(max(doubles, 2), dtype=torch.float64, device=a.device)
    if result is None:
        result = torch.empty(_lib.APT_SSIM_WORDS, dtype=torch.int64, device=a.device)
    if work.numel() < doubles:
        raise _lib.AptError(f"work has {work.numel()} elements, expected at least {doubles}")
    windows = max(width - 10, 0) * max(height - 10, 0)
    _lib.metrics_check(_lib.metrics_lib().apt_film_ssim_device(
        ctypes.byref(record), _stream_handle(stream), _dev_f32(a, "a", 3 * n), _dev_f32(b, "b", 3 * n), width, height,
        _dev_words(work, "work", torch.float64), _dev_words(result, "result", torch.int64, _lib.APT_SSIM_WORDS),
        None if ssim_map is None else _dev_f32(ssim_map, "ssim_map", windows)), "apt_film_ssim_device")
    return result


def compare_summary(result, ssim_result=None):
    """The words of film_compare (and of film_ssim, or None) as numbers -> dict: mse, clipped_mse, rel_mse, mae (the sums over 3 *
    good in float64, nan when no pixel is good), psnr = 10 * log10(1 / clipped_mse), max_abs and max_index (the largest absolute
    difference of a channel and the first pixel that reaches it; nan and -1 when no pixel is good), bad (the excluded pixels), and ssim
    (the mean over the windows; None without ssim_result).  A device tensor is READ BACK: this synchronises torch's current stream."""
    import math

    import numpy as np

    def words(t, count):
        w = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        w = np.ascontiguousarray(w).view(np.uint64)
        if w.size != count:
            raise _lib.AptError(f"a result of {w.size} words, expected {count}")
        return w

    r = words(result, _lib.APT_COMPARE_WORDS)
    sums = r[:4].view(np.float64)
    key, bad, n = int(r[4]), int(r[5]), int(r[6])
    good = n - bad
    mean = [float(s) / (3 * good) if good else float("nan") for s in sums]
    out = {"mse": mean[0], "clipped_mse": mean[1], "rel_mse": mean[2], "mae": mean[3]}
    out["psnr"] = (10.0 * math.log10(1.0 / mean[1]) if mean[1] > 0 else float("inf")) if good else float("nan")
    out["max_abs"] = float(np.array([key >> 32], dtype=np.uint32).view(np.float32)[0]) if good else float("nan")
    out["max_index"] = 0xFFFFFFFF - (key & 0xFFFFFFFF) if good else -1
    out["bad"] = bad
    out["ssim"] = None
    if ssim_result is not None:
        s = words(ssim_result, _lib.APT_SSIM_WORDS)
        out["ssim"] = float(s[:1].view(np.float64)[0]) / int(s[1])
    return out


def film_upscale(record, lo, lo_features, lo_width, lo_height, hi_features, width, height, work=None, out=None, resolved=None, stream=None):
    """apt_film_upscale_device (libupscale_mi355x.so, include/render_mi355x_upscale.h): full-size radiance rebuilt from the low image --
    lo float32 [3][lo_width * lo_height], MEAN radiance, lo_features [APT_FEATURE_PLANES][lo_width * lo_height] -- under the guidance of
    hi_features [APT_FEATURE_PLANES][width * height] by `record` (_lib.film_upscale_record) -> (out float32 [3][width * height], mean
    radiance; resolved int32 [width * height], 0 where the fallback decided the pixel).  work: a float32 tensor of
    apt_film_upscale_work_floats(lo_width, lo_height) elements.  None: new tensors.  Not synchronised."""
    require_gpu()
    nl, n = lo_width * lo_height, width * height
    floats = _lib.upscale_lib().apt_film_upscale_work_floats(lo_width, lo_height)
    if work is None:
        work = torch.empty(max(floats, 4), dtype=torch.float32, device=lo.device)
    if out is None:
        out = torch.empty((3, n), dtype=torch.float32, device=lo.device)
    if resolved is None:
        resolved = torch.empty(n, dtype=torch.int32, device=lo.device)
    if work.numel() < floats:
        raise _lib.AptError(f"work has {work.numel()} elements, expected at least {floats}")
    _lib.upscale_check(_lib.upscale_lib().apt_film_upscale_device(
        ctypes.byref(record), _stream_handle(stream), _dev_f32(lo, "lo", 3 * nl), _dev_f32(lo_features, "lo_features", _lib.APT_FEATURE_PLANES * nl),
        lo_width, lo_height, _dev_f32(hi_features, "hi_features", _lib.APT_FEATURE_PLANES * n), width, height, _dev_f32(work, "work"),
        _dev_f32(out, "out", 3 * n), _dev_u32(resolved, "resolved", n)), "apt_film_upscale_device")
    return out, resolved


def film_upscale_patch(sums, pixel_list, list_count, passes, out, stream=None):
    """apt_film_upscale_patch_device: the pixels that the first list_count entries of pixel_list name, in `out` float32 [3][N], replaced
    by sums / passes -- sums: the compact planes of `passes` list passes added up (its first 3 * list_count floats, [3][list_count]).
    Returns out; not synchronised."""
    require_gpu()
    n = out.numel() // 3
    if sums.numel() < 3 * list_count or pixel_list.numel() < list_count:
        raise _lib.AptError("film_upscale_patch: sums or pixel_list is shorter than list_count asks")
    _lib.upscale_check(_lib.upscale_lib().apt_film_upscale_patch_device(
        _stream_handle(stream), _dev_f32(sums, "sums"), _dev_u32(pixel_list, "pixel_list"), list_count, passes, n, _dev_f32(out, "out", 3 * n)),
        "apt_film_upscale_patch_device")
    return out


class Upscaler:
    """Guided upscaling of a film rendered at lo_width x lo_height to width x height (include/render_mi355x_upscale.h): upscale()
    rebuilds full-size mean radiance from the low film's mean under the guidance of the full-size feature planes, unresolved() lists
    the pixels the guides found no agreeing tap for, refine() renders those at full resolution and patches them in.  Owns the work
    buffer, the output planes, the `resolved` words and what the list and the list passes need.  It never sets a camera: the context's
    camera and the params are the caller's, as everywhere."""

    def __init__(self, width, height, lo_width, lo_height, device="cuda", **record_fields):
        self.width, self.height, self.lo_width, self.lo_height = width, height, lo_width, lo_height
        self.record = _lib.film_upscale_record(**record_fields)
        n = width * height
        self._work = torch.empty(max(_lib.upscale_lib().apt_film_upscale_work_floats(lo_width, lo_height), 4), dtype=torch.float32, device=device)
        self.out = torch.empty((3, n), dtype=torch.float32, device=device)
        self.resolved = torch.empty(n, dtype=torch.int32, device=device)
        self.pixel_list = torch.empty(n, dtype=torch.int32, device=device)
        self._count = torch.zeros(1, dtype=torch.int32, device=device)
        self._select_work = torch.empty(_lib.adaptive_lib().apt_film_select_work_words(n), dtype=torch.int32, device=device)
        self._moments = torch.zeros((2, n), dtype=torch.float32, device=device)      # never read by the selection used here
        self._scratch = self._sums = None
        self.count = None                   # the length of pixel_list: None until unresolved() has run for the last upscale()

    def upscale(self, lo_mean, lo_features, hi_features, stream=None):
        """-> float32 [3][width * height] planes of MEAN radiance (the held output, written again by the next call) for
        Film.resolve(source=), Film.bloom(source=) and Film.compare(source=).  Not synchronised."""
        film_upscale(self.record, lo_mean, lo_features, self.lo_width, self.lo_height, hi_features, self.width, self.height, self._work,
                     self.out, self.resolved, stream)
        self.count = None
        return self.out

    def unresolved(self, stream=None):
        """-> (pixel_list int32 [N], count): the pixels of the last upscale() that the fallback decided, ascending, through the
        unchanged render.film_select (base_passes = 2, min_passes = max_passes = 3, `resolved` as `extra`).  Reads the count back (one
        4-byte copy): this synchronises `stream`."""
        rec = _lib.film_select_record(2, min_passes=3, max_passes=3)
        film_select(rec, self._moments, self.resolved, self._select_work, self.pixel_list, self._count, stream)
        with torch.cuda.stream(_torch_stream(stream)):
            self.count = int(self._count.cpu()[0])
        return self.pixel_list, self.count

    def refine(self, params, spheres, materials, passes=1, lights=None, first_pass=0, stream=None, context=None):
        """`passes` list passes (pass indices first_pass ..) of `params` at FULL resolution over the unresolved pixels, their mean
        patched into the held output -> how many pixels were rendered.  Each pass goes into a compact scratch (a list launch always
        stores) and is added to the sum with one fp32 add.  Calls unresolved() when it has not run since the last upscale()."""
        if (params.width, params.height) != (self.width, self.height):
            raise _lib.AptError("Upscaler.refine: params.width / height are not the full size")
        if passes < 1:
            raise _lib.AptError("Upscaler.refine: passes must be at least 1")
        if self.count is None:
            self.unresolved(stream)
        count = self.count
        if count == 0:
            return 0
        ctx = _default if context is None else context
        if self._scratch is None:
            self._scratch = torch.empty(3 * self.width * self.height, dtype=torch.float32, device=self.out.device)
            self._sums = torch.empty(3 * self.width * self.height, dtype=torch.float32, device=self.out.device)
        scratch, sums = self._scratch[:3 * count], self._sums[:3 * count]
        for k in range(passes):
            ctx.render_frame_film(params, spheres, materials, sums if k == 0 else scratch, first_pass + k, lights, 0, count, stream,
                                  pixel_list=self.pixel_list)
            if k:
                with torch.cuda.stream(_torch_stream(stream)):
                    sums.add_(scratch)
        film_upscale_patch(sums, self.pixel_list, count, passes, self.out, stream)
        return count


class History:
    """Temporal accumulation over the frames of a moving camera (include/render_mi355x_history.h): push(mean, features, camera) blends
    one more frame -- Film.mean() and Film.features() of a film rendered with `camera` -- into the history reprojected from the frame
    before.  Owns the two ping-pong history buffers, the previous features and the previous camera.  `frames`: how many were pushed
    since the last reset()."""

    def __init__(self, width, height, device="cuda", **record_fields):
        self.width, self.height = width, height
        self.record = _lib.film_history_record(**record_fields)
        self._hist = [torch.empty((6, width, height), dtype=torch.float32, device=device) for _ in range(2)]
        self._features = self._camera = None
        self.frames = 0

    def reset(self):
        """Forget the history: the next push is a first frame."""
        self.frames = 0
        self._features = self._camera = None

    def push(self, mean, features, camera=None, stream=None):
        """One more frame: mean float32 [3][N], features [APT_FEATURE_PLANES][N] (kept by reference until the next push: hand over a
        tensor that is not written again), camera an ApCamera (None: apt_camera_default_host's record, what a frame without a
        context camera is rendered from).  Returns self; not synchronised."""
        from . import gen_data
        cam = gen_data.default_camera(self.width, self.height) if camera is None else camera.copy()
        out = self._hist[self.frames & 1]
        prev = None if self.frames == 0 else (self._hist[(self.frames - 1) & 1], self._features, self._camera)
        film_history(self.record, mean, features, cam, out, prev, stream)
        self._features, self._camera = features, cam
        self.frames += 1
        return self

    @property
    def buffer(self):
        """The current history, float32 (6, width, height)."""
        if self.frames == 0:
            raise _lib.AptError("History: no frame was pushed")
        return self._hist[(self.frames - 1) & 1]

    def radiance(self):
        """The accumulated mean radiance, float32 [3][N]: a view of the current buffer; Film.resolve(source=...) takes it."""
        return self.buffer[:3].reshape(3, -1)

    def length(self):
        """The per-pixel history length, float32 [N]: a view."""
        return self.buffer[5].reshape(-1)

    def denoise_inputs(self, stream=None):
        """-> (film [3][N], moments [2][N]) for render.film_denoise with _lib.film_denoise_record(2) and the last pushed features."""
        return film_history_export(self.buffer, stream=stream)


class Film:
    """An unclipped float32 accumulation buffer for the pixels [pixel_begin, pixel_begin + pixel_count) of a width x height image
    (include/render_mi355x.h "film"): add_pass renders one more independent frame into it, resolve turns the mean into a displayable
    image.  `buffer` is the [3][count] tensor of sums, `passes` how many frames it holds.  moments=True (a whole image only) also
    keeps `moments`, the [2][count] sums of each pass's luminance and its square (include/render_mi355x_denoise.h), which denoise() needs: a
    pass is then rendered into a scratch film and added from there, to the same bits.  adaptive=True (needs moments=True) also keeps
    `extra`, int32 [count]: the passes each pixel received beyond `passes` through add_adaptive_pass (include/render_mi355x_adaptive.h),
    `rounds` of them so far; without it the film is what it was."""

    def __init__(self, width, height, pixel_begin=0, pixel_count=None, device="cuda", moments=False, adaptive=False):
        self.width, self.height, self.pixel_begin = width, height, pixel_begin
        self.pixel_count = width * height - pixel_begin if pixel_count is None else pixel_count
        if moments and (pixel_begin != 0 or self.pixel_count != width * height):
            raise _lib.AptError("Film: moments=True needs the whole image: the filter they serve has no band form")
        self.buffer = torch.zeros((3, self.pixel_count), dtype=torch.float32, device=device)
        self.moments = torch.zeros((2, self.pixel_count), dtype=torch.float32, device=device) if moments else None
        self._scratch = torch.empty((3, self.pixel_count), dtype=torch.float32, device=device) if moments else None
        self.passes = 0
        self._tables = {}
        if adaptive and not moments:
            raise _lib.AptError("Film: adaptive=True needs moments=True: the selection reads them")
        self.adaptive, self.rounds = bool(adaptive), 0
        self.extra = self.pixel_list = self._count = self._work = None
        if adaptive:
            n = self.pixel_count
            self.extra = torch.zeros(n, dtype=torch.int32, device=device)
            self.pixel_list = torch.empty(n, dtype=torch.int32, device=device)
            self._count = torch.zeros(1, dtype=torch.int32, device=device)
            self._work = torch.empty(_lib.adaptive_lib().apt_film_select_work_words(n), dtype=torch.int32, device=device)

    def reset(self):
        """Forget the passes: the next one stores, the moments too; an adaptive film forgets its rounds as well."""
        self.passes = 0
        self.rounds = 0
        if self.extra is not None:
            self.extra.zero_()

    def add_pass(self, params, spheres, materials, lights=None, stream=None, context=None):
        """One more frame of `params` (its width and height must be the film's), with pass index self.passes."""
        if (params.width, params.height) != (self.width, self.height):
            raise _lib.AptError("Film.add_pass: params.width / height are not the film's")
        if self.rounds:
            raise _lib.AptError("Film.add_pass: the film has had adaptive rounds, and pass index `passes` has been used by one: reset() first")
        ctx = _default if context is None else context
        if self.moments is None:
            ctx.render_frame_film(params, spheres, materials, self.buffer, self.passes, lights, self.pixel_begin, self.pixel_count, stream)
        else:
            # the pass by itself: a later pass ADDS, so it goes onto zeros (0 + r is r: a pass holds no -0); pass 0 stores
            if self.passes:
                with torch.cuda.stream(_torch_stream(stream)):
                    self._scratch.zero_()
            ctx.render_frame_film(params, spheres, materials, self._scratch, self.passes, lights, 0, self.pixel_count, stream)
            film_accumulate(self._scratch, self.buffer, self.moments, self.passes, stream)
        self.passes += 1
        return self

    def add_adaptive_pass(self, params, spheres, materials, lights=None, stream=None, context=None, **select_fields):
        """One adaptive round -> how many pixels it rendered.  Select (apt_film_select_default_host's record for `passes`, with any of
        min_passes, max_passes, threshold, floor replaced) the pixels whose mean luminance is still uncertain, read their number back
        (one 4-byte copy: this synchronises `stream`), render them as a list pass with pass index passes + rounds -- to the bits a whole
        pass of that index would give them -- and add it to the film, the moments and `extra`.  `rounds` advances even when nothing
        was selected.  The film needs adaptive=True and at least 2 passes; `pixel_list` then holds the round's list."""
        if not self.adaptive:
            raise _lib.AptError("Film.add_adaptive_pass: the film was not made with adaptive=True")
        if self.passes < 2:
            raise _lib.AptError("Film.add_adaptive_pass: the variance of the mean needs at least 2 uniform passes")
        if (params.width, params.height) != (self.width, self.height):
            raise _lib.AptError("Film.add_adaptive_pass: params.width / height are not the film's")
        ctx = _default if context is None else context
        rec = _lib.film_select_record(self.passes, **select_fields)
        film_select(rec, self.moments, self.extra, self._work, self.pixel_list, self._count, stream)
        with torch.cuda.stream(_torch_stream(stream)):
            count = int(self._count.cpu()[0])
        if count:
            scratch = self._scratch.view(-1)[:3 * count]
            ctx.render_frame_film(params, spheres, materials, scratch, self.passes + self.rounds, lights, 0, count, stream,
                                  pixel_list=self.pixel_list)
            film_accumulate_list(scratch, self.pixel_list, count, self.buffer, self.moments, self.extra, stream)
        self.rounds += 1
        return count

    def denoise(self, params, spheres, iterations=None, features=None, stream=None, context=None, **sigmas):
        """The film's mean through apt_film_denoise_device -> float32 [3][count], the denoised mean radiance; resolve(source=...)
        makes an image of it.  The film needs moments=True and at least 2 passes.  iterations and sigma_n, sigma_z, sigma_c, sigma_a,
        sigma_l, albedo_floor replace apt_film_denoise_default_host's values.  features: the film's feature planes (None: rendered
        through Film.features with `params` and `spheres`)."""
        if self.moments is None:
            raise _lib.AptError("Film.denoise: the film keeps no moments (Film(..., moments=True))")
        if self.passes < 2:
            raise _lib.AptError("Film.denoise: the variance of the mean needs at least 2 passes")
        if self.rounds and bool(self.extra.any()):
            raise _lib.AptError("Film.denoise: pixels of the film hold extra adaptive passes, and the filter divides by ONE pass count")
        if features is None:
            features = self.features(params, spheres, stream, context)
        rec = _lib.film_denoise_record(self.passes, iterations, **sigmas)
        return film_denoise(rec, self.buffer, self.moments, features, self.width, self.height, stream=stream)

    def features(self, params, spheres, stream=None, context=None):
        """apt_render_frame_features for the film's own pixel range (params.width and height must be the film's) -> a new float32
        [APT_FEATURE_PLANES][count] tensor: what lies under the film's pixels.  Independent of the passes the film holds."""
        if (params.width, params.height) != (self.width, self.height):
            raise _lib.AptError("Film.features: params.width / height are not the film's")
        out = torch.empty((_lib.APT_FEATURE_PLANES, self.pixel_count), dtype=torch.float32, device=self.buffer.device)
        return (_default if context is None else context).render_frame_features(params, spheres, out, self.pixel_begin,
                                                                                self.pixel_count, stream)

    def mean(self):
        """The film divided by its passes (fp32, as the resolve's first step) -> float32 [3][count]."""
        if self.passes == 0:
            raise _lib.AptError("Film.mean: the film holds no pass")
        if self.rounds:
            return film_mean(self.buffer, self.passes, self.extra)
        return self.buffer / torch.tensor(self.passes, dtype=torch.float32, device=self.buffer.device)

    def resolve(self, exposure=1.0, tonemap="clip", white=None, curve="srgb", want_float=False, stream=None, source=None):
        """apt_film_resolve_device: mean, exposure, tone operator ("clip" or "reinhard"; white: the radiance that maps to 1, None:
        plain Reinhard) and the 8-bit encoding by `curve` ("srgb" or "linear") -> u8 [count][3], or (u8, float32 [3][count]).
        source: planes of MEAN radiance [3][count] to resolve in the film's place, with passes = 1: what denoise() returns."""
        from . import gen_data
        if source is None and self.passes == 0:
            raise _lib.AptError("Film.resolve: the film holds no pass")
        tm = {"clip": _lib.APT_TONEMAP_CLIP, "reinhard": _lib.APT_TONEMAP_REINHARD}.get(tonemap)
        if tm is None:
            raise _lib.AptError(f"Film.resolve: unknown tone operator {tonemap!r}")
        if curve not in self._tables:
            self._tables[curve] = torch.from_numpy(gen_data.film_curve(curve)).to(self.buffer.device)
        if source is None and self.rounds:   # every pixel over its own pass count first: then a source of mean radiance like any other
            source = film_mean(self.buffer, self.passes, self.extra, stream=stream)
        rec = _lib.film_resolve_record(self.passes if source is None else 1, exposure, tm,
                                       0.0 if white is None else 1.0 / (float(white) * float(white)))
        film = _dev_f32(self.buffer, "film") if source is None else _dev_f32(source, "source", 3 * self.pixel_count)
        u8 = torch.empty((self.pixel_count, 3), dtype=torch.uint8, device=self.buffer.device)
        out = torch.empty((3, self.pixel_count), dtype=torch.float32, device=self.buffer.device) if want_float else None
        check(lib().apt_film_resolve_device(ctypes.byref(rec), _stream_handle(stream), film, self.pixel_count,
                                            _dev_f32(self._tables[curve], "table", 256), None if out is None else out.data_ptr(),
                                            u8.data_ptr()), "apt_film_resolve_device")
        return (u8, out) if want_float else u8

    def _post_source(self, source, what, stream=None):
        """-> (planes, passes) that the post entries read: `source` as MEAN radiance, or the film's own sums and pass count."""
        if source is not None:
            return source, 1
        if self.passes == 0:
            raise _lib.AptError(f"Film.{what}: the film holds no pass")
        if self.rounds:                      # every pixel over its own pass count first, as resolve does
            return film_mean(self.buffer, self.passes, self.extra, stream=stream), 1
        return self.buffer, self.passes

    def auto_exposure(self, source=None, prev=1.0, **fields):
        """The exposure metered from the film (include/render_mi355x_post.h): film_meter, then film_exposure with `prev`, the last
        frame's exposure -> float, for resolve(exposure=...).  source: planes of MEAN radiance [3][count] to meter in the film's place,
        with passes = 1: what denoise(), bloom() or History.radiance() return.  low_q, high_q, key, min_exposure, max_exposure and
        adapt replace apt_film_meter_default_host's values.  Reads the histogram back: synchronises torch's current stream."""
        planes, passes = self._post_source(source, "auto_exposure")
        rec = _lib.film_meter_record(passes, **fields)
        return film_exposure(rec, film_meter(rec, planes), prev)

    def bloom(self, source=None, stream=None, **fields):
        """The film's mean plus its glare through apt_film_bloom_device -> float32 [3][count] planes of MEAN radiance for
        resolve(source=..., exposure=...).  source: as auto_exposure's.  levels, threshold, cap, spread and intensity replace
        apt_film_bloom_default_host's values.  A whole image only: the pyramid has no band form."""
        if self.pixel_begin != 0 or self.pixel_count != self.width * self.height:
            raise _lib.AptError("Film.bloom: the film is a band of the image")
        planes, passes = self._post_source(source, "bloom", stream)
        return film_bloom(_lib.film_bloom_record(passes, **fields), planes, self.width, self.height, stream=stream)

    def compare(self, reference, exposure=1.0, eps=1e-2, ssim=True, source=None):
        """How far the film is from `reference` (include/render_mi355x_metrics.h) -> compare_summary's dict: mse, clipped_mse, rel_mse,
        mae, psnr, max_abs, max_index, bad, ssim.  reference: a Film of the same pixel range, or planes of MEAN radiance [3][count]
        (passes = 1).  source: planes of MEAN radiance to compare in the film's place, as auto_exposure's.  exposure multiplies the means
        before the clipped error and SSIM clip them to [0, 1]; eps is what the relative error adds to the squared reference.  ssim=True
        needs a whole image (the windows have no band form); ssim=False leaves "ssim" None and takes a band.  Reads the words back:
        synchronises torch's current stream."""
        whole = self.pixel_begin == 0 and self.pixel_count == self.width * self.height
        if ssim and not whole:
            raise _lib.AptError("Film.compare: the film is a band of the image (ssim=False compares a band)")
        planes, passes = self._post_source(source, "compare")
        if isinstance(reference, Film):
            if (reference.pixel_begin, reference.pixel_count) != (self.pixel_begin, self.pixel_count):
                raise _lib.AptError("Film.compare: the reference film covers other pixels")
            ref, ref_passes = reference._post_source(None, "compare")
        else:
            ref, ref_passes = reference, 1
        rec = _lib.film_compare_record(passes, ref_passes, exposure=exposure, eps=eps)
        words = film_compare(rec, planes, ref)
        ssim_words = film_ssim(rec, planes, ref, self.width, self.height) if ssim else None
        return compare_summary(words, ssim_words)

    def write_pfm(self, path):
        """apt_write_pfm of the mean; the film must cover the whole image."""
        if self.pixel_begin != 0 or self.pixel_count != self.width * self.height:
            raise _lib.AptError("Film.write_pfm: the film is a band of the image")
        planes = self.mean().cpu().numpy()
        check(lib().apt_write_pfm(str(path).encode(), self.width, self.height, planes.ctypes.data), "apt_write_pfm")


def gen_rays_device(params: RenderParams, stream=None, device="cuda"):
    """Device gen_rays with the counter-based generator -> [6][N] tensor."""
    require_gpu()
    rays = torch.empty(6 * params.num_paths, dtype=torch.float32, device=device)
    check(lib().apt_gen_rays_device(ctypes.byref(params), _stream_handle(stream), _dev_f32(rays, "rays")),
          "apt_gen_rays_device")
    return rays.view(6, -1)


def gen_rays_camera(params: RenderParams, cam, stream=None, device="cuda"):
    """apt_gen_rays_camera_device: the rays of camera `cam` (its lens included) -> [6][N] tensor, or [6][path_count] with
    APT_FLAG_BAND_BUFFERS; only paths [path_begin, path_begin + path_count) are written.  The rays a material frame traces with `cam` set."""
    require_gpu()
    n = _buffer_paths(params)
    rays = torch.empty(6 * n, dtype=torch.float32, device=device)
    check(lib().apt_gen_rays_camera_device(ctypes.byref(params), ctypes.byref(cam), _stream_handle(stream), _dev_f32(rays, "rays")),
          "apt_gen_rays_camera_device")
    return rays.view(6, -1)


def decode_color_device(params: RenderParams, colors, stream=None):
    """Device decode_color: colours [3][N] -> (fb float32 [3][W*H], fb_u8 [W*H][3])."""
    require_gpu()
    npix = params.width * params.height
    fb = torch.empty((3, npix), dtype=torch.float32, device=colors.device)
    u8 = torch.empty((npix, 3), dtype=torch.uint8, device=colors.device)
    check(lib().apt_decode_color_device(ctypes.byref(params), _stream_handle(stream),
                                        _dev_f32(colors.reshape(-1), "colors", 3 * params.num_paths), fb.data_ptr(), u8.data_ptr()),
          "apt_decode_color_device")
    return fb, u8


class TraceCounter:
    """Optional device counter of traced ray segments (for reporting under APT_FLAG_RETIRE)."""

    def __init__(self, device="cuda"):
        self.buf = torch.zeros(4, dtype=torch.int64, device=device)  # [0] segments, [1..2] refill statistics

    def __enter__(self):
        self.buf.zero_()
        lib().apt_set_trace_counter(self.buf.data_ptr())
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        lib().apt_set_trace_counter(None)

    @property
    def value(self):
        return int(self.buf[0].item())

    @property
    def stats(self):
        """(traced segments, lane-slots spent in bounce executions, lane-slots spent in ray-generate) --
        the last two only from the refill loop of render_frame with APT_FLAG_RETIRE; for scenes behind a grid
        they are (cells visited, candidates tested) instead."""
        return tuple(int(x) for x in self.buf[:3].tolist())

    @property
    def exact_reruns(self):
        """Wave-level exact re-runs of a bounce (fast sqrt/divide sequences outside their validity range)."""
        return int(self.buf[3].item())


def selftest_sqrt(variant=0, first_bits=0, count=1 << 32, stream=None):
    """Exhaustive check of the hot loop's fast sqrt against sqrtf(): -> (mismatches, first bad bits)."""
    require_gpu()
    res = torch.tensor([0, -1], dtype=torch.int64, device="cuda")
    check(lib().apt_selftest_sqrt(variant, _stream_handle(stream), first_bits, count, res.data_ptr()), "apt_selftest_sqrt")
    torch.cuda.synchronize()
    bad, first = res.tolist()
    return bad, first & 0xFFFFFFFF


def selftest_div3(first=0, count=1 << 32, stream=None):
    """Shared-reciprocal divide vs `/` on hashed operand sets: -> (mismatches, first bad, accepted)."""
    require_gpu()
    res = torch.tensor([0, -1, 0], dtype=torch.int64, device="cuda")
    check(lib().apt_selftest_div3(_stream_handle(stream), first, count, res.data_ptr()), "apt_selftest_div3")
    torch.cuda.synchronize()
    return tuple(res.tolist())


def selftest_div3_seeded(part=0, first=0, count=1 << 32, stream=None):
    """The two-path bounce's seeded divide vs `/` (include/render_mi355x.h apt_selftest_div3_seeded; part 0: apt_selftest_div3's operand
    sets, 1: every len2 bit pattern, 2: one divisor against every numerator mantissa): -> dict(bad, first, accepted, flagged,
    flagged_other, in_range, shared_ok, recip_off)."""
    require_gpu()
    res = torch.tensor([0, -1, 0, 0, 0, 0, 0, 0], dtype=torch.int64, device="cuda")
    check(lib().apt_selftest_div3_seeded(_stream_handle(stream), part, first, count, res.data_ptr()), "apt_selftest_div3_seeded")
    torch.cuda.synchronize()
    return dict(zip(("bad", "first", "accepted", "flagged", "flagged_other", "in_range", "shared_ok", "recip_off"), res.tolist()))


def selftest_direction(d3, flags=False, stream=None):
    """Ray-generate's fast direction with the device's own v_rsq_f64 against its exact form, on the float64 vectors d3 [n, 3] (a CUDA
    tensor): -> dict(accepted, rejected, bad, ray_rejected, max_cert), with flags=True also the per-vector flag bytes (numpy).
    `bad` counts accepted components that differ from the exact form: it must be 0."""
    require_gpu()
    assert d3.is_cuda and d3.dtype == torch.float64 and d3.dim() == 2 and d3.shape[1] == 3 and d3.is_contiguous()
    res = torch.zeros(5, dtype=torch.int64, device="cuda")
    fl = torch.zeros(d3.shape[0], dtype=torch.uint8, device="cuda") if flags else None
    check(lib().apt_selftest_direction(_stream_handle(stream), d3.data_ptr(), d3.shape[0], res.data_ptr(),
                                       fl.data_ptr() if flags else None), "apt_selftest_direction")
    torch.cuda.synchronize()
    r = res.cpu()
    out = dict(accepted=int(r[0]), rejected=int(r[1]), bad=int(r[2]), ray_rejected=int(r[3]), max_cert=float(r[4:5].view(torch.float64)[0]))
    return (out, fl.cpu().numpy()) if flags else out


def set_refill_lanes(lanes):
    """Compaction batch threshold (1..64, default 32); speed only, results do not depend on it."""
    _default.set_refill_lanes(lanes)


def test_scene(params: RenderParams, rays, spheres, stream=None):
    """First-hit debug mode (scripts/gen_data.py:134-188 test_scene) -> [3][N] tensor."""
    require_gpu()
    n = params.num_paths
    out = torch.empty(3 * n, dtype=torch.float32, device=rays.device)
    check(lib().apt_test_scene(ctypes.byref(params), _stream_handle(stream), _dev_f32(rays, "rays", 6 * n),
                               _dev_f32(spheres, "spheres", sphere_floats(params.num_spheres)),
                               _dev_f32(out, "out")), "apt_test_scene")
    return out.view(3, -1)


MT_GROUP_PIXELS = 78     # pixels per workgroup of the fused MT19937 frame kernel: 78 * 4 * S paths = 2 S generator blocks


def mt_group_checkpoints(w, h, s, seed=0, pixel_begin=0, pixel_count=None, mt_state=None):
    """Host-made generator states for render_reference_frame_fused(): -> (uint32 [groups][624], first_group).  One raw MT19937
    state per group of 78 pixels (block g * 2 S); mt_state = (block, raw state of that block) starts a far window without walking
    the stream from the seed."""
    import numpy as np
    from . import gen_data
    npix = w * h
    if pixel_count is None:
        pixel_count = npix - pixel_begin
    g_lo, g_hi = pixel_begin // MT_GROUP_PIXELS, (pixel_begin + pixel_count + MT_GROUP_PIXELS - 1) // MT_GROUP_PIXELS
    state = None
    if mt_state is not None:
        blk, raw = mt_state
        if blk > g_lo * 2 * s:
            raise _lib.AptError("mt_state lies after the first block requested")
        state = (np.array(raw, dtype=np.uint32) if blk == g_lo * 2 * s
                 else gen_data.mt19937_checkpoints_window(blk, g_lo * 2 * s - blk, seed, 1 << 30, raw)[1])
    ck, _ = gen_data.mt19937_checkpoints_window(g_lo * 2 * s, (g_hi - g_lo) * 2 * s, seed, 2 * s, state)
    return ck, g_lo


def render_reference_frame_fused(w, h, s, depth=5, seed=0, spheres=None, mode=None, flags=0, stream=None, pixel_begin=0,
                                 pixel_count=None, checkpoints=None, mt_state=None):
    """The reference's whole pipeline (np.random.seed(seed); gen_rays; test_soa arithmetic; decode_color) in ONE launch, with no
    ray / colour buffers in HBM (apt_render_frame_mt): -> (fb float32 [3][pixel_count], fb_u8 [pixel_count][3]), not synchronised;
    bit-identical to render_reference_frame().  Any sample count with a pairwise-sum plan (every s <= 7688; the reference's default is
    16 x 16, s = 1).  checkpoints = (device int32 tensor [groups][624], first_group) from mt_group_checkpoints() to reuse a table."""
    import numpy as np
    from . import gen_data
    from ._lib import APT_MODE_ORACLE, make_params
    require_gpu()
    if spheres is None:
        spheres = torch.from_numpy(gen_data.gen_spheres()).cuda()
    npix = w * h
    if pixel_count is None:
        pixel_count = npix - pixel_begin
    # Everything this call allocates -- the generator states it uploads, the frame buffers -- is allocated and filled ON the stream the
    # kernel runs on (a caller's side stream included), so the upload is ordered before the launch and the caching allocator does not
    # hand the table to another stream while the kernel still reads it (the cross-stream lifetime hazard fixed for
    # render_reference_frame in round 3).
    caller = torch.cuda.current_stream()    # the stream a caller's own table was uploaded on (read BEFORE the `with` below changes it)
    tstream = caller if stream is None else (torch.cuda.ExternalStream(stream) if isinstance(stream, int) else stream)
    with torch.cuda.stream(tstream):
        if checkpoints is None:
            ck, g_lo = mt_group_checkpoints(w, h, s, seed, pixel_begin, pixel_count, mt_state)
            checkpoints = (torch.from_numpy(ck.view(np.int32)).cuda(), g_lo)
        else:
            # a caller's table, made on the caller's current stream: this launch must come after its upload (ordering) and the
            # allocator must not recycle it before the launch is through (lifetime) -- both matter when `stream` is a side stream.
            # (Round 5 waited on torch.cuda.current_stream() INSIDE the `with`: that is tstream itself, a wait on nothing.)
            tstream.wait_stream(caller)
        ck_d, g_lo = checkpoints
        ck_d.record_stream(tstream)
        p = make_params(w, h, s, depth=depth, mode=APT_MODE_ORACLE if mode is None else mode, flags=flags)
        fb = torch.empty((3, pixel_count), dtype=torch.float32, device="cuda")
        u8 = torch.empty((pixel_count, 3), dtype=torch.uint8, device="cuda")
    check(lib().apt_render_frame_mt(ctypes.byref(p), _stream_handle(tstream), ck_d.data_ptr(), ck_d.shape[0], g_lo,
                                    _dev_f32(spheres, "spheres"), pixel_begin, pixel_count, fb.data_ptr(), u8.data_ptr()),
          "apt_render_frame_mt")
    return fb, u8


def render_reference_frame(w, h, s, depth=5, seed=0, spheres=None, mode=None, flags=0, stream=None, band_pixels=None,
                           pixel_begin=0, pixel_count=None, mt_state=None):
    """The reference's whole pipeline on the device, bit-exact with running scripts/gen_data.py
    (np.random.seed(seed); gen_rays; gen_spheres; test_soa) and scripts/data_visualization.py:
    MT19937 gen_rays -> render (O-mode by default = the NumPy oracle's arithmetic) -> decode_color.

    band_pixels=None: three whole-frame launches with [6][N] / [3][N] intermediates (36 bytes per path: 19 GB at C2)
        -> (fb float32 [3][W*H], fb_u8 uint8 [W*H][3], colors [3][N]); not synchronised.
    band_pixels=B: the same pipeline band by band in band-relative buffers (APT_FLAG_BAND_BUFFERS) of B pixels
        (36*4*S*B bytes, e.g. 604 MB for B = 65536 at S = 64), for pixels [pixel_begin, pixel_begin+pixel_count)
        -> (fb [3][pixel_count], fb_u8 [pixel_count][3], None).  The MT19937 checkpoints are made window by
        window on the host (chained); mt_state = (block, raw uint32[624] state of that block) lets a far window start
        without walking the stream from the seed (C3's last band is 1.1e8 blocks in)."""
    import numpy as np
    from . import gen_data
    from ._lib import APT_FLAG_BAND_BUFFERS, APT_MODE_ORACLE, make_params
    require_gpu()
    if spheres is None:
        spheres = torch.from_numpy(gen_data.gen_spheres()).cuda()
    mode = APT_MODE_ORACLE if mode is None else mode
    if band_pixels is None:
        p = make_params(w, h, s, depth=depth, mode=mode, flags=flags)
        rays = gen_data.gen_rays_device(w, h, s, seed=seed, stream=stream)
        colors = render_paths(p, rays.reshape(-1), spheres, stream=stream)
        fb, u8 = decode_color_device(p, colors, stream=stream)
        return fb, u8, colors
    npix = w * h
    if pixel_count is None:
        pixel_count = npix - pixel_begin
    per_pixel, stride = 4 * s, 64
    fb = torch.empty((3, pixel_count), dtype=torch.float32, device="cuda")
    u8 = torch.empty((pixel_count, 3), dtype=torch.uint8, device="cuda")
    rays = torch.empty(6 * band_pixels * per_pixel, dtype=torch.float32, device="cuda")
    colors = torch.empty(3 * band_pixels * per_pixel, dtype=torch.float32, device="cuda")
    # Everything of a band -- the three launches, the copy of its pixels into `fb` and the wait before its buffers are reused --
    # runs on ONE stream: torch's current stream inside the `with` below (a caller's side stream included; before round 3 the copy
    # and the wait used the current stream while the launches used `stream`).
    tstream = torch.cuda.current_stream() if stream is None else (torch.cuda.ExternalStream(stream) if isinstance(stream, int) else stream)
    st = _stream_handle(tstream)
    state_blk, state = (None, None) if mt_state is None else mt_state

    def advance(raw, blk_from, blk_to):     # raw state of block blk_from -> raw state of block blk_to (host, sequential)
        if blk_to == blk_from:
            return np.array(raw, dtype=np.uint32)
        return gen_data.mt19937_checkpoints_window(blk_from, blk_to - blk_from, seed, 1 << 30, raw)[1]

    for q0 in range(pixel_begin, pixel_begin + pixel_count, band_pixels):
        nq = min(band_pixels, pixel_begin + pixel_count - q0)
        b, c = q0 * per_pixel, nq * per_pixel
        blk0, blk1 = b // 156, (b + c + 155) // 156
        if state_blk is not None and state_blk > blk0:
            raise _lib.AptError("mt_state lies after the first path requested")
        if state_blk is not None and state_blk < blk0:      # walk the stored state forward to this band (host, sequential)
            state, state_blk = advance(state, state_blk, blk0), blk0
        ck, nxt = gen_data.mt19937_checkpoints_window(blk0, blk1 - blk0, seed, stride, state if state_blk == blk0 else None)
        # the window's end state is the raw state of block blk1; the next band starts at block (b + c) // 156 = blk1 or blk1 - 1
        # (a band boundary inside a block), so keep the state of the LAST block of this window instead when they overlap
        with torch.cuda.stream(tstream):                    # the upload is ordered before the launch that reads it
            ck_d = torch.from_numpy(ck.view(np.int32)).cuda()
            fb_band = torch.empty((3, nq), dtype=torch.float32, device="cuda")
        p = make_params(w, h, s, depth=depth, mode=mode, flags=flags | APT_FLAG_BAND_BUFFERS, path_begin=b, path_count=c)
        check(lib().apt_gen_rays_mt_device_ex(ctypes.byref(p), st, ck_d.data_ptr(), stride, ck.shape[0], blk0, rays.data_ptr()),
              "apt_gen_rays_mt_device_ex")
        check(lib().render_do_ex(ctypes.byref(p), st, rays.data_ptr(), _dev_f32(spheres, "spheres"), colors.data_ptr()), "render_do_ex")
        o = q0 - pixel_begin
        check(lib().apt_decode_color_band(ctypes.byref(p), st, colors.data_ptr(), nq, fb_band.data_ptr(), u8[o:o + nq].data_ptr()),
              "apt_decode_color_band")
        with torch.cuda.stream(tstream):
            fb[:, o:o + nq] = fb_band
        tstream.synchronize()                               # the checkpoint table of this band may now be freed / rays reused
        state_blk, state = blk1, nxt
        if (b + c) % 156:                                    # the next band starts inside block blk1 - 1: re-derive from this window's table
            last_cp = (blk1 - 1 - blk0) // stride
            state, state_blk = advance(ck[last_cp], blk0 + last_cp * stride, blk1 - 1), blk1 - 1
    return fb, u8, None
