"""Host-side input writers, the counterpart of the reference's scripts/gen_data.py:
gen_rays (:21-75), gen_spheres (:92-132).  The arithmetic runs in librender_mi355x.so
(apt_gen_rays_host / apt_gen_spheres_host / apt_gen_scene_host); outputs are bit-identical
to the reference's rays.bin / spheres.bin for the same (w, h, s, seed)."""
import ctypes
import os

import numpy as np

from ._lib import AptError, check, lib

width, height, samples = 16, 16, 1      # gen_data.py:6-8
eps, bounceMax = 1e-4, 5                # gen_data.py:9-10


def _fptr(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def gen_rays(w, h, s, seed=0, out_dir=None):
    """-> float32 [6][N] planes ox,oy,oz,dx,dy,dz; writes <out_dir>/rays.bin when given
    (the reference always writes ./input/rays.bin, gen_data.py:71)."""
    n = w * h * 4 * s
    rays = np.empty(6 * n, dtype=np.float32)
    check(lib().apt_gen_rays_host(w, h, s, seed, _fptr(rays)), "apt_gen_rays_host")
    if out_dir is not None:
        rays.tofile(os.path.join(out_dir, "rays.bin"))
    return rays.reshape(6, n)


def mt19937_checkpoints(num_paths, seed=0, stride=64):
    """Host-made MT19937 checkpoints for gen_rays_device(): uint32 [ceil(blocks/stride)][624]."""
    blocks = (num_paths + 155) // 156
    n = (blocks + stride - 1) // stride
    states = np.empty((n, 624), dtype=np.uint32)
    check(lib().apt_mt19937_checkpoints_host(seed, blocks, stride, states.ctypes.data), "apt_mt19937_checkpoints_host")
    return states


def mt19937_checkpoints_window(first_block, num_blocks, seed=0, stride=64, state_in=None):
    """Checkpoints of output blocks first_block + k*stride (k < ceil(num_blocks/stride)) -> (uint32 [n][624], raw state
    of block first_block + num_blocks).  state_in = raw state of block first_block (chains windows, or a stored state);
    None walks there from the seed (first_block + 1 sequential twists)."""
    n = (num_blocks + stride - 1) // stride
    states = np.empty((n, 624), dtype=np.uint32)
    out = np.empty(624, dtype=np.uint32)
    st = None if state_in is None else np.ascontiguousarray(state_in, dtype=np.uint32)
    check(lib().apt_mt19937_checkpoints_window(None if st is None else st.ctypes.data, seed, first_block, num_blocks, stride,
                                               states.ctypes.data, out.ctypes.data), "apt_mt19937_checkpoints_window")
    return states, out


def gen_rays_device(w, h, s, seed=0, stride=64, checkpoints=None, stream=None):
    """gen_rays on the GPU, bit-exact with the reference (np.random.seed(seed) MT19937 stream):
    -> torch float32 [6][N] on the device.  `checkpoints` (a CUDA int32/uint32 tensor from
    mt19937_checkpoints) can be passed to reuse a table."""
    import torch
    from . import render
    from ._lib import make_params, require_gpu
    require_gpu()
    p = make_params(w, h, s)
    if checkpoints is None:
        checkpoints = torch.from_numpy(mt19937_checkpoints(p.num_paths, seed, stride).view(np.int32)).cuda()
    rays = torch.empty(6 * p.num_paths, dtype=torch.float32, device="cuda")
    check(lib().apt_gen_rays_mt_device(ctypes.byref(p), render._stream_handle(stream), checkpoints.data_ptr(), stride,
                                       checkpoints.shape[0], rays.data_ptr()), "apt_gen_rays_mt_device")
    return rays.view(6, -1)


def gen_spheres(out_dir=None):
    """-> the 128-float (512-byte) [10][8] table; writes <out_dir>/spheres.bin when given."""
    sph = np.zeros(128, dtype=np.float32)
    check(lib().apt_gen_spheres_host(_fptr(sph)), "apt_gen_spheres_host")
    if out_dir is not None:
        sph.tofile(os.path.join(out_dir, "spheres.bin"))
    return sph


def gloss(alpha):
    """The material word of a rough-metal sphere (APT_MAT_GLOSS_WORD; needs APT_FLAG_GLOSS in the launch's flags): GGX roughness alpha
    in steps of 2^-16, q = round(alpha * 65536) clamped to [1, 65535].  alpha -> 0 tends to MAT_SPEC, alpha 0.5 is satin.  Pure Python."""
    from ._lib import MAT_GLOSS
    q = min(65535, max(1, int(round(float(alpha) * 65536.0))))
    return MAT_GLOSS | (q << 8)


_gloss_word = gloss     # (gen_spheres_materials has an argument of that name)


def materials_flags(table, mis=False):
    """apt_materials_flags_host: the flags a material table earns -- APT_FLAG_GLOSS when it holds a well-formed gloss word, else 0.
    `table`: the host array of codes (gen_spheres_materials / gen_scene_materials).  OR the result into make_params(flags=).
    mis=True: APT_FLAG_MIS as well, when -- and only when -- the table earns APT_FLAG_GLOSS: the rough-metal hits then sample the lights
    too (multiple importance sampling, balance heuristic), which is what makes the highlight of a small lamp converge.  The launch reads
    the bit next to APT_FLAG_NEE or a light table only; render_frame, render_do_ex, Film.add_pass and render_frame_film take it in
    params.flags like every other flag."""
    from ._lib import APT_FLAG_MIS
    t = np.ascontiguousarray(np.asarray(table).astype(np.int64) & 0xFFFFFFFF, dtype=np.uint32).ravel()
    flags = int(lib().apt_materials_flags_host(t.ctypes.data, t.size))
    return flags | (APT_FLAG_MIS if mis and flags else 0)


def gen_spheres_materials(gloss=None):
    """The material entries' demo scene (apt_gen_spheres_materials_host): gen_spheres' eight spheres plus smallpt's glass ball as
    sphere 8 -> (spheres float32 [128] = [10][9] planes zero padded, materials int32 [9] of MAT_* codes; light index 7).
    gloss=alpha: the mirror ball (sphere 6) is a rough-metal ball of that roughness instead (render with APT_FLAG_GLOSS)."""
    sph = np.zeros(128, dtype=np.float32)
    mat = np.zeros(9, dtype=np.uint32)
    check(lib().apt_gen_spheres_materials_host(_fptr(sph), mat.ctypes.data), "apt_gen_spheres_materials_host")
    if gloss is not None:
        mat[6] = _gloss_word(gloss)
    return sph, mat.view(np.int32)


def gen_scene_materials(num_spheres, seed=0):
    """gen_scene(num_spheres, seed) and the material codes that go with it (apt_gen_scene_materials_host, the same seed): walls and
    light MAT_DIFF, every small sphere one of the three codes -> (spheres float32 zero-padded [10][Ns], materials int32 [Ns])."""
    mat = np.zeros(num_spheres, dtype=np.uint32)
    check(lib().apt_gen_scene_materials_host(num_spheres, seed, mat.ctypes.data), "apt_gen_scene_materials_host")
    return gen_scene(num_spheres, seed), mat.view(np.int32)


def with_lamp(spheres, num_spheres, light_index, radius=1.5, centre=(50.0, 81.6 - 16.5, 81.6), emission=400.0):
    """A copy of a [10][Ns] sphere table (gen_spheres, gen_spheres_materials, gen_scene: zero padded or not) whose sphere `light_index`
    is smallpt's explicit lamp: radius 1.5 at (50, 81.6 - 16.5, 81.6), emission 400 per channel, albedo 0.  A light this small is what
    APT_FLAG_NEE is for.  r -> r^2 in float64 and one rounding to float32, as gen_spheres stores it.  Build a grid from the returned
    table, not from the original: the lamp is then binned in cells instead of sitting in the always-tested list.  Pure Python."""
    ns = int(num_spheres)
    if not 0 <= int(light_index) < ns:
        raise AptError("with_lamp: light_index %d is not a sphere of a %d-sphere table" % (light_index, ns))
    out = np.array(spheres, dtype=np.float32).ravel()
    if out.size < 10 * ns:
        raise AptError("with_lamp: the table holds fewer than 10 * num_spheres floats")
    em = (emission,) * 3 if np.isscalar(emission) else tuple(emission)
    record = (float(radius) ** 2, *centre, *em, 0.0, 0.0, 0.0)
    planes = out[:10 * ns].reshape(10, ns)       # a view: writes go to `out`
    planes[:, int(light_index)] = np.array(record, dtype=np.float64).astype(np.float32)
    return out


def with_lamps(spheres, num_spheres, indices, radius=1.5, centres=None, emission=400.0):
    """with_lamp for several spheres at once: a copy of the table whose spheres `indices` are lamps.  radius / emission: one value for
    all, or a list with one per lamp (each emission a number or an (r, g, b) triple, so colours may differ per lamp); centres: one (x, y, z)
    per lamp, or None = every sphere keeps the centre it has.  As with with_lamp, build grids and light tables from the returned
    table.  Pure Python."""
    idx = [int(i) for i in indices]
    n = len(idx)
    if len(set(idx)) != n:
        raise AptError("with_lamps: a sphere is listed twice")
    per = lambda v: [v] * n if np.isscalar(v) else list(v)
    radii, ems = per(radius), per(emission)
    if len(radii) != n or len(ems) != n or (centres is not None and len(centres) != n):
        raise AptError("with_lamps: radius / centres / emission must be one value or one per lamp")
    out = np.array(spheres, dtype=np.float32).ravel()
    for j, k in enumerate(idx):
        if not 0 <= k < int(num_spheres):
            raise AptError("with_lamps: index %d is not a sphere of a %d-sphere table" % (k, num_spheres))
        here = out[:10 * int(num_spheres)].reshape(10, int(num_spheres))[1:4, k]
        centre = tuple(float(c) for c in here) if centres is None else tuple(centres[j])
        out = with_lamp(out, num_spheres, k, radius=radii[j], centre=centre, emission=ems[j])
    return out


def lights_bytes(num_spheres, num_lights):
    """apt_lights_bytes: the size of a light table of num_lights lights for a scene of num_spheres spheres."""
    return int(lib().apt_lights_bytes(num_spheres, num_lights))


def build_lights(spheres, num_spheres, indices=None):
    """The light table of the lights= argument of render_frame / render_do_ex (apt_build_lights_host) -> uint32 numpy buffer to copy to
    the device (torch.from_numpy(t.view(np.int32)).cuda()).  indices: the spheres to list, in this order; None: every sphere with an
    emission channel > 0.  Selection probabilities: half by emitted power, half uniform, exact on the 24-bit grid of the draw."""
    spheres = np.ascontiguousarray(spheres, dtype=np.float32).ravel()
    if spheres.size < 10 * int(num_spheres):
        raise AptError("build_lights: the table holds fewer than 10 * num_spheres floats")
    if indices is None:
        ptr, n, bound = None, 0, int(num_spheres)
    else:
        ind = np.ascontiguousarray(indices, dtype=np.int64).ravel()
        if ind.size and (ind.min() < 0 or ind.max() > 0xFFFFFFFF):
            raise AptError("build_lights: a light index is out of range")
        ind = ind.astype(np.uint32)
        ptr, n, bound = ind.ctypes.data, int(ind.size), int(ind.size)
    buf = np.zeros(lights_bytes(num_spheres, bound) // 4, dtype=np.uint32)
    nbytes = ctypes.c_size_t(0)
    check(lib().apt_build_lights_host(_fptr(spheres), num_spheres, ptr, n, buf.ctypes.data, buf.nbytes, ctypes.byref(nbytes)),
          "apt_build_lights_host")
    return buf[:nbytes.value // 4].copy()


def gen_scene(num_spheres, seed=0, out_dir=None):
    """Build-defined large scene (BASELINE config 4): six walls, Ns-7 random small spheres,
    light at index Ns-1.  -> zero-padded [10][Ns] table."""
    n = ctypes.c_size_t(0)
    check(lib().apt_gen_scene_host(num_spheres, seed, None, ctypes.byref(n)), "apt_gen_scene_host")
    sph = np.zeros(n.value, dtype=np.float32)
    check(lib().apt_gen_scene_host(num_spheres, seed, _fptr(sph), None), "apt_gen_scene_host")
    if out_dir is not None:
        sph.tofile(os.path.join(out_dir, "spheres.bin"))
    return sph


def build_grid(spheres, num_spheres):
    """Host-built uniform grid for a large scene (apt_build_grid_host) -> uint32 numpy buffer to copy to the
    device; pass its device address as RenderParams.accel."""
    spheres = np.ascontiguousarray(spheres, dtype=np.float32).ravel()
    nbytes = ctypes.c_size_t(0)
    check(lib().apt_build_grid_host(_fptr(spheres), num_spheres, None, ctypes.byref(nbytes)), "apt_build_grid_host")
    buf = np.zeros(nbytes.value // 4, dtype=np.uint32)
    check(lib().apt_build_grid_host(_fptr(spheres), num_spheres, buf.ctypes.data, ctypes.byref(nbytes)), "apt_build_grid_host")
    return buf


def grid_flags(grid, num_spheres):
    """apt_grid_flags: the flags a built grid earns for a scene of `num_spheres` spheres (APT_FLAG_GRID_SLOTS: one launch per
    frame instead of two) -- `grid` is build_grid()'s numpy buffer or build_grid_device()'s tensor (its 128-byte head is copied
    to the host: a set-up step, not part of a launch path).  OR the result into RenderParams.flags next to accel."""
    # the header is 128 BYTES whatever the element type of the buffer the caller holds it in (apt_grid_flags reads that many)
    if hasattr(grid, "data_ptr"):
        flat = grid.reshape(-1)
        if flat.numel() * flat.element_size() < 128:
            raise AptError("grid_flags: the buffer is shorter than a grid header (128 bytes)")
        n = (128 + flat.element_size() - 1) // flat.element_size()
        head = flat[:n].cpu().contiguous().numpy().view(np.uint8)[:128]
    else:
        flat = np.ascontiguousarray(grid).reshape(-1)
        if flat.nbytes < 128:
            raise AptError("grid_flags: the buffer is shorter than a grid header (128 bytes)")
        head = flat.view(np.uint8)[:128]
    head = np.ascontiguousarray(head)
    return int(lib().apt_grid_flags(head.ctypes.data, num_spheres))


def build_grid_device(spheres_dev, num_spheres, stream=None):
    """The same grid built on the GPU from the device-resident table (apt_build_grid_device) -> torch int32 tensor on the
    device (pass its data_ptr() as RenderParams.accel).  Byte-identical to build_grid()."""
    import torch
    from . import render
    from ._lib import require_gpu
    require_gpu()
    st = render._stream_handle(stream)
    nbytes = ctypes.c_size_t(0)
    check(lib().apt_build_grid_device(spheres_dev.data_ptr(), num_spheres, st, None, 0, ctypes.byref(nbytes)), "apt_build_grid_device")
    buf = torch.empty(nbytes.value // 4, dtype=torch.int32, device=spheres_dev.device)
    check(lib().apt_build_grid_device(spheres_dev.data_ptr(), num_spheres, st, buf.data_ptr(), nbytes.value, ctypes.byref(nbytes)),
          "apt_build_grid_device")
    return buf


if __name__ == "__main__":              # gen_data.py:435-446
    os.makedirs("input", exist_ok=True)
    gen_rays(width, height, samples, seed=0, out_dir="./input")
    gen_spheres(out_dir="./input")
    print("===========Python Script Done=============")


def _new_camera():
    from ._lib import ApCamera
    c = ApCamera()
    c.struct_size = ctypes.sizeof(ApCamera)
    return c


def default_camera(w, h):
    """The reference's camera for a w x h image as a record (apt_camera_default_host): gen_rays' frame bit for bit, offset 140, no lens.
    Setting it renders what no camera renders, through the camera kernels."""
    c = _new_camera()
    check(lib().apt_camera_default_host(w, h, ctypes.byref(c)), "apt_camera_default_host")
    return c


def camera(eye, dir=None, target=None, up=(0, 1, 0), vfov_deg=None, scale=0.5135, offset=140.0, aperture=0.0, focus=None, width=None,
           height=None):
    """A look-along camera (apt_camera_build_host) for a width x height image: at `eye`, looking along `dir` or at `target` (dir = target
    - eye), `up` roughly up.  vfov_deg: the vertical field of view in degrees, 0 < vfov < 180 (scale = 2 * tan(vfov / 2)); else `scale`,
    the full image height at forward depth 1 (the reference's 0.5135), in [2^-20, 2^20].  offset: the segments start this far along the
    ray in units of forward depth (the reference's 140 steps through its front wall; 0 starts at the eye).  aperture: lens radius, 0 =
    pinhole; focus: forward depth of the plane in focus (None with a target: the distance to it)."""
    import math
    if width is None or height is None:
        raise AptError("camera: width and height are required")
    if (dir is None) == (target is None):
        raise AptError("camera: give exactly one of dir and target")
    eye = [float(x) for x in eye]
    if target is not None:
        dir = [float(t) - e for t, e in zip(target, eye)]
        if focus is None:
            focus = math.sqrt(sum(x * x for x in dir))
    if vfov_deg is not None:
        if not 0.0 < vfov_deg < 180.0:
            raise AptError("camera: vfov_deg must lie in (0, 180)")
        scale = 2.0 * math.tan(math.radians(vfov_deg) / 2.0)
    if focus is None:
        if aperture > 0:
            raise AptError("camera: a lens (aperture > 0) needs focus or target")
        focus = 0.0
    d3 = ctypes.c_double * 3
    c = _new_camera()
    check(lib().apt_camera_build_host(d3(*eye), d3(*[float(x) for x in dir]), d3(*[float(x) for x in up]), scale, offset, aperture, focus,
                                      width, height, ctypes.byref(c)), "apt_camera_build_host")
    return c


def environment(horizon=(0.0, 0.0, 0.0), zenith=None, sun_dir=(0.0, 1.0, 0.0), sun_radiance=(0.0, 0.0, 0.0), sun_angle_deg=0.0,
                sample_sun=True):
    """An environment record (apt_environment_build_host) for render.set_environment / Context.set_environment: a sky that blends from
    `horizon` (straight down) to `zenith` (straight up, +y; None: the horizon's value, a uniform sky) and a sun of radiance
    `sun_radiance` in the cone of half angle sun_angle_deg (0 = no sun, at most 90) around `sun_dir` (any length).  Radiances are one
    number or an (r, g, b) triple.  sample_sun: DIFF hits sample the sun directly (APT_ENV_SAMPLE_SUN: the same expectation, far less
    noise for a small sun).  sun_omc = 1 - cos(angle) is made here with numpy as 2 * sin(angle / 2)^2, which does not cancel for a
    small angle; the real sun's 0.2666 degrees give 1.08e-5."""
    from ._lib import APT_ENV_SAMPLE_SUN, ApEnvironment
    rgb = lambda v: [float(v)] * 3 if np.isscalar(v) else [float(x) for x in v]
    if not 0.0 <= float(sun_angle_deg) <= 90.0:
        raise AptError("environment: sun_angle_deg must lie in [0, 90]")
    half = np.sin(np.radians(np.float64(sun_angle_deg)) * 0.5)
    omc = float(2.0 * half * half)
    d3 = ctypes.c_double * 3
    e = ApEnvironment()
    e.struct_size = ctypes.sizeof(ApEnvironment)
    check(lib().apt_environment_build_host(d3(*rgb(horizon)), d3(*rgb(horizon if zenith is None else zenith)), d3(*[float(x) for x in sun_dir]),
                                           d3(*rgb(sun_radiance)), omc, APT_ENV_SAMPLE_SUN if sample_sun and omc > 0.0 else 0, ctypes.byref(e)),
          "apt_environment_build_host")
    return e


def _table_of(rows):
    """rows of (radius, x, y, z, emission rgb, albedo rgb) -> the zero-padded [10][Ns] table; r -> r^2 in float64, one rounding."""
    rows = np.array(rows, dtype=np.float64)
    rows[:, 0] = rows[:, 0] ** 2
    ns = rows.shape[0]
    out = np.zeros((ns * 10 + 127) // 128 * 128, dtype=np.float32)
    out[:10 * ns] = rows.T.astype(np.float32).ravel()
    return out


def film_curve(curve="srgb"):
    """The 256-entry table of render.Film.resolve / apt_film_resolve_* (apt_film_curve_host): table[0] = 0, table[k] the linear value
    at which the 8-bit code k begins, for curve "srgb" or "linear" (or APT_CURVE_*) -> float32 [256]."""
    from ._lib import APT_CURVE_LINEAR, APT_CURVE_SRGB
    code = {"linear": APT_CURVE_LINEAR, "srgb": APT_CURVE_SRGB}.get(curve, curve)
    if not isinstance(code, int):
        raise AptError(f"film_curve: unknown curve {curve!r}")
    table = np.zeros(256, dtype=np.float32)
    check(lib().apt_film_curve_host(code, _fptr(table)), "apt_film_curve_host")
    return table


def gen_spheres_open():
    """An open 8-sphere scene for an environment (render.set_environment): a ground sphere of radius 1e5 whose top is y = 0 and seven
    balls standing on it around (50, ., 60), in front of the reference camera -- three DIFF, a mirror, a glass ball, and two rough-metal
    balls (render with materials_flags(materials), APT_FLAG_GLOSS).  No walls and no emitter: without an environment every image of
    it is black -> (spheres float32 [128] = [10][8] planes zero padded, materials int32 [8]).  Pure Python."""
    from ._lib import MAT_DIFF, MAT_REFR, MAT_SPEC
    rows = [[1e5, 50.0, -1e5, 60.0, 0, 0, 0, 0.55, 0.5, 0.45],        # the ground
            [16.5, 27.0, 16.5, 47.0, 0, 0, 0, 0.999, 0.999, 0.999],   # mirror
            [16.5, 73.0, 16.5, 78.0, 0, 0, 0, 0.999, 0.999, 0.999],   # glass
            [12.0, 50.0, 12.0, 30.0, 0, 0, 0, 0.75, 0.25, 0.25],      # DIFF, red
            [8.0, 10.0, 8.0, 90.0, 0, 0, 0, 0.25, 0.75, 0.25],        # DIFF, green
            [8.0, 92.0, 8.0, 40.0, 0, 0, 0, 0.25, 0.25, 0.75],        # DIFF, blue
            [10.0, 52.0, 10.0, 100.0, 0, 0, 0, 0.9, 0.7, 0.3],        # rough metal, satin
            [6.0, 30.0, 6.0, 105.0, 0, 0, 0, 0.8, 0.8, 0.85]]         # rough metal, nearly a mirror
    mat = np.array([MAT_DIFF, MAT_SPEC, MAT_REFR, MAT_DIFF, MAT_DIFF, MAT_DIFF, gloss(0.35), gloss(0.05)], dtype=np.int32)
    return _table_of(rows), mat


def gen_scene_open(num_spheres, seed=0):
    """An open many-sphere scene for an environment: sphere 0 is gen_spheres_open's ground (radius 1e5, top at y = 0, DIFF) and spheres
    1 .. num_spheres - 1 are the small spheres of gen_scene_materials(num_spheres + 6, seed) -- its spheres 6 .. num_spheres + 4, radius
    0.5 .. 2 in the box [1, 99] x [0, 81.6] x [0, 170], with their material codes -- without its six walls and its light.  The walls
    of gen_scene are spheres that ENCLOSE the room, so taking away the ceiling alone opens nothing: every upward ray still ends on
    the inside of another wall; hence this scene instead of a variant of that one.  apt_build_grid_host accepts it (checked on the
    CPU, tests/test_environment_cpu.py: the ground goes to the always-tested list, the small spheres into cells), and
    num_spheres <= 64 runs through LDS tiles -> (spheres float32 zero-padded [10][Ns], materials int32 [Ns]).  No emitter: light it
    with an environment, or turn small spheres into lamps with with_lamps.  Pure Python on top of gen_scene_materials."""
    ns = int(num_spheres)
    if ns < 2:
        raise AptError("gen_scene_open: needs num_spheres >= 2 (the ground and a sphere)")
    from ._lib import MAT_DIFF
    src, smat = gen_scene_materials(ns + 6, seed)
    small = src[:10 * (ns + 6)].reshape(10, ns + 6)[:, 6:ns + 5]
    out = np.zeros((ns * 10 + 127) // 128 * 128, dtype=np.float32)
    planes = out[:10 * ns].reshape(10, ns)
    planes[:, 0] = _table_of([[1e5, 50.0, -1e5, 60.0, 0, 0, 0, 0.55, 0.5, 0.45]])[:10]
    planes[:, 1:] = small
    mat = np.empty(ns, dtype=np.int32)
    mat[0] = MAT_DIFF
    mat[1:] = smat[6:ns + 5]
    return out, mat
