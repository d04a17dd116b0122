"""What the *_device queries of a DeviceScene share: their inputs and outputs resolved to addresses, and the one call; and the
queries added since the class's surface was recorded (tests/python_api_surface.json holds DeviceScene to its members of then):
trace_radiance_device, camera_rays_device, trace_path_device, camera_sample_rays_device, occlusion_device and
occlusion_rays_device, functions of a DeviceScene, and occlusion_rays, which needs neither a scene nor a device."""
import ctypes as C
import math

from ._abi import OcclusionParams, P3DError, _check, _stream, lib
from ._device_args import (OCCLUSION_ACCUMULATE, PATH_ACCUMULATE, PATH_MAX_DEPTH, RADIANCE_MAX_DEPTH, RADIANCE_SKYBOX, _CAMERA_RAYS_OUTPUTS,
                           _CAMERA_SAMPLE_RAYS_OUTPUTS, _OCCLUSION_OUTPUTS, _OCCLUSION_RAYS_OUTPUTS, _PATH_OUTPUTS, _RADIANCE_OUTPUTS,
                           _device_blocks, _device_rows, _device_vector)


def _device_rays(scene, who, origin, direction, t_max):
    """(address of origin, of direction, of t_max or None, n) of the rays of a device query, or P3DError"""
    d_o, n = _device_rows(origin, who + ": origin", 3, ("float32",), scene.device)
    d_d, n_d = _device_rows(direction, who + ": direction", 3, ("float32",), scene.device)
    d_tm, n_tm = _device_vector(t_max, who + ": t_max", ("float32",), scene.device) if t_max is not None else (None, n)
    if n_d != n or n_tm != n:
        raise P3DError(-1, "%s: %d origins, %d directions%s" % (who, n, n_d, "" if t_max is None else ", %d limits" % n_tm))
    return d_o, d_d, d_tm, n


def _device_outputs(scene, who, names, n, out, like, table, rows_of):
    """name -> (tensor or None, address) for the outputs `names`: taken from the dict `out` (tensors or raw (address, rows)
    pairs, checked like the inputs), or allocated on the scene's device when `out` is None"""
    res = {}
    for name in names:
        dtype, cols = table[name]
        if out is None:
            import torch
            dev = like.device if hasattr(like, "device") else torch.device("cuda", scene.device)
            tail = () if cols is None else tuple(cols) if isinstance(cols, tuple) else (cols,)
            tensor = torch.empty((n,) + tail, dtype=getattr(torch, dtype), device=dev)
        else:
            if name not in out:
                raise P3DError(-1, "%s: out has no %r" % (who, name))
            tensor = out[name]
        what = "%s: out[%r]" % (who, name)
        if cols is None:
            ptr, rows = _device_vector(tensor, what, (dtype,), scene.device)
        elif isinstance(cols, tuple):
            ptr, rows = _device_blocks(tensor, what, cols, (dtype,), scene.device)
        else:
            ptr, rows = _device_rows(tensor, what, cols, (dtype,), scene.device)
        if rows != n:
            raise P3DError(-1, "%s: %d rows for %d %s" % (what, rows, n, rows_of))
        res[name] = (tensor, ptr)
    return res


def _device_points(scene, who, points, max_dist):
    """(address of points, of max_dist or None, n) of the points of a device query, or P3DError"""
    d_p, n = _device_rows(points, who + ": points", 3, ("float32",), scene.device)
    d_m, n_m = _device_vector(max_dist, who + ": max_dist", ("float32",), scene.device) if max_dist is not None else (None, n)
    if n_m != n:
        raise P3DError(-1, "%s: %d points, %d limits" % (who, n, n_m))
    return d_p, d_m, n


def _device_query(scene, who, accel, inputs, table, names, want, order, stream, out, like, rows_of="rays", k=None, known=None, refusal=None,
                  options=()):
    """What the *_device queries share.  In this order: a name in `want` that `known` (default: `table`) does not hold is
    refused; inputs() gives the input addresses and, last, n; `refusal`, the caller's own (about k), is raised if there is
    one; the outputs `names` are resolved against `table`; and L.p3d_<who> is called with (scene, accel, n, [k,] inputs,
    `options` (plain numbers), the outputs in the C order `order` - null where not in names -, stream) -> {name: tensor}.
    An input that is a ctypes value already (a count that stands between two buffers in the C order) is passed as it is"""
    unknown = [w for w in want if w not in (table if known is None else known)]
    if unknown:
        raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
    *addresses, n = inputs()
    if refusal:
        raise P3DError(-1, "%s: %s" % (who, refusal))
    res = _device_outputs(scene, who, names, n, out, like, table, rows_of)
    args = ([] if k is None else [k & 0xffffffff]) + [a if isinstance(a, C._SimpleCData) else C.c_void_p(a) for a in addresses] + list(options)
    args += [C.c_void_p(res[name][1]) if name in res else None for name in order]
    _check(getattr(scene._L, "p3d_" + who)(scene._h, int(accel), n, *args, _stream(stream)))
    return {name: v[0] for name, v in res.items()}


def trace_radiance_device(scene, accel, origin, direction, max_depth, flags=0, want=("rgb", "hit_id"), stream=0, out=None):
    """p3d_trace_radiance_device: what n rays held in device memory see in the DeviceScene `scene` - the Whitted colour rayTracing
    returns for each as a primary ray, max_depth (0 .. RADIANCE_MAX_DEPTH) levels deep, enqueued on `stream` without a wait ->
    {name: tensor} for the names in `want` ("rgb" (n, 3), always there, and "hit_id" (n,): the object of the first closest hit
    or -1).  A ray that equals the primary ray of a pixel (camera_rays_device) gives that pixel of a STACK_PER_PIXEL frame
    without anti-aliasing, bit for bit.  flags: 0 or RADIANCE_SKYBOX (a miss returns the cubemap's texel; needs set_skybox).
    Every accel; rays, `out`, `stream` and the refusals as DeviceScene.trace_closest_device."""
    who = "trace_radiance_device"
    max_depth, flags = int(max_depth), int(flags)
    names = ["rgb"] + [w for w in ("hit_id",) if w in want]
    refusal = None
    if not 0 <= max_depth <= RADIANCE_MAX_DEPTH:
        refusal = "max_depth must be 0 .. %d, got %d" % (RADIANCE_MAX_DEPTH, max_depth)
    elif flags & ~RADIANCE_SKYBOX:
        refusal = "unknown flag in %#x (RADIANCE_SKYBOX is %d)" % (flags, RADIANCE_SKYBOX)

    def rays():
        d_o, d_d, _, n = _device_rays(scene, who, origin, direction, None)
        return d_o, d_d, n

    return _device_query(scene, who, accel, rays, _RADIANCE_OUTPUTS, names, want, ("rgb", "hit_id"), stream, out, origin, refusal=refusal,
                         options=(max_depth, flags))


def camera_rays_device(scene, camera=None, tile=None, stream=0, out=None):
    """p3d_camera_rays_device: the primary rays of the pixel centres of `tile` (None = the whole frame) through `camera` (a
    Camera of the scene's resolution, e.g. from look_at; None = the scene's), enqueued on `stream` without a wait ->
    {"origin", "direction"}: float32 (w * h, 3) tensors in the row order of scene.render(cfg, tile) - the floats a frame without
    anti-aliasing traces, and what trace_radiance_device takes.  `out`: a dict of tensors (or raw (address, rows) pairs)
    to write into; otherwise they are allocated on torch's current stream.  A lens camera (aperture != 0) is refused."""
    who = "camera_rays_device"
    t = tile or scene.full_tile()
    n = t.w * t.h
    if n <= 0:
        raise P3DError(-1, "%s: an empty tile" % who)
    res = _device_outputs(scene, who, ("origin", "direction"), n, out, None, _CAMERA_RAYS_OUTPUTS, "pixels")
    _check(scene._L.p3d_camera_rays_device(scene._h, C.byref(camera) if camera is not None else None, C.byref(t),
                                           C.c_void_p(res["origin"][1]), C.c_void_p(res["direction"][1]), _stream(stream)))
    return {name: v[0] for name, v in res.items()}


def trace_path_device(scene, accel, origin, direction, max_depth, samples=1, sample_begin=0, seed=0, rng=None, flags=0, want=("hit_id",),
                      out=None, stream=0):
    """p3d_trace_path_device: the path-traced radiance n rays held in device memory see in the DeviceScene `scene` - the SUM of
    Radiance over the samples sample_begin .. sample_begin + samples - 1 of each ray as a primary ray, max_depth bounces deep,
    enqueued on `stream` without a wait -> {"rgb": (n, 3), and, if in `want`, "hit_id": (n,)}.  Nothing is divided.
    rng None: sample s of ray i draws from the stream a frame seeds for (pixel i, sample s) with `seed`.  rng given: an int64
    (n, 2) tensor (or a raw pair) of {state, inc} bit patterns, e.g. camera_sample_rays_device's; ray i draws all its samples
    from that one stream, which is written back.  flags: RADIANCE_SKYBOX, PATH_ACCUMULATE (the sum starts from what
    out["rgb"] holds and is added to in place; needs out={"rgb": ...}).  Every accel; rays, `out`, `stream` and the refusals
    as trace_radiance_device."""
    who = "trace_path_device"
    max_depth, flags, samples, sample_begin = int(max_depth), int(flags), int(samples), int(sample_begin)
    names = ["rgb"] + [w for w in ("hit_id",) if w in want]
    refusal = None
    if not 0 <= max_depth <= PATH_MAX_DEPTH:
        refusal = "max_depth must be 0 .. %d, got %d" % (PATH_MAX_DEPTH, max_depth)
    elif samples < 1:
        refusal = "samples must be at least 1, got %d" % samples
    elif sample_begin < 0 or sample_begin + samples > 1 << 32:
        refusal = "sample_begin + samples must stay within 0 .. 2^32, got %d + %d" % (sample_begin, samples)
    elif flags & ~(RADIANCE_SKYBOX | PATH_ACCUMULATE):
        refusal = "unknown flag in %#x (RADIANCE_SKYBOX is %d, PATH_ACCUMULATE is %d)" % (flags, RADIANCE_SKYBOX, PATH_ACCUMULATE)
    elif (flags & PATH_ACCUMULATE) and (out is None or "rgb" not in out):
        refusal = "PATH_ACCUMULATE adds to out['rgb'], which is not given"

    unknown = [w for w in want if w not in _PATH_OUTPUTS]
    if unknown:
        raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
    d_o, d_d, _, n = _device_rays(scene, who, origin, direction, None)
    d_r = None
    if rng is not None:
        d_r, n_r = _device_rows(rng, who + ": rng", 2, ("int64",), scene.device)
        if n_r != n:
            raise P3DError(-1, "%s: %d rays, %d rng states" % (who, n, n_r))
    if refusal:
        raise P3DError(-1, "%s: %s" % (who, refusal))
    res = _device_outputs(scene, who, names, n, out, origin, _PATH_OUTPUTS, "rays")
    _check(scene._L.p3d_trace_path_device(scene._h, int(accel), n, C.c_void_p(d_o), C.c_void_p(d_d), max_depth, sample_begin, samples,
                                          int(seed) & 0xffffffffffffffff, C.c_void_p(d_r), flags, C.c_void_p(res["rgb"][1]),
                                          C.c_void_p(res["hit_id"][1]) if "hit_id" in res else None, _stream(stream)))
    return {name: v[0] for name, v in res.items()}


def camera_sample_rays_device(scene, cfg, sample, camera=None, tile=None, want=("rng",), out=None, stream=0):
    """p3d_camera_sample_rays_device: sample `sample` (0 .. spp_sqrt^2 - 1) of every pixel of `tile` (None = the whole frame)
    through `camera` (None = the scene's) as a frame of the Config `cfg` casts it - jittered or tent-filtered, through the
    lens with depth_of_field - enqueued on `stream` without a wait -> {"origin", "direction": float32 (w * h, 3), and, if in
    `want`, "rng": int64 (w * h, 2), the uint64 bit patterns {state, inc} of the pixel's stream after the sample's draws}, in
    the row order of scene.render(cfg, tile): what trace_path_device takes.  `out` as camera_rays_device."""
    who = "camera_sample_rays_device"
    unknown = [w for w in want if w not in ("rng",)]
    if unknown:
        raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
    t = tile or scene.full_tile()
    n = t.w * t.h
    if n <= 0:
        raise P3DError(-1, "%s: an empty tile" % who)
    names = ("origin", "direction") + (("rng",) if "rng" in want else ())
    res = _device_outputs(scene, who, names, n, out, None, _CAMERA_SAMPLE_RAYS_OUTPUTS, "pixels")
    _check(scene._L.p3d_camera_sample_rays_device(scene._h, C.byref(camera) if camera is not None else None, C.byref(t), C.byref(cfg),
                                                  int(sample) & 0xffffffff, C.c_void_p(res["origin"][1]), C.c_void_p(res["direction"][1]),
                                                  C.c_void_p(res["rng"][1]) if "rng" in res else None, _stream(stream)))
    return {name: v[0] for name, v in res.items()}


def _occlusion_params(who, samples, sample_begin, seed, point_offset, bias, flags=0, team=0):
    """The OcclusionParams of a call, or P3DError for what the library would refuse of them"""
    samples, sample_begin, point_offset, flags, team, bias = int(samples), int(sample_begin), int(point_offset), int(flags), int(team), float(bias)
    if samples < 1:
        raise P3DError(-1, "%s: samples must be at least 1, got %d" % (who, samples))
    if sample_begin < 0 or sample_begin + samples > 1 << 32:
        raise P3DError(-1, "%s: sample_begin + samples must stay within 0 .. 2^32, got %d + %d" % (who, sample_begin, samples))
    if not 0 <= point_offset < 1 << 32:
        raise P3DError(-1, "%s: point_offset must be 0 .. 2^32 - 1, got %d" % (who, point_offset))
    if flags & ~OCCLUSION_ACCUMULATE:
        raise P3DError(-1, "%s: unknown flag in %#x (OCCLUSION_ACCUMULATE is %d)" % (who, flags, OCCLUSION_ACCUMULATE))
    if not math.isfinite(bias):
        raise P3DError(-1, "%s: bias must be finite, got %r" % (who, bias))
    if team < 0 or team > 64 or team & (team - 1):
        raise P3DError(-1, "%s: team must be 0 (the library chooses) or a power of two <= 64, got %d" % (who, team))
    return OcclusionParams(int(seed) & 0xffffffffffffffff, samples, sample_begin, point_offset, flags, bias, team)


def _occlusion_points(scene, who, points, normals, max_dist):
    """(address of points, of normals, of max_dist or None, n) of an occlusion query, or P3DError"""
    d_p, d_m, n = _device_points(scene, who, points, max_dist)
    d_n, n_n = _device_rows(normals, who + ": normals", 3, ("float32",), scene.device)
    if n_n != n:
        raise P3DError(-1, "%s: %d points, %d normals" % (who, n, n_n))
    return d_p, d_n, d_m, n


def occlusion_device(scene, accel, points, normals, samples, max_dist=None, sample_begin=0, seed=0, point_offset=0, bias=1e-4, flags=0,
                     team=0, want=("unoccluded",), stream=0, out=None):
    """p3d_occlusion_device: how open the n surface points held in device memory are in the DeviceScene `scene` - for each, the
    number of the `samples` cosine-weighted rays over the hemisphere around its normal (float32 (n, 3), used as given: bring unit
    normals) that meet nothing within max_dist (float32 (n,); None: no limit), enqueued on `stream` without a wait ->
    {"unoccluded": int32 (n,), and, if in `want`, "bent": float32 (n, 3), the unnormalised sum of the free directions}.
    unoccluded / samples is the ambient-occlusion term.  Sample s of point i draws from the stream of (point_offset + i, s) with
    `seed`: a later call with the next sample_begin and flags=OCCLUSION_ACCUMULATE (needs `out`) continues the estimate, a split
    batch with point_offset gives the rows of the whole.  team: lanes per point, 0 (the library chooses) or a power of two <= 64;
    the counts do not depend on it.  ACCEL_NONE and ACCEL_BVH; points, `out`, `stream` and the refusals as
    DeviceScene.nearest_device.  The rays themselves: occlusion_rays_device, occlusion_rays."""
    who = "occlusion_device"
    names = ["unoccluded"] + [w for w in ("bent",) if w in want]
    unknown = [w for w in want if w not in _OCCLUSION_OUTPUTS]
    if unknown:
        raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
    params = _occlusion_params(who, samples, sample_begin, seed, point_offset, bias, flags, team)
    if (params.flags & OCCLUSION_ACCUMULATE) and (out is None or any(name not in out for name in names)):
        raise P3DError(-1, "%s: OCCLUSION_ACCUMULATE adds to the tensors of `out`, which are not given" % who)
    return _device_query(scene, who, accel, lambda: _occlusion_points(scene, who, points, normals, max_dist), _OCCLUSION_OUTPUTS, names, want,
                         ("unoccluded", "bent"), stream, out, points, rows_of="points", options=(C.byref(params),))


def occlusion_rays_device(scene, points, normals, samples, sample_begin=0, seed=0, point_offset=0, bias=1e-4, stream=0, out=None):
    """p3d_occlusion_rays_device: the rays occlusion_device casts, written out -> {"origin", "direction"}: float32 (n * samples, 3),
    row i * samples + j = sample sample_begin + j of point i; what DeviceScene.trace_any_device takes.  `out`, `stream` as there."""
    who = "occlusion_rays_device"
    params = _occlusion_params(who, samples, sample_begin, seed, point_offset, bias)
    d_p, d_n, _, n = _occlusion_points(scene, who, points, normals, None)
    res = _device_outputs(scene, who, ("origin", "direction"), n * params.samples, out, points, _OCCLUSION_RAYS_OUTPUTS, "rays")
    _check(scene._L.p3d_occlusion_rays_device(scene._h, n, C.c_void_p(d_p), C.c_void_p(d_n), C.byref(params), C.c_void_p(res["origin"][1]),
                                              C.c_void_p(res["direction"][1]), _stream(stream)))
    return {name: v[0] for name, v in res.items()}


def occlusion_rays(points, normals, samples, sample_begin=0, seed=0, point_offset=0, bias=1e-4):
    """p3d_occlusion_rays: the same rays from host arrays, bit for bit, with no scene and no device: (n, 3) points and normals ->
    (origin, direction), float32 (n * samples, 3) numpy arrays"""
    import numpy as np
    who = "occlusion_rays"
    params = _occlusion_params(who, samples, sample_begin, seed, point_offset, bias)
    p, w = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(normals, np.float32)
    if p.ndim != 2 or p.shape[1] != 3 or w.shape != p.shape:
        raise P3DError(-1, "%s: points %r and normals %r, needed: (n, 3) both" % (who, p.shape, w.shape))
    origin, direction = np.empty((len(p) * params.samples, 3), np.float32), np.empty((len(p) * params.samples, 3), np.float32)
    _check(lib().p3d_occlusion_rays(len(p), p.ctypes.data, w.ctypes.data, C.byref(params), origin.ctypes.data, direction.ctypes.data))
    return origin, direction
