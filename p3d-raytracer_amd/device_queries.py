"""What the *_device queries of a DeviceScene share: their inputs and outputs resolved to addresses, and the one call; and the
queries added since the class's surface was recorded (tests/python_api_surface.json holds DeviceScene to its members of then):
trace_radiance_device and camera_rays_device, functions of a DeviceScene."""
import ctypes as C

from ._abi import P3DError, _check, _stream
from ._device_args import (RADIANCE_MAX_DEPTH, RADIANCE_SKYBOX, _CAMERA_RAYS_OUTPUTS, _RADIANCE_OUTPUTS, _device_blocks, _device_rows,
                           _device_vector)


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
    `options` (plain numbers), the outputs in the C order `order` - null where not in names -, stream) -> {name: tensor}"""
    unknown = [w for w in want if w not in (table if known is None else known)]
    if unknown:
        raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
    *addresses, n = inputs()
    if refusal:
        raise P3DError(-1, "%s: %s" % (who, refusal))
    res = _device_outputs(scene, who, names, n, out, like, table, rows_of)
    args = ([] if k is None else [k & 0xffffffff]) + [C.c_void_p(a) for a in addresses] + list(options)
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
