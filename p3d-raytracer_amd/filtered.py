"""Queries that leave objects out, per query (include/p3d_filter.h): nearest_k_filtered_device, sweep_sphere_filtered_device and
the segment family of the ray queries, trace_any_filtered_device, trace_hits_filtered_device and occlusion_filtered_device,
functions of a DeviceScene over device tensors, and host_nearest_k_filtered and host_sweep_sphere_filtered, the brute force on
the CPU over a HostScene.  For a cloth vertex, a particle or a body that is itself part of the scene.  Functions and not
members: tests/python_api_surface.json holds both classes to the members they had.

A filter is a skip list, `skip`: int32 (n, s) with s <= FILTER_SKIP_MAX object indices per query (an entry < 0 or >= the
object count names nothing: pad with -1), and a skip range, `skip_range`: int32 (n, 2) rows (first, count).  Either may be
None.  The answers are those of the unfiltered query over the scene without the named objects; with both None they are the
unfiltered query's, bit for bit."""
import ctypes as C

from ._abi import P3DError
from ._device_args import (NEAREST_K_MAX, OCCLUSION_ACCUMULATE, TRACE_HITS_K_MAX, _OCCLUSION_OUTPUTS, _device_rows, _nearest_k_outputs,
                           _trace_hits_outputs)
from .device_queries import _device_points, _device_query, _device_rays, _occlusion_params, _occlusion_points
from ._host_args import _host_nearest_k
from .sweep import _host_sweep, _sweep

FILTER_SKIP_MAX = 8  # P3D_FILTER_SKIP_MAX


def _device_filter(scene, who, skip, n_skip, skip_range, n, rows_of):
    """(address of skip or None, n_skip as the C argument, address of skip_range or None) of a device query of n rows.  A
    tensor brings its own width; a raw (address, rows) pair needs `n_skip`"""
    d_s, width = None, 0
    if skip is not None:
        if hasattr(skip, "shape") and hasattr(skip, "dim"):
            if skip.dim() != 2:
                raise P3DError(-1, "%s: skip: shape %r, needed: (n, s) with s <= %d" % (who, tuple(skip.shape), FILTER_SKIP_MAX))
            width = int(skip.shape[1])
            if n_skip is not None and int(n_skip) != width:
                raise P3DError(-1, "%s: skip has %d columns, n_skip says %d" % (who, width, int(n_skip)))
        elif n_skip is None:
            raise P3DError(-1, "%s: skip as a raw (address, rows) pair needs n_skip" % who)
        else:
            width = int(n_skip)
        if width < 0:
            raise P3DError(-1, "%s: n_skip must be 0 .. %d, got %d" % (who, FILTER_SKIP_MAX, width))
        if width > 0:  # (no columns: no list)
            d_s, rows = _device_rows(skip, who + ": skip", width, ("int32",), scene.device)
            if rows != n:
                raise P3DError(-1, "%s: %d %s, %d skip rows" % (who, n, rows_of, rows))
    d_r = None
    if skip_range is not None:
        d_r, rows = _device_rows(skip_range, who + ": skip_range", 2, ("int32",), scene.device)
        if rows != n:
            raise P3DError(-1, "%s: %d %s, %d skip ranges" % (who, n, rows_of, rows))
    return d_s, C.c_uint32(width & 0xffffffff), d_r


def nearest_k_filtered_device(scene, accel, points, k, max_dist=None, skip=None, skip_range=None, want=("count", "object", "dist"), stream=0,
                              out=None, n_skip=None):
    """p3d_nearest_k_filtered_device: DeviceScene.nearest_k_device for the scene without the objects each point names (the
    module's docstring has the filter; k = 1 is nearest_device's answer).  skip: a contiguous int32 (n, s) CUDA/HIP tensor on the
    scene's device, or a raw (address, rows) pair with n_skip = s; skip_range: int32 (n, 2) likewise.  Outputs, `want`, `out`,
    `stream` and the refusals as nearest_k_device; the answers are host_nearest_k_filtered's, bit for bit."""
    who = "nearest_k_filtered_device"
    k = int(k)
    names = ["count", "object"] + [w for w in ("dist", "closest", "normal") if w in want]
    refusal = None
    if out is None and not 1 <= k <= NEAREST_K_MAX:  # (with the caller's outputs the library says it)
        refusal = "k must be 1 .. %d, got %d" % (NEAREST_K_MAX, k)

    def inputs():
        d_p, d_m, n = _device_points(scene, who, points, max_dist)
        return (d_p, d_m) + _device_filter(scene, who, skip, n_skip, skip_range, n, "points") + (n,)

    return _device_query(scene, who, accel, inputs, _nearest_k_outputs(max(k, 0)), names, want, ("count", "object", "dist", "closest", "normal"),
                         stream, out, points, "points", k=k, refusal=refusal)


def sweep_sphere_filtered_device(scene, accel, origin, direction, radius, t_max=None, skip=None, skip_range=None, want=("t",), out=None, stream=0,
                                 n_skip=None):
    """p3d_sweep_sphere_filtered_device: sweep.sweep_sphere_device for the scene without the objects each ball names (a particle
    that is a sphere of the scene skips itself).  skip, skip_range, n_skip as nearest_k_filtered_device; everything else, the
    refusals included, as sweep_sphere_device; the answers are host_sweep_sphere_filtered's, bit for bit."""
    who = "sweep_sphere_filtered_device"
    return _sweep(scene, who, accel, origin, direction, radius, t_max, want, out, stream,
                  more=lambda n: _device_filter(scene, who, skip, n_skip, skip_range, n, "balls"))


def trace_any_filtered_device(scene, accel, origin, direction, t_max=None, skip=None, skip_range=None, stream=0, out=None, n_skip=None):
    """p3d_trace_any_filtered_device: the segment query of DeviceScene.trace_any_device for the scene without the objects each
    ray names -> {"occluded": uint8 (n,)}: 1 iff some object the ray does not skip is hit at t < t_max.  t_max: float32 (n,);
    None: a +inf tensor is filled here (the library itself requires the limit: the feeler without one takes no filter).  skip,
    skip_range, n_skip as nearest_k_filtered_device.  ACCEL_NONE and ACCEL_BVH; everything else as trace_any_device."""
    who = "trace_any_filtered_device"

    def inputs():
        limits = t_max
        if limits is None and hasattr(origin, "new_full") and origin.dim() == 2:
            import torch
            limits = origin.new_full((origin.shape[0],), float("inf"))  # (written on torch's current stream, like a new output)
            handle = getattr(stream, "cuda_stream", stream)
            if handle:  # (the allocator must not hand the block on before `stream` has passed the call)
                limits.record_stream(stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(handle)))
        d_o, d_d, d_tm, n = _device_rays(scene, who, origin, direction, limits)
        inputs.keep = limits  # (alive until the call is enqueued)
        return (d_o, d_d, d_tm) + _device_filter(scene, who, skip, n_skip, skip_range, n, "rays") + (n,)

    return _device_query(scene, who, accel, inputs, {"occluded": ("uint8", None)}, ["occluded"], (), ("occluded",), stream, out, origin)


def trace_hits_filtered_device(scene, accel, origin, direction, k, t_max=None, skip=None, skip_range=None, want=("count", "object", "t"),
                               stream=0, out=None, n_skip=None):
    """p3d_trace_hits_filtered_device: DeviceScene.trace_hits_device for the scene without the objects each ray names: a skipped
    object is not listed, not counted in "total" and tightens no bound.  k = 0 with want=("total",) is the parity without the
    asking body; k = 1 is the filtered closest hit of the segment family.  skip, skip_range, n_skip as
    nearest_k_filtered_device; outputs, `want`, `out`, `stream` and the refusals as trace_hits_device."""
    who = "trace_hits_filtered_device"
    k = int(k)
    names = (["count", "object"] + [w for w in ("t", "hit_point", "normal") if w in want] if k != 0 else []) + [w for w in ("total",) if w in want]
    refusal = None
    if k < 0 or (out is None and k > TRACE_HITS_K_MAX):  # (too large a k with the caller's outputs: the library says it)
        refusal = "k must be 0 .. %d, got %d" % (TRACE_HITS_K_MAX, k)
    elif not names:
        refusal = "k = 0 is the count alone: want must hold 'total'"

    def inputs():
        d_o, d_d, d_tm, n = _device_rays(scene, who, origin, direction, t_max)
        return (d_o, d_d, d_tm) + _device_filter(scene, who, skip, n_skip, skip_range, n, "rays") + (n,)

    return _device_query(scene, who, accel, inputs, _trace_hits_outputs(max(k, 0)), names, want, ("count", "total", "object", "t", "hit_point", "normal"),
                         stream, out, origin, k=k, known=_trace_hits_outputs(1), refusal=refusal)


def occlusion_filtered_device(scene, accel, points, normals, samples, max_dist=None, skip=None, skip_range=None, sample_begin=0, seed=0,
                              point_offset=0, bias=1e-4, flags=0, team=0, want=("unoccluded",), stream=0, out=None, n_skip=None):
    """p3d_occlusion_filtered_device: device_queries.occlusion_device for the scene without the objects each POINT names: one
    filter row per point, shared by all its samples (a particle that is a sphere of the scene skips itself and is open where
    nothing else is near).  The rays are occlusion_rays_device's, unchanged.  skip, skip_range, n_skip as
    nearest_k_filtered_device; everything else, the refusals included, as occlusion_device."""
    who = "occlusion_filtered_device"
    names = ["unoccluded"] + [w for w in ("bent",) if w in want]
    unknown = [w for w in want if w not in _OCCLUSION_OUTPUTS]
    if unknown:
        raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
    params = _occlusion_params(who, samples, sample_begin, seed, point_offset, bias, flags, team)
    if (params.flags & OCCLUSION_ACCUMULATE) and (out is None or any(name not in out for name in names)):
        raise P3DError(-1, "%s: OCCLUSION_ACCUMULATE adds to the tensors of `out`, which are not given" % who)
    # (the C order has params between the points and the filter: both are resolved here and handed on as they stand)
    d_p, d_n, d_m, n = _occlusion_points(scene, who, points, normals, max_dist)
    d_s, width, d_r = _device_filter(scene, who, skip, n_skip, skip_range, n, "points")
    return _device_query(scene, who, accel, lambda: (d_p, d_n, d_m, n), _OCCLUSION_OUTPUTS, names, want, ("unoccluded", "bent"), stream, out,
                         points, rows_of="points", options=(C.byref(params), C.c_void_p(d_s), width, C.c_void_p(d_r)))


def host_nearest_k_filtered(host_scene, points, k, max_dist=None, skip=None, skip_range=None):
    """p3d_host_scene_nearest_k_filtered: HostScene.nearest_k for the scene without the objects each point names, by brute force
    on the CPU -> (count int32 (n,), object int32 (n, k), dist float32 (n, k), closest float32 (n, k, 3)).  skip: int32 (n, s),
    s <= FILTER_SKIP_MAX; skip_range: int32 (n, 2); either may be None."""
    return _host_nearest_k(host_scene, "host_nearest_k_filtered", points, k, max_dist, filters=(skip, skip_range))


def host_sweep_sphere_filtered(host_scene, origin, direction, radius, t_max=None, skip=None, skip_range=None):
    """p3d_host_scene_sweep_sphere_filtered: sweep.host_sweep_sphere for the scene without the objects each ball names ->
    (object int32 (n,), t float32 (n,), centre float32 (n, 3), contact float32 (n, 3))."""
    return _host_sweep(host_scene, "host_sweep_sphere_filtered", origin, direction, radius, t_max, filters=(skip, skip_range))
