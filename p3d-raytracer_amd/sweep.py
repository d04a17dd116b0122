"""Sphere sweeps (include/p3d_sweep.h): the first contact of moving balls with a scene.  sweep_sphere_device, a function of a
DeviceScene over device tensors, and host_sweep_sphere, the brute force on the CPU over a HostScene.  Functions and not
members: tests/python_api_surface.json holds both classes to the members they had."""
import ctypes as C
import weakref

import numpy as np

from ._abi import ACCEL_BVH, ACCEL_GRID, P3DError, Prim
from ._device_args import _SWEEP_OUTPUTS, _device_vector
from ._host_args import _host_filter, _host_query, _per_row, _row_pair
from .device_queries import _device_query, _device_rays

UNSUPPORTED = -3  # P3D_ERR_UNSUPPORTED
PRIM_BOX, PRIM_PLANE = 2, 3  # P3D_PRIM_BOX, P3D_PRIM_PLANE


_KINDS = weakref.WeakKeyDictionary()  # HostScene -> (holds a box, holds a plane)


def _kinds(host_scene):
    """(holds a box, holds a plane) of a HostScene, read once per scene: no update changes an object's kind"""
    known = _KINDS.get(host_scene)
    if known is None:
        d = host_scene.desc(False, False)
        words, at = C.sizeof(Prim) // 4, Prim.type.offset // 4  # p3d_prim as uint32 words, and which of them is `type`
        types = np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(C.c_uint32)), shape=(d.n_prims, words))[:, at] if d.n_prims else np.zeros(0, np.uint32)
        known = _KINDS[host_scene] = (bool((types == PRIM_BOX).any()), bool((types == PRIM_PLANE).any()))
    return known


def _refuse_by_host_scene(scene, who, accel, grid, box):
    """What a per-object device query refuses before the library is called: the grid (`grid`: the query's sentence) and,
    where the DeviceScene came from a HostScene, a scene that holds a box (`box`: the query's sentence; None: boxes are
    taken) and a plane under ACCEL_BVH"""
    refusal = None
    if int(accel) == ACCEL_GRID:
        refusal = grid
    elif getattr(scene, "host", None) is not None:
        holds_box, holds_plane = _kinds(scene.host)
        if box and holds_box:
            refusal = box
        elif holds_plane and int(accel) == ACCEL_BVH:
            refusal = "the scene holds a plane, which the tree cannot find (use ACCEL_NONE)"
    if refusal:
        raise P3DError(UNSUPPORTED, "%s: %s" % (who, refusal))


def _torch_stream(stream, device):
    """`stream` as _abi._stream takes it (a torch.cuda.Stream, a raw hipStream_t, 0 or None) as a torch stream"""
    import torch
    if hasattr(stream, "cuda_stream"):
        return stream
    return torch.cuda.ExternalStream(int(stream), device=device) if stream else torch.cuda.default_stream(device)


def sweep_sphere_device(scene, accel, origin, direction, radius, t_max=None, want=("t",), out=None, stream=0):
    """p3d_sweep_sphere_device: the first contact of n moving balls held in device memory with the DeviceScene `scene`,
    enqueued on `stream` without a wait.  Ball i has its centre on origin[i] + t * direction[i] (float32 (n, 3) each; the
    direction is used as given, t is in its units) and the radius radius[i] (float32 (n,), or one number for all), and is
    followed up to t_max[i] (float32 (n,); None: no limit) -> {name: tensor}: "object" int32 (n,), always there (-1: nothing
    met), and of "t" (n,), "centre", "contact" and "normal" (n, 3) those named in `want`: the contact time (FLT_MAX where
    nothing is met), the centre then, the point of the object the ball touches and the object's normal there (zeros).
    ACCEL_NONE and ACCEL_BVH; ACCEL_GRID, a scene that holds a box, and ACCEL_BVH over a scene that holds a plane are refused
    with P3D_ERR_UNSUPPORTED - by this function already where the scene came from a HostScene.  Rays, `out`, `stream` and the
    other refusals as DeviceScene.trace_closest_device."""
    return _sweep(scene, "sweep_sphere_device", accel, origin, direction, radius, t_max, want, out, stream)


def _sweep(scene, who, accel, origin, direction, radius, t_max, want, out, stream, more=None):
    """sweep_sphere_device, and what filtered.sweep_sphere_filtered_device shares with it: more(n) -> the inputs that follow
    t_max in the C order of p3d_<who>"""
    names = ["object"] + [w for w in ("t", "centre", "contact", "normal") if w in want]
    _refuse_by_host_scene(scene, who, accel, "no sphere sweep through the grid (use ACCEL_BVH or ACCEL_NONE)",
                          "the scene holds a box: a ball against a box (a rounded box, and its inside) is not swept")

    filled = []  # one number for all radii: the tensor made of it, held HERE until the library call has returned

    def balls():
        d_o, d_d, d_tm, n = _device_rays(scene, who, origin, direction, t_max)
        r = radius
        if not (hasattr(r, "data_ptr") or isinstance(r, tuple)):  # a tensor filled on `stream`, in front of the kernel
            import torch
            dev = origin.device if hasattr(origin, "device") else torch.device("cuda", scene.device)
            with torch.cuda.stream(_torch_stream(stream, dev)):
                r = torch.full((n,), float(r), dtype=torch.float32, device=dev)
            filled.append(r)
        d_r, n_r = _device_vector(r, who + ": radius", ("float32",), scene.device)
        if n_r != n:
            raise P3DError(-1, "%s: %d origins, %d radii" % (who, n, n_r))
        return (d_o, d_d, d_r, d_tm) + (tuple(more(n)) if more else ()) + (n,)

    # `filled` outlives the call: _device_query resolves the inputs first, allocates the outputs next and enqueues the kernel
    # last, so a tensor owned by balls() would be back with torch's allocator - and handed out again as an output of the same
    # size - before the kernel that reads it is launched.  It was allocated on `stream`; freed after the launch, the allocator
    # reuses it behind the kernel in that stream's order
    res = _device_query(scene, who, accel, balls, _SWEEP_OUTPUTS, names, want, ("object", "t", "centre", "contact", "normal"), stream, out, origin,
                        rows_of="balls")
    del filled[:]
    return res


def host_sweep_sphere(host_scene, origin, direction, radius, t_max=None):
    """p3d_host_scene_sweep_sphere: the same on the CPU, by brute force over every object of the HostScene `host_scene`:
    (n, 3) origins and directions, a radius per ball or one number, t_max (n,) or None -> (object int32 (n,), t float32 (n,),
    centre float32 (n, 3), contact float32 (n, 3)); -1, FLT_MAX and zeros where nothing is met.  A scene that holds a box is
    refused (P3D_ERR_UNSUPPORTED)."""
    return _host_sweep(host_scene, "host_sweep_sphere", origin, direction, radius, t_max)


def _host_sweep(host_scene, who, origin, direction, radius, t_max, filters=None):
    """host_sweep_sphere and, with filters = (skip, skip_range), filtered.host_sweep_sphere_filtered"""
    o, d = _row_pair(who, "origins", origin, "directions", direction)
    n = len(o)
    args, form = (o, d, _per_row(who, radius, n, "origins", "radii", one_for_all=True), _per_row(who, t_max, n, "origins", "limits")), "sweep_sphere"
    if filters is not None:
        args, form = args + _host_filter(who, filters[0], filters[1], n, "balls"), "sweep_sphere_filtered"
    return _host_query(host_scene, form, n, args, _SWEEP_OUTPUTS, ("object", "t", "centre", "contact"))
