"""Nearest surfaces to a segment (include/p3d_segment.h): capsule overlap and edge proximity.  nearest_segment_k_device, a function
of a DeviceScene over device tensors, and host_nearest_segment_k, the brute force on the CPU over a HostScene; segment_box_d2,
the bound the tree is culled with, for the tests.  Functions and not members: tests/python_api_surface.json holds both classes to
the members they had.

Segment i runs from a[i] to b[i].  The answers are the (at most) k objects whose surface comes nearest to any point of the
segment, in the order (d2, object index), each with its distance, the parameter s of the segment's nearest point
x = a + (b - a) s, that point, and the object's nearest point; a segment that crosses a surface has distance exactly 0 to it.
Filters (`skip`, `skip_range`) are filtered.py's."""
import numpy as np

from ._abi import P3DError, _check, lib
from ._device_args import NEAREST_K_MAX, _device_rows, _device_vector
from .device_queries import _device_query
from ._host_args import _host_filter, _host_query, _per_row, _row_pair
from .filtered import _device_filter
from .sweep import _refuse_by_host_scene

_ORDER = ("count", "object", "dist", "param", "on_segment", "closest", "normal")


def _nearest_segment_k_outputs(k):
    """name -> (dtype, columns) of p3d_nearest_segment_k_device's outputs for this k: k rows per segment"""
    return {"count": ("int32", None), "object": ("int32", k), "dist": ("float32", k), "param": ("float32", k),
            "on_segment": ("float32", (k, 3)), "closest": ("float32", (k, 3)), "normal": ("float32", (k, 3))}


def nearest_segment_k_device(scene, accel, a, b, k, max_dist=None, skip=None, skip_range=None, want=("count", "object", "dist", "param"), stream=0,
                             out=None, n_skip=None):
    """p3d_nearest_segment_k_device: the k nearest surfaces to n segments held in device memory, in the DeviceScene `scene`,
    enqueued on `stream` without a wait.  a, b: float32 (n, 3) CUDA/HIP tensors (or raw (address, rows) pairs), the segments'
    ends; max_dist: float32 (n,) or None (for a capsule: its radius); skip, skip_range, n_skip: as nearest_k_filtered_device ->
    {name: tensor}: "count" int32 (n,) and "object" int32 (n, k), always there, and of "dist", "param" (n, k), "on_segment",
    "closest" and "normal" (n, k, 3) those named in `want`.  Rows behind count: -1, FLT_MAX, zeros.  ACCEL_NONE and ACCEL_BVH;
    ACCEL_GRID, a scene that holds a box, and ACCEL_BVH over a scene that holds a plane are refused with P3D_ERR_UNSUPPORTED - by
    this function already where the scene came from a HostScene.  `out`, `stream` and the other refusals as
    nearest_k_filtered_device; the answers are host_nearest_segment_k's, bit for bit."""
    who = "nearest_segment_k_device"
    k = int(k)
    names = ["count", "object"] + [w for w in _ORDER[2:] if w in want]
    _refuse_by_host_scene(scene, who, accel, "no nearest-surface query through the grid (use ACCEL_BVH or ACCEL_NONE)",
                          "the scene holds a box: a segment against a box's faces is not part of this query")
    refusal = None
    if out is None and not 1 <= k <= NEAREST_K_MAX:  # (with the caller's outputs the library says it)
        refusal = "k must be 1 .. %d, got %d" % (NEAREST_K_MAX, k)

    def inputs():
        d_a, n = _device_rows(a, who + ": a", 3, ("float32",), scene.device)
        d_b, n_b = _device_rows(b, who + ": b", 3, ("float32",), scene.device)
        d_m, n_m = _device_vector(max_dist, who + ": max_dist", ("float32",), scene.device) if max_dist is not None else (None, n)
        if n_b != n or n_m != n:
            raise P3DError(-1, "%s: %d a rows, %d b rows%s" % (who, n, n_b, "" if max_dist is None else ", %d limits" % n_m))
        return (d_a, d_b, d_m) + _device_filter(scene, who, skip, n_skip, skip_range, n, "segments") + (n,)

    return _device_query(scene, who, accel, inputs, _nearest_segment_k_outputs(max(k, 0)), names, want, _ORDER, stream, out, a, "segments", k=k,
                         refusal=refusal)


def host_nearest_segment_k(host_scene, a, b, k, max_dist=None, skip=None, skip_range=None):
    """p3d_host_scene_nearest_segment_k: the same on the CPU, by brute force over every object of the HostScene `host_scene` in
    object order -> (count int32 (n,), object int32 (n, k), dist float32 (n, k), param float32 (n, k), on_segment float32
    (n, k, 3), closest float32 (n, k, 3)).  skip: int32 (n, s), s <= FILTER_SKIP_MAX; skip_range: int32 (n, 2); either may be
    None.  A scene that holds a box is refused (P3D_ERR_UNSUPPORTED)."""
    who = "host_nearest_segment_k"
    pa, pb = _row_pair(who, "a", a, "b", b)
    n, k = len(pa), int(k)
    args = (k & 0xffffffff, pa, pb, _per_row(who, max_dist, n, "segments", "limits")) + _host_filter(who, skip, skip_range, n, "segments")
    return _host_query(host_scene, "nearest_segment_k", n, args, _nearest_segment_k_outputs(max(k, 0)), _ORDER[:-1])


def segment_box_d2(a, b, lo, hi):
    """p3d_debug_segment_box_d2: the rule's lower bound of the squared distance from each segment a[i] b[i] to the box
    lo[i] .. hi[i] (float32 (n, 3) each) -> float32 (n,): the key of a BVH node under this query.  No scene, no device."""
    arrays = [np.ascontiguousarray(x, np.float32) for x in (a, b, lo, hi)]
    if arrays[0].ndim != 2 or arrays[0].shape[1] != 3 or any(x.shape != arrays[0].shape for x in arrays):
        raise P3DError(-1, "segment_box_d2: %r, needed: four (n, 3) arrays" % ([x.shape for x in arrays],))
    out = np.zeros(len(arrays[0]), np.float32)
    _check(lib().p3d_debug_segment_box_d2(len(out), *(x.ctypes.data for x in arrays), out.ctypes.data))
    return out
