"""Overlap queries (include/p3d_overlap.h): the objects that touch an axis-aligned box.  overlap_box_device, a function of a
DeviceScene over device tensors, and host_overlap_box, the brute force on the CPU over a HostScene.  Functions and not members:
tests/python_api_surface.json holds both classes to the members they had.

Box i is the closed box lo[i] .. hi[i].  The answers are the number of objects the box overlaps and the (at most) k lowest
object indices among them, ascending; k = 0 is the count alone.  "Overlaps" means the surface nearest_device measures to - the
closed triangle, a sphere's shell, a box's faces, the plane; with solid=True spheres and boxes count as solids.  Touching
counts; a box with lo > hi on some axis, or with a NaN, finds nothing.  Filters (`skip`, `skip_range`) are filtered.py's."""
from ._abi import P3DError
from ._device_args import NEAREST_K_MAX, _device_rows
from .device_queries import _device_query
from ._host_args import _host_filter, _host_query, _row_pair
from .filtered import _device_filter
from .sweep import _refuse_by_host_scene

OVERLAP_SOLID = 1  # P3D_OVERLAP_SOLID
_ORDER = ("total", "object")


def _overlap_outputs(k):
    """name -> (dtype, columns) of p3d_overlap_box_device's outputs for this k: k rows per box, none for k = 0"""
    table = {"total": ("int32", None)}
    if k > 0:
        table["object"] = ("int32", k)
    return table


def overlap_box_device(scene, accel, lo, hi, k, skip=None, skip_range=None, solid=False, stream=0, out=None, n_skip=None):
    """p3d_overlap_box_device: the objects of the DeviceScene `scene` that n boxes held in device memory overlap, enqueued on
    `stream` without a wait.  lo, hi: float32 (n, 3) CUDA/HIP tensors (or raw (address, rows) pairs), the boxes' corners; k: 0 ..
    NEAREST_K_MAX; skip, skip_range, n_skip: as nearest_k_filtered_device (a body asks with its own box and skips its own
    range) -> {"total": int32 (n,), "object": int32 (n, k)}: the number of overlapping objects and the lowest k of them,
    ascending, -1 behind them; "object" is left out for k = 0.  ACCEL_NONE and ACCEL_BVH; ACCEL_GRID and ACCEL_BVH over a scene
    that holds a plane are refused with P3D_ERR_UNSUPPORTED - by this function already where the scene came from a HostScene.
    `out`, `stream` and the other refusals as nearest_k_filtered_device; the answers are host_overlap_box's, bit for bit."""
    who = "overlap_box_device"
    k = int(k)
    _refuse_by_host_scene(scene, who, accel, "no overlap query through the grid (use ACCEL_BVH or ACCEL_NONE)", None)
    refusal = None
    if out is None and not 0 <= k <= NEAREST_K_MAX:  # (with the caller's outputs the library says it)
        refusal = "k must be 0 .. %d, got %d" % (NEAREST_K_MAX, k)

    def inputs():
        d_lo, n = _device_rows(lo, who + ": lo", 3, ("float32",), scene.device)
        d_hi, n_hi = _device_rows(hi, who + ": hi", 3, ("float32",), scene.device)
        if n_hi != n:
            raise P3DError(-1, "%s: %d lo rows, %d hi rows" % (who, n, n_hi))
        return (d_lo, d_hi) + _device_filter(scene, who, skip, n_skip, skip_range, n, "boxes") + (n,)

    table = _overlap_outputs(max(k, 0))
    return _device_query(scene, who, accel, inputs, table, list(table), (), _ORDER, stream, out, lo, "boxes", k=k, refusal=refusal,
                         options=(OVERLAP_SOLID if solid else 0,))


def host_overlap_box(host_scene, lo, hi, k, skip=None, skip_range=None, solid=False):
    """p3d_host_scene_overlap_box: the same on the CPU, by brute force over every object of the HostScene `host_scene` in object
    order -> (total int32 (n,), object int32 (n, k)).  skip: int32 (n, s), s <= FILTER_SKIP_MAX; skip_range: int32 (n, 2); either
    may be None."""
    who = "host_overlap_box"
    plo, phi = _row_pair(who, "lo", lo, "hi", hi)
    n, k = len(plo), int(k)
    args = (k & 0xffffffff, plo, phi) + _host_filter(who, skip, skip_range, n, "boxes") + (OVERLAP_SOLID if solid else 0,)
    return _host_query(host_scene, "overlap_box", n, args, {"total": ("int32", None), "object": ("int32", min(max(k, 0), NEAREST_K_MAX))}, _ORDER)
