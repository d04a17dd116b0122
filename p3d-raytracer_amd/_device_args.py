"""Arguments of the device-buffer calls: tensors (or raw (address, rows) pairs) checked before the library sees them, and the
tables of the queries' outputs."""
from ._abi import P3DError


def _device_rows(x, what, cols, dtypes, device):
    """(address, rows) of a contiguous (rows, cols) CUDA/HIP torch.Tensor of one of `dtypes` on `device`, or of a raw
    (address, rows) pair, which is taken at its word.  Anything else: P3DError, and the library is not called."""
    if isinstance(x, tuple) and len(x) == 2 and not hasattr(x[0], "data_ptr"):
        ptr, rows = int(x[0]), int(x[1])
        if ptr <= 0 or rows <= 0:
            raise P3DError(-1, "%s: a raw pair needs an address and a row count > 0" % what)
        return ptr, rows
    if not (hasattr(x, "data_ptr") and hasattr(x, "is_cuda")):
        raise P3DError(-1, "%s: a CUDA/HIP torch.Tensor or an (address, rows) pair is needed, got %s" % (what, type(x).__name__))
    if str(x.dtype).replace("torch.", "") not in dtypes:
        raise P3DError(-1, "%s: dtype %s, needed: %s" % (what, x.dtype, " or ".join(dtypes)))
    if x.dim() != 2 or x.shape[1] != cols or x.shape[0] == 0:
        raise P3DError(-1, "%s: shape %r, needed: (n, %d) with n > 0" % (what, tuple(x.shape), cols))
    if not x.is_contiguous():
        raise P3DError(-1, "%s: the tensor is not contiguous" % what)
    if not x.is_cuda:
        raise P3DError(-1, "%s: the tensor is in host memory (device %s)" % (what, x.device))
    if x.device.index is not None and x.device.index != device:
        raise P3DError(-1, "%s: the tensor is on device %d, the scene on device %d" % (what, x.device.index, device))
    return int(x.data_ptr()), int(x.shape[0])


def _device_vector(x, what, dtypes, device):
    """_device_rows for one value per row: a contiguous (rows,) tensor, or a raw (address, rows) pair"""
    if hasattr(x, "data_ptr") and hasattr(x, "dim"):
        if x.dim() != 1:
            raise P3DError(-1, "%s: shape %r, needed: (n,) with n > 0" % (what, tuple(x.shape)))
        x = x.unsqueeze(1)  # (a strided vector stays non-contiguous)
    return _device_rows(x, what, 1, dtypes, device)


def _device_blocks(x, what, tail, dtypes, device):
    """_device_rows for a block of values per row: a contiguous (rows,) + tail tensor (tail: two sizes), or a raw (address, rows) pair"""
    if hasattr(x, "data_ptr") and hasattr(x, "dim"):
        if x.dim() != 3 or tuple(x.shape[1:]) != tuple(tail):
            raise P3DError(-1, "%s: shape %r, needed: (n, %d, %d) with n > 0" % (what, tuple(x.shape), tail[0], tail[1]))
        if x.is_contiguous():
            x = x.view(x.shape[0], tail[0] * tail[1])
        else:
            raise P3DError(-1, "%s: the tensor is not contiguous" % what)
    return _device_rows(x, what, tail[0] * tail[1], dtypes, device)


_TRACE_OUTPUTS = {"hit_id": ("int32", None), "t": ("float32", None), "hit_point": ("float32", 3), "normal": ("float32", 3)}
_NEAREST_OUTPUTS = {"object": ("int32", None), "dist": ("float32", None), "closest": ("float32", 3), "normal": ("float32", 3)}
NEAREST_K_MAX = 16  # P3D_NEAREST_K_MAX


def _nearest_k_outputs(k):
    """name -> (dtype, columns) of p3d_nearest_k_device's outputs for this k: k rows per point"""
    return {"count": ("int32", None), "object": ("int32", k), "dist": ("float32", k), "closest": ("float32", (k, 3)), "normal": ("float32", (k, 3))}


TRACE_HITS_K_MAX = 16  # P3D_TRACE_HITS_K_MAX


def _trace_hits_outputs(k):
    """name -> (dtype, columns) of p3d_trace_hits_device's outputs for this k: k rows per ray (k = 0: the count alone)"""
    rows = {"count": ("int32", None), "object": ("int32", k), "t": ("float32", k), "hit_point": ("float32", (k, 3)), "normal": ("float32", (k, 3))}
    return dict(rows if k else {}, total=("int32", None))


RADIANCE_MAX_DEPTH = 16  # P3D_RADIANCE_MAX_DEPTH
RADIANCE_SKYBOX = 1      # P3D_RADIANCE_SKYBOX
_RADIANCE_OUTPUTS = {"rgb": ("float32", 3), "hit_id": ("int32", None)}
_CAMERA_RAYS_OUTPUTS = {"origin": ("float32", 3), "direction": ("float32", 3)}
PATH_ACCUMULATE = 2      # P3D_PATH_ACCUMULATE
PATH_MAX_DEPTH = 1024    # of a path-traced frame
_PATH_OUTPUTS = {"rgb": ("float32", 3), "hit_id": ("int32", None)}
_CAMERA_SAMPLE_RAYS_OUTPUTS = {"origin": ("float32", 3), "direction": ("float32", 3), "rng": ("int64", 2)}
OCCLUSION_ACCUMULATE = 1  # P3D_OCCLUSION_ACCUMULATE
_OCCLUSION_OUTPUTS = {"unoccluded": ("int32", None), "bent": ("float32", 3)}  # (the uint32 counts as int32 tensors)
_OCCLUSION_RAYS_OUTPUTS = {"origin": ("float32", 3), "direction": ("float32", 3)}
_SWEEP_OUTPUTS = {"object": ("int32", None), "t": ("float32", None), "centre": ("float32", 3), "contact": ("float32", 3), "normal": ("float32", 3)}
