"""What the *_device queries of a DeviceScene share: their inputs and outputs resolved to addresses, and the one call."""
import ctypes as C

from ._abi import P3DError, _check, _stream
from ._device_args import _device_blocks, _device_rows, _device_vector


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


def _device_query(scene, who, accel, inputs, table, names, want, order, stream, out, like, rows_of="rays", k=None, known=None, refusal=None):
    """What the *_device queries share.  In this order: a name in `want` that `known` (default: `table`) does not hold is
    refused; inputs() gives the input addresses and, last, n; `refusal`, the caller's own (about k), is raised if there is
    one; the outputs `names` are resolved against `table`; and L.p3d_<who> is called with (scene, accel, n, [k,] inputs,
    the outputs in the C order `order` - null where not in names -, stream) -> {name: tensor}"""
    unknown = [w for w in want if w not in (table if known is None else known)]
    if unknown:
        raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
    *addresses, n = inputs()
    if refusal:
        raise P3DError(-1, "%s: %s" % (who, refusal))
    res = _device_outputs(scene, who, names, n, out, like, table, rows_of)
    args = ([] if k is None else [k & 0xffffffff]) + [C.c_void_p(a) for a in addresses]
    args += [C.c_void_p(res[name][1]) if name in res else None for name in order]
    _check(getattr(scene._L, "p3d_" + who)(scene._h, int(accel), n, *args, _stream(stream)))
    return {name: v[0] for name, v in res.items()}
