"""Arguments of the host forms of the queries (p3d_host_scene_*): numpy arrays checked before the library sees them, zeroed
outputs from the tables of _device_args, and the one call all of them make."""
import numpy as np

from ._abi import P3DError, _check
from ._device_args import _nearest_k_outputs


def _refuse(error, msg):
    """The module functions raise P3DError(-1, ...); the HostScene methods pass error=ValueError"""
    raise P3DError(-1, msg) if error is None else error(msg)


def _address(a):
    return a.ctypes.data if a is not None and a.size else None


def _points(x):
    """float32 (n, 3) rows of anything that holds 3 n numbers"""
    return np.ascontiguousarray(x, np.float32).reshape(-1, 3)


def _row_pair(who, name_a, a, name_b, b):
    """Two float32 (n, 3) arrays of the same n, or P3DError"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.ndim != 2 or a.shape[1] != 3 or b.shape != a.shape:
        _refuse(None, "%s: %s %r and %s %r, needed: (n, 3) both" % (who, name_a, a.shape, name_b, b.shape))
    return a, b


def _per_row(who, x, n, rows_of, what, one_for_all=False, error=None):
    """One float32 per row - limits, radii - checked against the n `rows_of`; None stays None.  one_for_all: a single number
    stands for every row"""
    if x is None:
        return None
    if one_for_all and np.ndim(x) == 0:
        x = np.broadcast_to(np.asarray(x, np.float32), (n,))
    v = np.ascontiguousarray(x, np.float32).reshape(-1)
    if len(v) != n:
        _refuse(error, "%s: %d %s, %d %s" % (who, n, rows_of, len(v), what))
    return v


def _host_filter(who, skip, skip_range, n, rows_of):
    """(skip array or None, n_skip, skip_range array or None) of a host query of n rows: its three C arguments"""
    s, width = None, 0
    if skip is not None:
        s = np.ascontiguousarray(skip, np.int32)
        if s.ndim != 2 or len(s) != n:
            raise P3DError(-1, "%s: skip %r, needed: (%d, s) for %d %s" % (who, s.shape, n, n, rows_of))
        width = s.shape[1]
    r = None
    if skip_range is not None:
        r = np.ascontiguousarray(skip_range, np.int32)
        if r.shape != (n, 2):
            raise P3DError(-1, "%s: skip_range %r, needed: (%d, 2)" % (who, r.shape, n))
    return s, width, r


def _host_query(host_scene, form, n, args, table, names):
    """p3d_host_scene_<form>(scene, n, *args, *outputs) -> the outputs: zeroed arrays of n rows for `names` of a {name: (dtype,
    columns)} table (columns: None, k or (k, 3)).  Arrays among `args` (held by the caller) and the outputs go by address, null
    where one is None or empty; numbers go as they are"""
    def shape(columns):
        return (n,) + (() if columns is None else columns if isinstance(columns, tuple) else (columns,))
    out = tuple(np.zeros(shape(table[name][1]), table[name][0]) for name in names)
    call = [a if isinstance(a, int) else _address(a) for a in args] + [_address(o) for o in out]
    _check(getattr(host_scene._L, "p3d_host_scene_" + form)(host_scene._h, n, *call))
    return out


def _host_nearest_k(host_scene, who, points, k, max_dist, filters=None, error=None):
    """HostScene.nearest_k and, with filters = (skip, skip_range), filtered.host_nearest_k_filtered"""
    p = _points(points)
    n, k = len(p), int(k)
    m = _per_row(who, max_dist, n, "points", "limits", error=error)
    args, form = (k & 0xffffffff, p, m), "nearest_k"
    if filters is not None:
        args, form = args + _host_filter(who, filters[0], filters[1], n, "points"), "nearest_k_filtered"
    return _host_query(host_scene, form, n, args, _nearest_k_outputs(max(k, 0)), ("count", "object", "dist", "closest"))
