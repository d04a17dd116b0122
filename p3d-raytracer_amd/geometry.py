"""CPU geometry in numpy: what the device updates compute for a host scene that follows them, and the SAH cost of a tree."""
import numpy as np


def _xform_arrays(ranges, xforms, sphere_scale):
    """(ranges as (n, 3) int64, xforms as (k, 12) float32, sphere_scale as (k,) float32) of the arguments of
    transformed / DeviceScene.transform_prims"""
    r = np.asarray(list(ranges), np.int64).reshape(-1, 3)
    m = np.ascontiguousarray(xforms, np.float32)
    if m.ndim == 3 and m.shape[1:] == (3, 4):
        m = m.reshape(-1, 12)
    if m.ndim != 2 or m.shape[1] != 12:
        raise ValueError("xforms: an (n, 3, 4) or (n, 12) array is needed, got shape %r" % (m.shape,))
    sc = np.ones(len(m), np.float32) if sphere_scale is None else np.ascontiguousarray(sphere_scale, np.float32).reshape(-1)
    if len(sc) != len(m):
        raise ValueError("sphere_scale: %d values for %d transforms" % (len(sc), len(m)))
    return r, m, sc


def transformed(prim_type, prim_v, ranges, xforms, sphere_scale=None):
    """What p3d_scene_transform_prims computes for the nine geometry floats, stated in numpy float32, one rounded operation
    at a time: -> (objects, new_v), the arguments of HostScene.set_geometry that bring a host scene along.  `ranges`: an
    iterable of (first, count, xform); `xforms`: (n, 3, 4) or (n, 12) float32, row-major; `sphere_scale`: n values, default
    1.  A point: x' = ((m0 x + m1 y) + m2 z) + m3; the vertices of a triangle, the centre of a sphere (radius' = radius *
    sphere_scale) and min / max of a box are points.  prim_v holds the REST geometry.  Planes are refused, and boxes unless
    the transform is a positive scale per axis and a translation."""
    r, m, sc = _xform_arrays(ranges, xforms, sphere_scale)
    prim_type = np.asarray(prim_type)
    v = np.ascontiguousarray(prim_v, np.float32).reshape(-1, 9)
    objects, rows = [], []
    for first, count, x in r:
        if count <= 0 or first < 0 or first + count > len(v) or not 0 <= x < len(m):
            raise ValueError("transformed: bad range (%d, %d, %d)" % (first, count, x))
        idx = np.arange(first, first + count)
        kind = prim_type[idx]
        if (kind == 3).any():
            raise ValueError("transformed: range (%d, %d) covers a plane" % (first, count))
        t = m[x].reshape(3, 4)
        if (kind == 2).any() and not ((np.diag(t[:, :3]) > 0).all() and (t[:, :3][~np.eye(3, dtype=bool)] == 0).all()):
            raise ValueError("transformed: range (%d, %d) covers a box, and transform %d is not positive-diagonal" % (first, count, x))
        out = v[idx].copy()
        for cols, k in (((0,), 0), ((0, 3, 6), 1), ((0, 3), 2)):
            sel = kind == k
            for c in cols:
                px, py, pz = v[idx, c][sel], v[idx, c + 1][sel], v[idx, c + 2][sel]
                for row in range(3):
                    out[sel, c + row] = ((t[row, 0] * px + t[row, 1] * py) + t[row, 2] * pz) + t[row, 3]
        sph = kind == 0
        out[sph, 3] = v[idx, 3][sph] * sc[x]
        objects.append(idx)
        rows.append(out)
    if not objects:
        return np.zeros(0, np.uint32), np.zeros((0, 9), np.float32)
    return np.concatenate(objects).astype(np.uint32), np.concatenate(rows).astype(np.float32)


def deformed(prim_v, first, positions, indices=None):
    """The host route of DeviceScene.update_triangles, a plain gather in numpy: triangle first + k takes the positions
    indices[k] of `positions` ((V, 3) float32), or 3k, 3k + 1, 3k + 2 without indices -> (objects, rows), the arguments of
    HostScene.set_geometry that bring a host scene along.  prim_v (the scene's (n, 9) geometry) bounds the range."""
    pos = np.ascontiguousarray(positions, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError("deformed: positions must be (V, 3), got shape %r" % (pos.shape,))
    if indices is None:
        if len(pos) % 3:
            raise ValueError("deformed: a soup needs 3 positions per triangle, got %d" % len(pos))
        idx = np.arange(len(pos), dtype=np.int64).reshape(-1, 3)
    else:
        idx = np.asarray(indices)
        if idx.ndim != 2 or idx.shape[1] != 3 or idx.dtype.kind not in "iu":
            raise ValueError("deformed: indices must be an integer (F, 3) array")
        idx = idx.astype(np.uint32).astype(np.int64) if idx.dtype.itemsize == 4 else idx.astype(np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(pos)):
            raise ValueError("deformed: an index is outside the %d positions" % len(pos))
    n = len(np.asarray(prim_v).reshape(-1, 9))
    if first < 0 or len(idx) == 0 or first + len(idx) > n:
        raise ValueError("deformed: objects [%d, %d) of %d" % (first, first + len(idx), n))
    return np.arange(first, first + len(idx), dtype=np.uint32), np.ascontiguousarray(pos[idx].reshape(-1, 9))


def deformed_spheres(prim_v, first, centre_radius):
    """The host route of DeviceScene.update_spheres: sphere first + k takes centre and radius centre_radius[k] ((N, 4)
    float32), the other five floats of its row stay -> (objects, rows) for HostScene.set_geometry."""
    cr = np.ascontiguousarray(centre_radius, np.float32)
    if cr.ndim != 2 or cr.shape[1] != 4:
        raise ValueError("deformed_spheres: centre_radius must be (N, 4), got shape %r" % (cr.shape,))
    v = np.ascontiguousarray(prim_v, np.float32).reshape(-1, 9)
    if first < 0 or len(cr) == 0 or first + len(cr) > len(v):
        raise ValueError("deformed_spheres: objects [%d, %d) of %d" % (first, first + len(cr), len(v)))
    rows = v[first:first + len(cr)].copy()
    rows[:, :4] = cr
    return np.arange(first, first + len(cr), dtype=np.uint32), rows


def tree_cost(tree):
    """The SAH cost p3d_scene_bvh_cost reports (include/p3d.h), evaluated in float64 on a tree with the bvh_* keys of
    DeviceScene.export_bvh() or HostScene.arrays(bvh=True): A = (dx dy + dy dz) + dz dx per node, inner nodes count once, a
    leaf once per object, over A(root).  No nodes or a root without area: 0."""
    lo, hi = np.asarray(tree["bvh_bmin"], np.float32).reshape(-1, 3), np.asarray(tree["bvh_bmax"], np.float32).reshape(-1, 3)
    if len(lo) == 0:
        return 0.0
    d = hi.astype(np.float64) - lo.astype(np.float64)
    area = (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0]
    count_leaf = np.asarray(tree["bvh_count_leaf"], np.uint32)
    weight = np.where(count_leaf & np.uint32(0x80000000), (count_leaf & np.uint32(0x7fffffff)).astype(np.float64), 1.0)
    return float((weight * area).sum() / area[0]) if area[0] > 0 else 0.0
