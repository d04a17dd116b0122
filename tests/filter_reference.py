"""Filters of the filtered queries (include/p3d_filter.h: p3d_nearest_k_filtered_device, p3d_sweep_sphere_filtered_device and their
host forms), stated in numpy and differently from host/filter_rule.hpp: which objects a batch's filters name, as one boolean
table; the float64 per-object tables of nearest_reference.table / sweep_reference.table with those entries set to "never", so
that the existing check_k / check_sweep hold a filtered answer to the model of the thinned scene; the filters both suites draw;
the unfiltered rows with the skipped objects taken out; and the vertices of a mesh with the triangles round each.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np

SKIP_MAX = 8  # P3D_FILTER_SKIP_MAX
N_SKIPS = (0, 1, 8)
FLT_MAX = np.finfo(np.float32).max


def skipped(n_objs, n, skip=None, skip_range=None):
    """(n_objs, n) bool: object j is named by query i's filter.  Python integers decide the range: no overflow to think about"""
    out = np.zeros((n_objs, n), bool)
    if skip is not None and np.asarray(skip).size:
        s = np.asarray(skip, np.int64)
        assert s.shape[0] == n and s.shape[1] <= SKIP_MAX
        for column in s.T:
            ok = (column >= 0) & (column < n_objs)  # anything else names nothing
            out[column[ok], np.nonzero(ok)[0]] = True
    if skip_range is not None:
        j = np.arange(n_objs)
        for i, (first, count) in enumerate(np.asarray(skip_range).tolist()):
            if count > 0:
                out[:, i] |= (j >= first) & (j < first + count)
    return out


def masked(table, skip, skip_range, never):
    """A per-object table (objects, queries) with the skipped entries set to `never`: inf for distances, NaN for contact times"""
    return np.where(skipped(table.shape[0], table.shape[1], skip, skip_range), never, table)


def objects_of(arrays, sphere=0, triangle=1):
    """The model's objects (intersect_reference.load_objects' dicts) of a scene of spheres and triangles from HostScene.arrays():
    for the golden fixtures, whose files hold lines the model's loader does not read"""
    out = []
    for kind, v in zip(arrays["prim_type"], np.asarray(arrays["prim_v"], np.float64)):
        assert kind in (sphere, triangle)
        out.append(dict(kind=int(kind), c=v[:3], r=float(v[3])) if kind == sphere else dict(kind=int(kind), p0=v[0:3], p1=v[3:6], p2=v[6:9]))
    return out


def holds_in_float32(objects, T, o, d, r, tol_centre, tol_t, plane=3):
    """(queries,) bool: float32 can hold the contact of this table (objects, queries; NaN: not met) to the tolerances of the
    unfiltered test, which are relative to max(1, r) and max(1, T) - not to the size of the coordinates, and not to how shallow
    an approach is.  With the obstacle in front skipped a ball flies on and may meet the next one - a plane has no end - far
    outside the scene or at a grazing angle, which the unfiltered sets, for which the tolerances were measured, do not hold
    (they reach |centre| = 85).  From the float64 model and the number format alone.  False where
      - half a float32 spacing of the model's centre at contact, 2^-24 max |o + T d|, exceeds tol_centre max(1, r): the
        centre's own rounding is larger than the tolerance on its distance from the object (planes: |centre| = 34 902, numbers
        3.9e-3 apart, 200 times the tolerance), or
      - the contact is with a plane and the bound on the rounding of the float32 dot product d.N, 3 x 2^-24 sum |d_k N_k|, is a
        larger share of |d.N| than tol_t: T is the height over that approach speed and takes its relative error (mixed_planes:
        cos(d, N) = 1.4e-3, the share 1.3e-4).
    A test gives such a query a filter that names nothing, so that it stays in the batch as an unfiltered case"""
    import intersect_reference as ref
    o, d, r = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(r, np.float64)
    filled = np.where(np.isnan(T), np.inf, T)
    which, first = filled.argmin(0), filled.min(0)
    met = np.isfinite(first)
    centre = o + np.where(met, first, 0.0)[:, None] * d
    coarse = 2.0 ** -24 * np.abs(centre).max(1) > tol_centre * np.maximum(1.0, r)
    shallow = np.zeros(len(o), bool)
    for j, ob in enumerate(objects):
        if ob["kind"] == plane:
            normal = ref.unit_normal(ob)
            with np.errstate(divide="ignore", invalid="ignore"):
                share = 3 * 2.0 ** -24 * (np.abs(d) * np.abs(normal)).sum(1) / np.abs(d @ normal)
            shallow |= (which == j) & ~(share <= tol_t)
    return ~(met & (coarse | shallow))


def emptied(skip, skip_range, rows):
    """The filters with those of `rows` (bool) made to name nothing: a list of -1, a range of count 0"""
    if skip is not None:
        skip = np.where(rows[:, None], np.int32(-1), skip).astype(np.int32)
    if skip_range is not None:
        skip_range = np.where(rows[:, None], np.int32(0), skip_range).astype(np.int32)
    return skip, skip_range


def draw(n, n_objs, n_skip, ranged, seed, answers=None):
    """The filters of n queries -> (skip int32 (n, n_skip) or None, skip_range int32 (n, 2) or None).
    answers: (n, >= n_skip) objects each query would find first (its nearest ones, or its contact in column 0; -1: none).  Then
    three rows in four skip THOSE - what a filter is for, and what changes the answer - and every fourth random objects; in
    every row of a list with room one slot is -1, one is past the object count and one repeats its neighbour, in turn.
    A range: first from -4 to n_objs + 1, count from -2 to a third of the scene; every 16th is (INT32_MAX - 1, INT32_MAX): a
    32-bit first + count would wrap to a negative end, or, from (-2^31, 2^31 - 1), to a range over everything"""
    rng = np.random.default_rng(seed)
    skip = None
    if n_skip:
        skip = rng.integers(0, n_objs, (n, n_skip)).astype(np.int32)
        if answers is not None:
            a = np.asarray(answers)[:, :n_skip]
            rows = np.arange(n) % 4 != 3
            skip[rows, :a.shape[1]] = a[rows]
        if n_skip >= 4:
            skip[0::3, n_skip - 1] = -1
            skip[1::3, n_skip - 2] = n_objs + rng.integers(0, 5, len(skip[1::3]))
            skip[2::3, n_skip - 3] = skip[2::3, n_skip - 4]
    skip_range = None
    if ranged:
        first = rng.integers(-4, n_objs + 2, n)
        count = rng.integers(-2, max(2, n_objs // 3), n)
        skip_range = np.stack([first, count], 1).astype(np.int32)
        skip_range[5::16] = (2 ** 31 - 2, 2 ** 31 - 1)
        skip_range[13::16] = (-2 ** 31, 2 ** 31 - 1)  # ends at -1: names nothing
    return skip, skip_range


def without(rows, skip, k):
    """rows = (count, object, dist, closest) of an UNFILTERED k-nearest query at some k' >= k -> the first k rows that survive
    the skip list, with their count and the no-answer values behind it: what the filtered query at k must equal where k' is
    large enough (k' >= k + the list's length: the longer list holds the k smallest survivors, or every object in reach)"""
    count, obj, dist, closest = rows
    n, wide = obj.shape
    keep = np.arange(wide)[None, :] < count[:, None]
    if skip is not None:
        keep &= ~(obj[:, :, None] == np.asarray(skip)[:, None, :]).any(2)
    order = np.argsort(~keep, axis=1, kind="stable")[:, :k]  # the kept rows first, in their order
    rows_i = np.arange(n)[:, None]
    kept = keep[rows_i, order]
    out_count = np.minimum(keep.sum(1), k).astype(np.int32)
    out_obj = np.where(kept, obj[rows_i, order], -1).astype(np.int32)
    out_dist = np.where(kept, dist[rows_i, order], FLT_MAX).astype(np.float32)
    out_closest = np.where(kept[:, :, None], closest[rows_i, order], np.float32(0)).astype(np.float32)
    return out_count, out_obj, out_dist, out_closest


def mesh_vertices(prim_type, prim_v, most=SKIP_MAX, triangle=1):
    """The distinct vertices of a scene's triangles that at most `most` triangles share -> (points float32 (V, 3), incident int32
    (V, most): the objects round each vertex, padded with -1)"""
    tri = np.nonzero(np.asarray(prim_type) == triangle)[0]
    corners = np.asarray(prim_v, np.float32)[tri, :9].reshape(-1, 3)
    points, inverse = np.unique(corners, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    round_vertex = [[] for _ in points]
    for corner, v in enumerate(inverse):
        obj = int(tri[corner // 3])
        if obj not in round_vertex[v]:
            round_vertex[v].append(obj)
    ok = np.array([len(objs) <= most for objs in round_vertex], bool)
    incident = np.array([objs + [-1] * (most - len(objs)) for objs in round_vertex if len(objs) <= most], np.int32).reshape(-1, most)
    return points[ok], incident
