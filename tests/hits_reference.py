"""The hits in order along a ray (p3d_trace_hits_device, include/p3d.h): helpers the CPU and the GPU suite share.

    H = the objects whose per-object test (a fresh copy of the ray each) hits at t < limit, ordered by (t, object index)
    count = min(|H|, k), total = |H|, rows 0 .. count - 1 = the first entries of H

brute_hits builds the exact expected outputs from an implementation's per-object (hit, t) arrays
(segment_reference.per_object); model_hits does the same from the float64 model's table; all_hits_margin is the conditioning
of a ray whose WHOLE hit set matters (not only "is anything in front", as in segment_reference.occluded_within): every object
takes part.  Rays under intersect_reference.THRESHOLD are ill-conditioned and left out of a comparison between back ends.
Also here: the two scenes the random ones cannot stand in for - forty stacked slats, which fill a list of sixteen, and a
closed cube of twelve triangles, for the parity of the crossings."""
import numpy as np

import intersect_reference as ref
import segment_reference as seg

FLT_MAX = np.finfo(np.float32).max
K_MAX = 16


def _limits(t_max, n):
    return np.full(n, np.inf, np.float32) if t_max is None else np.asarray(t_max, np.float32)


def brute_hits(tests, t_max, k):
    """-> (count (n,) int32, total (n,) int32, object (n, k) int32, t (n, k) float32) from per_object's float32 arrays: the
    hits with t < t_max (float32's comparison: a NaN t, a NaN limit: not in; a limit <= 0 keeps nothing; None: no limit),
    sorted by (t, index); the rows behind count hold -1 and FLT_MAX"""
    hit, t = tests
    t = np.asarray(t, np.float32)
    n = hit.shape[1]
    lim = _limits(t_max, n)
    with np.errstate(invalid="ignore"):
        inside = hit & (t < lim[None, :]) & (lim > 0)[None, :]
    total = inside.sum(0).astype(np.int32)
    count = np.minimum(total, k).astype(np.int32)
    key = np.where(inside, t, np.float32(np.inf))
    order = np.argsort(key, axis=0, kind="stable")[:k]  # stable: equal t (-0.0 and 0.0 too) to the smaller index
    obj = np.full((n, k), -1, np.int32)
    ts = np.full((n, k), FLT_MAX, np.float32)
    rows = min(k, len(order))
    listed = (np.arange(rows)[:, None] < count[None, :])
    obj[:, :rows] = np.where(listed, order[:rows], -1).T
    ts[:, :rows] = np.where(listed, np.take_along_axis(t, order[:rows], 0), FLT_MAX).T
    return count, total, obj, ts


def model_hits(table, t_max, k):
    """The float64 model's answer from intersect_reference._all's table -> (total (n,), object (n, k), t (n, k)); -1 and NaN
    behind the model's count"""
    hit, t = table[:2]
    n = hit.shape[1]
    lim = _limits(t_max, n).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = hit & (t < lim[None, :]) & (lim > 0)[None, :]
    total = inside.sum(0)
    key = np.where(inside, t, np.inf)
    order = np.argsort(key, axis=0, kind="stable")[:k]
    rows = min(k, len(order))
    listed = (np.arange(rows)[:, None] < np.minimum(total, k)[None, :])
    obj = np.full((n, k), -1, np.int64)
    ts = np.full((n, k), np.nan)
    obj[:, :rows] = np.where(listed, order[:rows], -1).T
    ts[:, :rows] = np.where(listed, np.take_along_axis(t, order[:rows], 0), np.nan).T
    return total, obj, ts


def all_hits_margin(objects, o, d, t_max, table=None):
    """The margin of (n, 3) rays with unit directions and n limits (None: no limit) when every object's decision matters:
    the minimum over the objects of - a hit: the smaller of its own margin and its distance to the limit, |t - t_max| /
    max(1, t); a miss: its own margin, unless it is a miss whatever the last bits say or would be a hit behind the limit (the
    four `sure` tests of segment_reference.occluded_within).  A NaN limit: 0."""
    hit, t, margin, cand = table if table is not None else ref._all(objects, o, d)
    n = hit.shape[1]
    t_max = _limits(t_max, n).astype(np.float64)[None, :]
    s, gap = seg.reach(objects, o, d)
    radius = np.array([np.inf if ob["kind"] == ref.PLANE else ref.bounding_sphere(ob)[1] for ob in objects])[:, None]
    with np.errstate(invalid="ignore"):
        near = np.abs(t - t_max) / np.maximum(1.0, np.abs(t))  # NaN where t is (a miss), inf for an infinite limit
        near = np.where(np.isnan(near), 0.0, near)
        slack = ref.THRESHOLD * np.maximum(1.0, np.where(np.isfinite(t_max), np.abs(t_max), 1.0))
        sure = (gap >= ref.THRESHOLD) | (s + radius < -slack) | (s - radius > t_max + slack) | (cand > t_max + slack)
        m = np.where(hit, np.minimum(margin, near), np.where(sure, np.inf, margin)).min(0) if len(objects) else np.full(n, np.inf)
    return np.where(np.isnan(t_max[0]), 0.0, m)


def check_against_model(objects, o, d, t_max, k, got, what, table=None):
    """An implementation's (count, total, object, t) against the model on well-conditioned rays, under the 5 % cap: total is
    the model's count, the listed objects are the model's first k as a set, and their order is the model's wherever the model's
    consecutive t differ by more than THRESHOLD * max(1, t) -> rays left out.  Where the model's k-th and (k + 1)-th hits lie
    that close (a box standing on a plane: one t) "the first k" is not one set: every hit clearly in front of the k-th must
    be listed, and nothing clearly behind it may be."""
    table = table if table is not None else ref._all(objects, o, d)
    ok, left = ref.well_conditioned(all_hits_margin(objects, o, d, t_max, table), what)
    count, total, obj, _ = got
    m_total, m_obj, m_t = model_hits(table, t_max, len(objects))
    wrong = ok & (total != m_total)
    assert not wrong.any(), "%s: total differs from the model's on %d rays, first at ray %d" % (what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]))
    assert (count[ok] == np.minimum(m_total, k)[ok]).all(), what + ": count"
    for i in np.nonzero(ok & (count > 0))[0]:
        c, every = int(count[i]), int(m_total[i])
        listed, ts = obj[i, :c], m_t[i, :every]
        tol = ref.THRESHOLD * max(1.0, abs(ts[c - 1]))
        # (where the k-th and (k + 1)-th hits do not tie, `may` is exactly the model's first c objects and `listed` has c distinct
        # members: set equality)
        must, may = set(m_obj[i, :every][ts < ts[c - 1] - tol].tolist()), set(m_obj[i, :every][ts <= ts[c - 1] + tol].tolist())
        assert len(set(listed.tolist())) == c and must <= set(listed.tolist()) <= may, "%s: ray %d lists %r, the model %r" % (what, i, listed, m_obj[i, :c])
        apart = np.ones(c, bool)  # entries whose model t stands clear of both neighbours'
        close = np.diff(ts[:c + 1]) <= ref.THRESHOLD * np.maximum(1.0, np.abs(ts[:c + 1][:-1]))
        apart[1:] &= ~close[:c - 1]
        apart[:len(close)] &= ~close[:c]
        assert (listed[apart] == m_obj[i, :c][apart]).all(), "%s: ray %d is ordered %r, the model %r" % (what, i, listed, m_obj[i, :c])
    print("%s: %d rays, %d left out, up to %d hits on a ray" % (what, len(ok), left, int(m_total.max()) if len(m_total) else 0))
    return left


# ---- scenes -----------------------------------------------------------------------------------------------------------------------

N_SLATS = 40
SLAT_GAP = 0.25


def _triangles(tris):
    return "".join("p 3\n" + "".join("%r %r %r\n" % tuple(float(x) for x in v) for v in t) for t in tris)


def write_slats(path):
    """N_SLATS large triangles stacked SLAT_GAP apart along z, from z = 0 up: a ray along z crosses them all, in file order"""
    tris = [[(-10, -10, SLAT_GAP * i), (10, -10, SLAT_GAP * i), (0, 10, SLAT_GAP * i)] for i in range(N_SLATS)]
    with open(str(path), "w") as f:
        f.write(ref.HEAD + _triangles(tris))
    return str(path)


def slat_rays(seed, n):
    """n rays from below the stack, within 0.1 of the +z direction, through the interiors of all slats -> float32 (o, d)"""
    rng = np.random.default_rng(seed)
    o = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-1.5, -0.5, (n, 1))], axis=1).astype(np.float32)
    d = ref.normalize32(np.concatenate([rng.uniform(-0.07, 0.07, (n, 2)), np.ones((n, 1))], axis=1).astype(np.float32))
    return o, d


def slat_limits(table, seed):
    """One float32 limit per ray: halfway between two consecutive hits of the model (so that none lies near a hit), or inf"""
    hit, t = table[:2]
    rng = np.random.default_rng(seed)
    n = hit.shape[1]
    ts = np.sort(np.where(hit, t, np.inf), axis=0)
    m = rng.integers(0, len(ts), n)  # len - 1: behind the last pair -> no limit
    lo = ts[np.minimum(m, len(ts) - 2), np.arange(n)]
    hi = ts[np.minimum(m, len(ts) - 2) + 1, np.arange(n)]
    with np.errstate(invalid="ignore"):
        mid = np.where(m == len(ts) - 1, np.inf, (lo + hi) / 2)
    return np.where(np.isfinite(mid), mid, np.inf).astype(np.float32)


CUBE_HALF = 1.0
_CUBE_QUADS = [  # the six faces of [-1, 1]^3, each as four corners in order
    [(-1, -1, -1), (-1, 1, -1), (1, 1, -1), (1, -1, -1)], [(-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)],
    [(-1, -1, -1), (1, -1, -1), (1, -1, 1), (-1, -1, 1)], [(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)],
    [(-1, -1, -1), (-1, -1, 1), (-1, 1, 1), (-1, 1, -1)], [(1, -1, -1), (1, 1, -1), (1, 1, 1), (1, -1, 1)]]


def write_cube(path):
    """A closed mesh: the cube [-1, 1]^3 as twelve triangles (and nothing else)"""
    tris = [t for q in _CUBE_QUADS for t in ([q[0], q[1], q[2]], [q[0], q[2], q[3]])]
    with open(str(path), "w") as f:
        f.write(ref.HEAD + _triangles(tris))
    return str(path)


def cube_rays(seed, n):
    """n rays with seeded unit directions: the first half from points strictly inside the cube, at least 5 % of its size from
    every face, the rest from points outside it (between 1.1 and 3 half-sizes out along at least one axis) -> (o, d, inside)"""
    rng = np.random.default_rng(seed)
    h = n // 2
    inner = rng.uniform(-0.9, 0.9, (h, 3)) * CUBE_HALF  # 0.1 = 5 % of the cube's size, 2, from a face
    outer = rng.uniform(-3, 3, (n - h, 3)) * CUBE_HALF
    axis = rng.integers(0, 3, n - h)
    outer[np.arange(n - h), axis] = rng.choice([-1.0, 1.0], n - h) * rng.uniform(1.1, 3.0, n - h) * CUBE_HALF
    o = np.concatenate([inner, outer]).astype(np.float32)
    d = ref.normalize32(ref._unit(rng, n).astype(np.float32))
    return o, d, np.arange(n) < h
