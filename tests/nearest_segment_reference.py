"""A float64 model of the nearest-surfaces-to-a-segment query (p3d_host_scene_nearest_segment_k, p3d_nearest_segment_k_device,
include/p3d_segment.h), stated differently from the rule of host/nearest_segment_rule.hpp so that a mistake shared by the host
form and the kernel cannot hide behind their bit parity.  There is NO closest-pair case analysis here: the distance from a
segment a b to an object is the minimum over s in [0, 1] of nearest_reference's POINT distance at a + s (b - a).

  triangle, plane  that function of s is convex (the distance to a convex set along a line): its minimum by golden-section
                   search in float64, down to an interval of 1e-12
  sphere           g(s) = |x(s) - c| is convex: its minimum from nearest_reference._segment, its maximum at the endpoints;
                   the distance is 0 if min g <= r <= max g, min g - r outside, r - max g inside

Only DISTANCES are modelled.  Distance is continuous in a and b, so the checks need no conditioning margin; ties are held to
"the reported object is as near as the model's nearest".  Limits are nearest_reference.draw_limits's: never within 10 % of the
distance they decide.

The minimum over a whole scene is not taken over every (object, segment) pair: the point distance is 1-Lipschitz, so an
object is no nearer to the segment than its distance at the midpoint less half the length, and the scene's minimum is no
larger than the smallest midpoint distance.  An object whose midpoint distance exceeds that smallest one by more than half the
length cannot be the nearest; the search leaves out those that exceed it by more than the WHOLE length.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import numpy as np

import intersect_reference as ref
import nearest_reference as near

SPHERE, TRIANGLE, BOX, PLANE = ref.SPHERE, ref.TRIANGLE, ref.BOX, ref.PLANE
N_SEGMENTS = near.N_POINTS
FLT_MAX = near.FLT_MAX
INTERVAL = 1e-12
EVERY_PIERCE, EVERY_POINT = 5, 7  # a fifth of the segments are built to pierce; every seventh of the others has a == b

# Measured: the largest error over the fixed segment sets of test_nearest_segment_reference.py (host_nearest_segment_k on the
# CPU against this model; the GPU must equal its bits), as intersect_reference.rel_err counts it: |got - want| / max(1, |want|).
# The asserted tolerance is 4 x the measured maximum: room for another seed or scene, not for another implementation.
MEASURED = {
    "dist": 5.67e-7,        # (a) dist against the model's minimum (worst: mixed_planes)
    "object": 2.72e-13,     # (b) the model's distance to the reported object against that minimum: two triangles that share the
                            #     nearest edge, each searched down to its own last interval
    "on_surface": 7.55e-7,  # (c) the point model's distance from the reported closest point to the reported object, against 0
                            #     (worst: planes, where a crossing far from the origin is rounded to float32)
    "closest": 1.18e-7,     # (d) |on_segment - closest| against dist
    "on_segment": 1.49e-7,  # (e) on_segment against a + (b - a) param
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}


# ---- the model ------------------------------------------------------------------------------------------------------------------

def _golden(f, k):
    """min over s in [0, 1] of the convex f, for k independent problems at once: f(s (k,)) -> (k,).  Every value f returns is
    the distance from SOME point of the segment, so the smallest one seen is never below the true minimum"""
    g = (np.sqrt(5.0) - 1.0) / 2.0
    lo, hi = np.zeros(k), np.ones(k)
    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
    f1, f2 = f(x1), f(x2)
    best = np.minimum(np.minimum(f(lo), f(hi)), np.minimum(f1, f2))
    while k and (hi - lo).max() > INTERVAL:
        left = f1 < f2  # the minimum lies in [lo, x2]; otherwise in [x1, hi]
        lo, hi = np.where(left, lo, x1), np.where(left, x2, hi)
        x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
        fresh = f(np.where(left, x1, x2))
        f1, f2 = np.where(left, fresh, f2), np.where(left, f1, fresh)
        best = np.minimum(best, fresh)
    return best


def _triangle_pairs(p0, p1, p2, x):
    """nearest_reference.triangles for PAIRS (triangle k, point k): the distance does not change under a translation, so
    triangle k moved by -x[k] against the origin"""
    return near.triangles(p0 - x, p1 - x, p2 - x, np.zeros((1, 3)))[:, 0]


def pair_distance(objects, j, a, b):
    """The model's distance from segment a[k] b[k] to object j[k], for k pairs (float64)"""
    j, a, b = np.asarray(j), np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty(len(j))
    kinds = np.array([ob["kind"] for ob in objects])[j] if len(j) else np.zeros(0, int)
    tri = np.nonzero(kinds == TRIANGLE)[0]
    if len(tri):
        p0, p1, p2 = (np.stack([objects[i][key] for i in j[tri]]) for key in ("p0", "p1", "p2"))
        at, bt = a[tri], b[tri]
        out[tri] = _golden(lambda s: _triangle_pairs(p0, p1, p2, at + s[:, None] * (bt - at)), len(tri))
    for i in np.unique(j[kinds != TRIANGLE]) if len(j) else ():
        ob, m = objects[i], np.nonzero(j == i)[0]
        am, bm = a[m], b[m]
        assert ob["kind"] in (SPHERE, PLANE), "a box is not part of the segment query"
        if ob["kind"] == PLANE:
            out[m] = _golden(lambda s: near.distance(ob, am + s[:, None] * (bm - am)), len(m))
        else:
            g_min = near._segment(am, bm, ob["c"][None])[:, 0]
            g_max = np.maximum(near._norm(am - ob["c"]), near._norm(bm - ob["c"]))
            out[m] = np.where(g_min > ob["r"], g_min - ob["r"], np.where(g_max < ob["r"], ob["r"] - g_max, 0.0))
    return out


def scene_minimum(objects, a, b, also=None, leave_out=None):
    """-> (d_min (n,), d_also (n,)): the model's smallest distance from each segment to the scene, and its distance to the
    object also[i] (-1: none, NaN).  leave_out: (objects, n) bool, objects a segment's filter names (never the nearest)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = len(a)
    mid, length = (a + b) / 2, near._norm(b - a)
    tab = near.table(objects, mid)
    if leave_out is not None:
        tab = np.where(leave_out, np.inf, tab)
    maybe = tab <= tab.min(0) + length * (1 + 1e-9) + 1e-300
    j, i = np.nonzero(maybe)
    d = pair_distance(objects, j, a[i], b[i])
    d_min = np.full(n, np.inf)
    np.minimum.at(d_min, i, d)
    d_also = np.full(n, np.nan)
    if also is not None:
        has = np.nonzero(np.asarray(also) >= 0)[0]
        d_also[has] = pair_distance(objects, np.asarray(also)[has], a[has], b[has])
    return d_min, d_also


# ---- the fixed inputs (shared by the CPU and the GPU suite) -----------------------------------------------------------------------

def _pierce(ob, length, rng):
    """A segment of about this length through the object's surface: a triangle's interior (every barycentric coordinate at
    least 0.1, so that the float32 rounding of the ends cannot carry the crossing over an edge) along its normal, a sphere's
    shell along a radius, a plane along its normal; each side of the surface gets 5 % to 50 % of the length"""
    before, behind = length * rng.uniform(0.05, 0.5, 2)
    if ob["kind"] == SPHERE:
        u = ref._unit(rng, 1)[0]
        x = ob["c"] + ob["r"] * u
    else:
        if ob["kind"] == TRIANGLE:
            w = 0.1 + 0.7 * rng.dirichlet((1.0, 1.0, 1.0))
        else:
            w = np.array([0.0, *rng.uniform(-2, 2, 2)])
            w[0] = 1.0 - w[1] - w[2]
        x = w[0] * ob["p0"] + w[1] * ob["p1"] + w[2] * ob["p2"]
        u = np.cross(ob["p1"] - ob["p0"], ob["p2"] - ob["p0"])
        u = u / np.linalg.norm(u)
    if rng.integers(0, 2):
        u = -u
    return x + before * u, x - behind * u


def scene_segments(objects, seed, n=N_SEGMENTS):
    """n float32 segments -> (a, b, pierced): starts uniform in the scene's bounds grown by 10 %, directions uniform, lengths
    log-uniform from 0.1 % to 30 % of the diagonal.  Every EVERY_PIERCE-th (from 0) is built to pierce the object pierced[i] (-1
    elsewhere); of the others every EVERY_POINT-th (from 1) has b == a"""
    rng = np.random.default_rng(seed)
    lo, hi = near.scene_bounds(objects)
    mid, half, diag = (lo + hi) / 2, (hi - lo) / 2, float(np.linalg.norm(hi - lo))
    length = diag * np.exp(rng.uniform(np.log(1e-3), np.log(0.3), n))
    a = mid + 1.1 * half * rng.uniform(-1, 1, (n, 3))
    b = a + ref._unit(rng, n) * length[:, None]
    pierced = np.full(n, -1, np.int32)
    for i in range(0, n, EVERY_PIERCE):
        pierced[i] = rng.integers(0, len(objects))
        a[i], b[i] = _pierce(objects[pierced[i]], length[i], rng)
    a, b = a.astype(np.float32), b.astype(np.float32)
    point = (np.arange(n) % EVERY_POINT == 1) & (pierced < 0)
    b[point] = a[point]
    return np.ascontiguousarray(a), np.ascontiguousarray(b), pierced


# ---- the assertions ---------------------------------------------------------------------------------------------------------------

def check_segments(objects, a, b, pierced, got, what, tol=None):
    """got = (count, object, dist, param, on_segment, closest) at k = 1, without a limit or a filter -> the five measured errors.
    (f), the pierce-built segments, is exact and leaves no case out"""
    tol = TOL if tol is None else tol
    count, obj, dist, param, on_segment, closest = (np.asarray(v) for v in got)
    n = len(a)
    assert (count == 1).all() and (obj[:, 0] >= 0).all() and (obj[:, 0] < len(objects)).all(), what + ": a segment without an answer"
    obj, dist, param, x, q = obj[:, 0], dist[:, 0], param[:, 0], on_segment[:, 0].astype(np.float64), closest[:, 0].astype(np.float64)
    a64, b64 = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d_min, d_obj = scene_minimum(objects, a, b, also=obj)
    on = np.zeros(n)
    for j in np.unique(obj):
        m = obj == j
        on[m] = near.distance(objects[j], q[m])
    err = {
        "dist": float(ref.rel_err(dist, d_min).max()),
        "object": float(ref.rel_err(d_obj, d_min).max()),
        "on_surface": float(on.max()),
        "closest": float(ref.rel_err(near._norm(x - q), dist).max()),
        "on_segment": float(ref.rel_err(x, a64 + (b64 - a64) * param.astype(np.float64)[:, None]).max()),
    }
    print("%s: %d segments, errors %s (tolerances %s)" % (what, n, {k: "%.3g" % v for k, v in err.items()}, {k: "%.3g" % v for k, v in tol.items()}))
    assert (param >= 0).all() and (param <= 1).all(), what + ": a parameter outside [0, 1]"
    # (f): the pierced object at distance exactly 0 - or a lower index at exactly 0, which the model must put at 0 as well
    built = np.nonzero(pierced >= 0)[0]
    assert len(built) >= n // EVERY_PIERCE
    assert (dist[built] == 0).all() and not np.signbit(dist[built]).any(), "%s: %d pierce-built segments are not at distance 0, first %d" % (
        what, int((dist[built] != 0).sum()), int(built[dist[built] != 0][0]) if (dist[built] != 0).any() else -1)
    other = built[obj[built] != pierced[built]]
    assert (obj[other] < pierced[other]).all(), what + ": a pierce-built segment reports a higher index than the pierced object"
    assert (d_obj[other] <= tol["dist"]).all(), what + ": an object reported in front of the pierced one is not at distance 0 for the model"
    assert (x[built] == q[built]).all(), what + ": a crossing has x != q"
    for k, v in err.items():
        assert v <= tol[k], "%s: %s is off by %g, tolerance %g" % (what, k, v, tol[k])
    return err
