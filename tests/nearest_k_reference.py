"""Helpers that hold the k-nearest query (p3d_host_scene_nearest_k, p3d_nearest_k_device, include/p3d.h) to the float64 model
of nearest_reference.py (its `table`: the distance from every object to every point, not restated here).

The model gives distances only, so a k-nearest answer is held to it through what is continuous in the per-object errors:

  order statistics  the j-th reported distance against the model's j-th smallest distance.  The j-th smallest of a set of
                    numbers moves by at most the largest change of any of them (order statistics are 1-Lipschitz), so ties -
                    the triangles round a shared vertex - need no exclusion
  reported object   the model's distance to the object a row names, against the row's distance
  closest point     it lies on the object the row names, at the row's distance from the point
  count             bracketed, not decided: with T = THRESHOLD, #(d < limit (1 - T)) <= |S| <= #(d < limit (1 + T)).  (Leaving
                    out the points where some object lies within T of the limit, as check_limited does for the nearest one,
                    fails its 5 % cap on the triangle mesh: 5 - 16 % of the points, because shared vertices put many triangles
                    at one distance.)  No case is left out.

and through what is exact: the order inside a row, the distinct objects, and the no-answer values of the rows behind count."""
import numpy as np

import intersect_reference as ref
import nearest_reference as near

THRESHOLD = ref.THRESHOLD
FLT_MAX = near.FLT_MAX
KS = (1, 4, 16)

# Measured: the largest error of HostScene.nearest_k on the CPU over the fixed sets of test_nearest_k_reference.py (the five
# scenes and seeds of test_nearest_reference.py, N_POINTS points, k = 1, 4 and 16, without limits and with draw_k_limits),
# counted as intersect_reference.rel_err counts it: |got - want| / max(1, |want|).  nearest_reference.TOL was measured for the
# nearest object only and is not reused.  The asserted tolerance is 4 x the measured maximum: room for another seed or scene,
# not for another implementation.  The yardstick is the float64 model, never the kernel (which must equal the host's bits).
MEASURED = {
    "dist": 1.52e-6,        # dist[:, j] against the model's j-th smallest distance (worst: mixed_planes, at every k)
    "object": 1.52e-6,      # the model's distance to the reported object against the reported dist (mixed_planes)
    "on_surface": 1.52e-6,  # the model's distance from the reported closest point to the reported object, against 0 (mixed_planes)
    "closest": 1.62e-7,     # |p - closest| against dist (mixed, k = 16)
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}


def sorted_table(tab, most=2 * max(KS)):
    """The model's `most` smallest distances per point, ascending: (min(most, objects), points)"""
    return np.sort(tab, axis=0)[:most]


def draw_k_limits(srt, k, seed):
    """One float32 limit per point: the model's r-th smallest distance, r uniform in [0, min(2 k, objects)), times a factor from
    nearest_reference.FACTORS (where that distance is under FLOOR: 10 x FLOOR for a factor under 1.5, else inf, as
    draw_limits does), then every 25th a zero, a negative number or a NaN in turn.  srt: sorted_table's, or the whole sorted
    table."""
    rng = np.random.default_rng(seed)
    n = srt.shape[1]
    r = rng.integers(0, min(2 * k, srt.shape[0]), n)
    factor = np.array(near.FACTORS)[rng.integers(0, len(near.FACTORS), n)]
    d = srt[r, np.arange(n)]
    with np.errstate(invalid="ignore"):
        lim = np.where(d < near.FLOOR, np.where(np.isfinite(factor) & (factor < 1.5), 10 * near.FLOOR, np.inf), d * factor)
    lim = lim.astype(np.float32)
    lim[0::75], lim[25::75], lim[50::75] = 0.0, -1.5, np.nan
    return lim


def count_bounds(tab, k, limits):
    """(least, most) count per point under float32 limits (None: no limit), as the model brackets it"""
    n_obj, n = tab.shape
    if limits is None:
        full = np.full(n, min(k, n_obj))
        return full, full
    lim = np.asarray(limits, np.float64)
    with np.errstate(invalid="ignore"):
        keeps = lim > 0  # a zero, a negative or a NaN limit keeps nothing
        lo = (tab < (lim * (1 - THRESHOLD))[None, :]).sum(0)
        hi = (tab < (lim * (1 + THRESHOLD))[None, :]).sum(0)
    return np.where(keeps, np.minimum(lo, k), 0), np.where(keeps, np.minimum(hi, k), 0)


def rule_d2(p, closest):
    """|p - q|^2 as the rule sums it (nearest_rule.hpp nearest_d2: float32, (dx dx + dy dy) + dz dz, no contraction): the d2 an
    answer was ordered by, recovered exactly from the closest point it reports.  p (n, 3), closest (n, k, 3) -> (n, k)"""
    x = np.asarray(p, np.float32)[:, None, :] - closest
    return (x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2]


def check_rows(p, k, got, what):
    """What is exact in an answer, whatever the scene: shapes and types, 0 <= count <= k; inside a row dist does not decrease,
    the objects are distinct and a tie goes to the lower index; the rows from count on hold the no-answer values.
    The tie is one of d2, the number the order is defined on, and d2 is recovered from the row itself (rule_d2; dist must be its
    float32 square root).  Equal DIST is not enough: sqrtf maps neighbouring d2 to one dist, and such a pair is ordered by its
    d2 whatever the indices (mixed_planes, k = 15, point 507: d2 0x1.0678b2p+4 of object 19 before 0x1.0678b4p+4 of object 4,
    both dist 4.050243).  So: (d2, object) ascends strictly along a row."""
    count, obj, dist, closest = got
    n = len(count)
    assert count.dtype == np.int32 and obj.dtype == np.int32 and dist.dtype == np.float32 and closest.dtype == np.float32, what
    assert obj.shape == (n, k) and dist.shape == (n, k) and closest.shape == (n, k, 3), what + ": shapes"
    assert ((count >= 0) & (count <= k)).all(), what + ": a count outside 0 .. k"
    filled = np.arange(k)[None, :] < count[:, None]
    pair = filled[:, 1:]  # rows j - 1 and j both filled
    assert (dist[:, 1:] >= dist[:, :-1])[pair].all(), what + ": dist decreases inside a row"
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = rule_d2(p, closest)
        assert d2.dtype == np.float32 and (np.sqrt(d2)[filled] == dist[filled]).all(), what + ": dist is not sqrtf of |p - closest|^2"
    assert (d2[:, 1:] >= d2[:, :-1])[pair].all(), what + ": d2 decreases inside a row"
    tie = pair & (d2[:, 1:] == d2[:, :-1])
    assert (obj[:, 1:] > obj[:, :-1])[tie].all(), what + ": equal d2, but the index does not ascend"
    assert (obj[filled] >= 0).all(), what + ": a filled row without an object"
    srt = np.sort(np.where(filled, obj, -1 - np.arange(k)[None, :]), axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), what + ": an object twice in one row"
    assert (obj[~filled] == -1).all() and (dist[~filled] == FLT_MAX).all(), what + ": the no-answer values"
    assert not closest[~filled].any() and not np.signbit(closest[~filled]).any(), what + ": the no-answer closest point"
    return filled


def check_k(objects, p, k, limits, got, what, tab=None):
    """got = (count, object, dist, closest) of a k-nearest query under float32 `limits` (None: no limit) against the model, no
    case left out -> the four measured errors (0 where no row is filled)"""
    count, obj, dist, closest = got
    tab = near.table(objects, p) if tab is None else tab
    n = len(p)
    assert len(count) == n and tab.shape == (len(objects), n)
    filled = check_rows(p, k, got, what)
    lo, hi = count_bounds(tab, k, limits)
    bad = (count < lo) | (count > hi)
    assert not bad.any(), "%s: %d counts outside the model's bracket, first at point %d: %d not in [%d, %d]" % (
        what, int(bad.sum()), int(np.nonzero(bad)[0][0]), int(count[bad][0]), int(lo[bad][0]), int(hi[bad][0]))
    assert (obj[filled] < len(objects)).all(), what + ": no such object"
    i, j = np.nonzero(filled)
    err = dict.fromkeys(MEASURED, 0.0)
    if len(i):
        srt = np.sort(tab, axis=0)[:k]
        o, d, q = obj[i, j], dist[i, j], closest[i, j].astype(np.float64)
        err["dist"] = float(ref.rel_err(d, srt[j, i]).max())
        err["object"] = float(ref.rel_err(tab[o, i], d).max())
        err["closest"] = float(ref.rel_err(near._norm(np.asarray(p, np.float64)[i] - q), d).max())
        on = np.zeros(len(i))
        for which in np.unique(o):
            m = o == which
            on[m] = near.distance(objects[which], q[m])
        err["on_surface"] = float(on.max())
    print("%s: %d points, k = %d, %d rows filled (count 0: %d, between: %d, k: %d), errors %s (tolerances %s)" % (
        what, n, k, len(i), int((count == 0).sum()), int(((count > 0) & (count < k)).sum()), int((count == k).sum()),
        {name: "%.3g" % v for name, v in err.items()}, {name: "%.3g" % v for name, v in TOL.items()}))
    for name, v in err.items():
        assert v <= TOL[name], "%s: %s is off by %g, tolerance %g" % (what, name, v, TOL[name])
    return err
