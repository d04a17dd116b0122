"""The float64 statement of the segment query (p3d_trace_any_device with t_max, include/p3d.h), on the per-object tests of
intersect_reference.py:

    occluded = some object is hit at t < t_max            (unit directions: t is a distance for every kind)

and the helpers the CPU and the GPU suite share: the exact brute force over an implementation's per-object test, and the
seeded limits.  The margin of a ray is that of intersect_reference.occluded restricted to the hits in front of the limit,
and it also carries |t - t_max| / max(1, t) for every object whose decision the limit makes: a hit the limit keeps or drops.
Rays under intersect_reference.THRESHOLD are ill-conditioned and left out of a comparison with this model."""
import numpy as np

import intersect_reference as ref

FACTORS = (0.5, 0.9, 1.1, 2.0, np.inf)  # of the model's nearest hit: the limit never lies within 10 % of the hit it decides


def reach(objects, o, d):
    """For every object and ray: (s, gap) - where along the unit direction the centre of the object's bounding sphere projects,
    and by how much the ray's LINE misses that sphere, (distance - r) / max(1, r); a plane is everywhere: (0, -inf)."""
    o, d = ref._rows(o), ref._rows(d)
    dh = d / np.sqrt(ref._dot(d, d))[:, None]
    s, gap = np.zeros((len(objects), len(o))), np.full((len(objects), len(o)), -np.inf)
    for j, ob in enumerate(objects):
        if ob["kind"] == ref.PLANE:
            continue
        c, r = ref.bounding_sphere(ob)
        m = c - o
        s[j] = ref._dot(m, dh)
        perp = m - s[j][:, None] * dh
        gap[j] = (np.sqrt(ref._dot(perp, perp)) - r) / max(1.0, r)
    return s, gap


def occluded_within(objects, o, d, t_max, table=None):
    """-> (occluded, margin) for (n, 3) rays with unit directions and n limits (table: intersect_reference._all of the rays, if
    the caller has it).
    occluded ray: the best margin among the hits in front of the limit, each no better than its distance to the limit.
    free ray: the worst over the objects that could change the answer - a hit behind the limit: the smaller of its own margin
    (an origin on a sphere or on a box's face: t jumps) and its distance to the limit; a miss: its own margin, unless it is a
    miss whatever the last bits say, or would be a hit behind the limit: the ray's line passes the object's bounding sphere
    at more than THRESHOLD (of max(1, r)), that sphere lies wholly behind the origin or the limit, or the place the test
    names for the hit it might be (t_cand of intersect_reference) lies behind the limit."""
    hit, t, margin, cand = table if table is not None else ref._all(objects, o, d)
    t_max = np.asarray(t_max, np.float64)[None, :]
    s, gap = reach(objects, o, d)
    radius = np.array([np.inf if ob["kind"] == ref.PLANE else ref.bounding_sphere(ob)[1] for ob in objects])[:, None]
    with np.errstate(invalid="ignore"):
        near = np.abs(t - t_max) / np.maximum(1.0, np.abs(t))  # NaN where t is (a miss), inf for an infinite limit
        near = np.where(np.isnan(near), 0.0, near)
        kept = hit & (t < t_max)
        occ = kept.any(0)
        m_occ = np.where(kept, np.minimum(margin, near), -np.inf).max(0)
        slack = ref.THRESHOLD * np.maximum(1.0, np.where(np.isfinite(t_max), np.abs(t_max), 1.0))
        sure = (gap >= ref.THRESHOLD) | (s + radius < -slack) | (s - radius > t_max + slack) | (cand > t_max + slack)
        m_free = np.where(hit, np.minimum(margin, near), np.where(sure, np.inf, margin)).min(0)
    m = np.where(occ, m_occ, m_free)
    return occ, np.where(np.isnan(t_max[0]), 0.0, m)


def draw_limits(objects, o, d, seed, table=None):
    """One float32 limit per ray: the model's nearest-hit distance times a factor drawn from FACTORS, or, for a ray the model
    sees hit nothing, uniform in [0.5, 8]."""
    rng = np.random.default_rng(seed)
    hit, t = (table if table is not None else ref._all(objects, o, d))[:2]
    t_near = np.where(hit, t, np.inf).min(0)
    t_near = np.where(np.isfinite(t_near), t_near, np.nan)
    factor = np.array(FACTORS)[rng.integers(0, len(FACTORS), len(t_near))]
    free = rng.uniform(0.5, 8.0, len(t_near))
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(t_near), free, t_near * factor).astype(np.float32)


def per_object(intercepts_fn, n_objects, o, d):
    """(hit, t): two (objects, rays) arrays of an implementation's per-object test, every test on a fresh copy of the ray:
    intercepts_fn(j, origin, direction) -> (hit, t, ...) for ONE ray, e.g. oracle.binding.Scene.object_intercepts"""
    o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
    hit = np.zeros((n_objects, len(o)), bool)
    t = np.zeros((n_objects, len(o)), np.float32)
    for j in range(n_objects):
        for k in range(len(o)):
            hit[j, k], t[j, k] = intercepts_fn(j, o[k], d[k])[:2]
    return hit, t


def brute_force(tests, t_max):
    """any(hit_j and t_j < t_max) over the objects, from per_object's arrays; the comparison is float32's (a NaN t, a NaN limit:
    not in front)"""
    hit, t = tests
    with np.errstate(invalid="ignore"):
        return (hit & (t < np.asarray(t_max, np.float32)[None, :])).any(0)


def nearest(tests):
    """The smallest t among per_object's hits -> (float32 t, has a hit); NaN t's take no part"""
    hit, t = tests
    with np.errstate(invalid="ignore"):
        th = np.where(hit & ~np.isnan(t), t, np.float32(np.inf)).min(0) if len(t) else np.full(hit.shape[1], np.inf, np.float32)
    return th.astype(np.float32), np.isfinite(th)


def tie_limits(t):
    """For hits at the float32 distances t: (t itself - a miss, the comparison is strict; its upper neighbour - a hit; its
    lower neighbour - a miss)"""
    t = np.asarray(t, np.float32)
    return t.copy(), np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))


def check_segment(objects, o, d, t_max, got, what):
    """An implementation's answers against the model on well-conditioned rays, under the 5 % cap -> cases left out"""
    occ, margin = occluded_within(objects, o, d, t_max)
    ok, left = ref.well_conditioned(margin, what)
    wrong = ok & (np.asarray(got, bool) != occ)
    print("%s: %d rays, %d occluded, %d left out" % (what, len(ok), int((ok & occ).sum()), left))
    assert not wrong.any(), "%s: %d rays differ from the model's, first at ray %d (margin %g)" % (
        what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]), float(margin[wrong][0]))
    assert 0 < (ok & occ).sum() < ok.sum(), what + ": the rays are all occluded or all free"
    return left
