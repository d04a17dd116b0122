"""A float64 model of the nearest-surface query (p3d_host_scene_nearest, p3d_nearest_device, include/p3d.h), stated
differently from the rule of host/nearest_rule.hpp so that a mistake shared by the host form and the kernel cannot hide
behind their bit parity:

  triangle  the minimum over five candidates: the foot of p on the triangle's plane where the three edge functions say it lies
            inside, and the closest points of the three edge segments (the vertices fall out of the segments) - no Voronoi
            regions, no barycentric quotients
  sphere    | |p - c| - r |
  box       the minimum over the six face rectangles (p clamped to the rectangle) - no inside / outside cases
  plane     |(p - A).N|

Only DISTANCES are modelled.  Distance is continuous in p, so the checks need no conditioning margin: a tie on a shared edge
may name either triangle, and is held to "the reported object is as near as the nearest", and the reported closest point is
held to lie on the reported object at the reported distance.  The found / not-found decision under a limit is discontinuous at
d = limit; the limits are drawn away from that (draw_limits), and a decision within THRESHOLD of it may be left out.

The objects are read from the .p3f file by intersect_reference.load_objects."""
import numpy as np

import intersect_reference as ref

SPHERE, TRIANGLE, BOX, PLANE = ref.SPHERE, ref.TRIANGLE, ref.BOX, ref.PLANE
THRESHOLD = ref.THRESHOLD
MAX_LEFT_OUT = ref.MAX_LEFT_OUT
FACTORS = (0.5, 0.9, 1.1, 2.0, np.inf)  # segment_reference.FACTORS: of the model's distance; never within 10 % of it
FLOOR = 1e-3            # a point nearer than this to a surface (the on-surface quarter) gets a limit of 10 x FLOOR or inf instead
N_POINTS = 2000
FLT_MAX = np.finfo(np.float32).max

# Measured: the largest error over the fixed point sets of test_nearest_reference.py (HostScene.nearest on the CPU; the GPU
# must equal its bits, so on these inputs its error is the host form's), as intersect_reference.rel_err counts it:
# |got - want| / max(1, |want|).  The asserted tolerance is 4 x the measured maximum: room for another seed or scene, not
# for another implementation.
MEASURED = {
    "dist": 1.52e-6,        # (a) dist against the model's minimum (worst: mixed_planes)
    "object": 0.0,          # (b) the model's distance to the reported object against that minimum: on these sets every
                            #     reported object IS the model's nearest, or ties with it exactly (a shared vertex: 0 and 0)
    "on_surface": 1.52e-6,  # (c) the model's distance from the reported closest point to the reported object, against 0
    "closest": 1.31e-7,     # (c) |p - closest| against dist
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}


# ---- the model ------------------------------------------------------------------------------------------------------------------

def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _segment(a, b, p):
    """distance from the points p (n, 3) to the segments a b ((m, 3) each) -> (m, n)"""
    ab = (b - a)[:, None, :]
    ap = p[None, :, :] - a[:, None, :]
    with np.errstate(all="ignore"):
        s = np.clip((ap * ab).sum(-1) / (ab * ab).sum(-1), 0.0, 1.0)
    s = np.nan_to_num(s)  # a = b: the point a
    return _norm(ap - s[..., None] * ab)


def triangles(p0, p1, p2, p):
    """(m, 3) vertices x (n, 3) points -> (m, n) distances"""
    n = np.cross(p1 - p0, p2 - p0)
    nn = (n * n).sum(-1)
    w = p[None, :, :] - p0[:, None, :]
    with np.errstate(all="ignore"):
        h = (w * n[:, None, :]).sum(-1) / nn[:, None]   # p = foot + h n
    foot = p[None, :, :] - h[..., None] * n[:, None, :]
    inside = np.ones(h.shape, bool)
    for a, b in ((p0, p1), (p1, p2), (p2, p0)):
        e = np.cross((b - a)[:, None, :], foot - a[:, None, :])
        inside &= (e * n[:, None, :]).sum(-1) >= 0
    face = np.where(inside, np.abs(h) * np.sqrt(nn)[:, None], np.inf)
    return np.minimum(np.minimum(face, _segment(p0, p1, p)), np.minimum(_segment(p1, p2, p), _segment(p2, p0, p)))


def distance(ob, p):
    """one object x (n, 3) points -> (n,) distances to its surface"""
    p = np.atleast_2d(np.asarray(p, np.float64))
    k = ob["kind"]
    if k == TRIANGLE:
        return triangles(ob["p0"][None], ob["p1"][None], ob["p2"][None], p)[0]
    if k == SPHERE:
        return np.abs(_norm(p - ob["c"]) - ob["r"])
    if k == PLANE:
        return np.abs((p - ob["p0"]) @ ref.unit_normal(ob))
    mn, mx = ob["mn"], ob["mx"]
    best = np.full(len(p), np.inf)
    for axis in range(3):
        for face in (mn[axis], mx[axis]):
            q = np.clip(p, mn, mx)
            q[:, axis] = face
            best = np.minimum(best, _norm(p - q))
    return best


def table(objects, p, chunk=256):
    """(objects, points) distances; the triangles in chunks"""
    p = np.atleast_2d(np.asarray(p, np.float64))
    out = np.empty((len(objects), len(p)))
    tri = [j for j, ob in enumerate(objects) if ob["kind"] == TRIANGLE]
    for s in range(0, len(tri), chunk):
        js = tri[s:s + chunk]
        out[js] = triangles(*(np.stack([objects[j][key] for j in js]) for key in ("p0", "p1", "p2")), p)
    for j, ob in enumerate(objects):
        if ob["kind"] != TRIANGLE:
            out[j] = distance(ob, p)
    return out


# ---- the fixed inputs (shared by the CPU and the GPU suite) -----------------------------------------------------------------------

def surface_point(ob, rng):
    """A random point on the object, float64"""
    k = ob["kind"]
    if k == SPHERE:
        return ob["c"] + ob["r"] * ref._unit(rng, 1)[0]
    if k == BOX:
        q = rng.uniform(ob["mn"], ob["mx"])
        axis = rng.integers(0, 3)
        q[axis] = (ob["mn"], ob["mx"])[rng.integers(0, 2)][axis]
        return q
    u, v = rng.uniform(0, 1, 2)
    if k == TRIANGLE and u + v > 1:
        u, v = 1 - u, 1 - v
    if k == PLANE:
        u, v = 4 * u - 2, 4 * v - 2
    return ob["p0"] + u * (ob["p1"] - ob["p0"]) + v * (ob["p2"] - ob["p0"])


def special_point(ob, rng):
    """Exactly on the object, or where its rule has a case of its own: a vertex, a centre, a corner, an edge's middle"""
    k = ob["kind"]
    pick = rng.integers(0, 3)
    if k == SPHERE:
        return ob["c"] if pick == 0 else surface_point(ob, rng)
    if k == BOX:
        if pick == 0:
            return (ob["mn"] + ob["mx"]) / 2
        if pick == 1:
            return np.where(rng.integers(0, 2, 3) == 1, ob["mx"], ob["mn"])
        return surface_point(ob, rng)
    if k == TRIANGLE:
        if pick == 0:
            return ob[("p0", "p1", "p2")[rng.integers(0, 3)]]
        if pick == 1:
            a, b = (("p0", "p1"), ("p1", "p2"), ("p2", "p0"))[rng.integers(0, 3)]
            return (ob[a] + ob[b]) / 2
    return surface_point(ob, rng)


def scene_bounds(objects):
    balls = [ref.bounding_sphere(ob) for ob in objects]
    lo = np.min([c - r for c, r in balls], axis=0)
    hi = np.max([c + r for c, r in balls], axis=0)
    return lo, hi


def scene_points(objects, seed, n=N_POINTS):
    """n float32 points, shuffled so that every prefix holds all three sorts: half uniform in the scene's bounds inflated by
    50 %; a quarter at small random offsets (up to 2 % of the diagonal, log-uniform from 1e-5 of it) from random surface
    points; a quarter exactly on surfaces, centres, box centres, corners and vertices"""
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(objects)
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    diag = float(np.linalg.norm(hi - lo))
    n_far, n_near = n // 2, n // 4
    far = mid + 1.5 * half * rng.uniform(-1, 1, (n_far, 3))
    near = np.stack([surface_point(objects[j], rng) for j in rng.integers(0, len(objects), n_near)])
    near = near + ref._unit(rng, n_near) * (diag * np.exp(rng.uniform(np.log(1e-5), np.log(2e-2), n_near)))[:, None]
    on = np.stack([special_point(objects[j], rng) for j in rng.integers(0, len(objects), n - n_far - n_near)])
    pts = np.concatenate([far, near, on]).astype(np.float32)
    return np.ascontiguousarray(pts[rng.permutation(n)])


def draw_limits(d_min, seed):
    """One float32 limit per point: the model's distance times a factor from FACTORS (a point within FLOOR of a surface: 10 x
    FLOOR or inf), then every 25th a zero, a negative number or a NaN in turn"""
    rng = np.random.default_rng(seed)
    factor = np.array(FACTORS)[rng.integers(0, len(FACTORS), len(d_min))]
    with np.errstate(invalid="ignore"):
        lim = np.where(d_min < FLOOR, np.where(np.isfinite(factor) & (factor < 1.5), 10 * FLOOR, np.inf), d_min * factor)
    lim = lim.astype(np.float32)
    lim[0::75], lim[25::75], lim[50::75] = 0.0, -1.5, np.nan
    return lim


def decide(d_min, limits):
    """The model's decision under float32 limits -> (found, margin): margin = |d - limit| / limit for a positive finite limit,
    inf where the limit itself decides (zero, negative, NaN, inf)"""
    lim = np.asarray(limits, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        found = (lim > 0) & (d_min < lim)
        margin = np.where((lim > 0) & np.isfinite(lim), np.abs(d_min - lim) / lim, np.inf)
    return found, margin


# ---- the assertions, the same for HostScene.nearest (CPU suite) and wherever else the model is asked ----------------------------

def check_nearest(objects, p, got, what, tab=None):
    """got = (object, dist, closest) without a limit -> the four measured errors"""
    obj, dist, closest = got
    tab = table(objects, p) if tab is None else tab
    n = len(p)
    assert (obj >= 0).all() and (obj < len(objects)).all(), what + ": a point without an answer"
    d_min = tab.min(0)
    p64 = np.asarray(p, np.float64)
    err = {
        "dist": float(ref.rel_err(dist, d_min).max()),
        "object": float(ref.rel_err(tab[obj, np.arange(n)], d_min).max()),
        "closest": float(ref.rel_err(_norm(p64 - closest), dist).max()),
    }
    on = np.zeros(n)
    for j in np.unique(obj):
        m = obj == j
        on[m] = distance(objects[j], closest[m])
    err["on_surface"] = float(on.max())
    print("%s: %d points, errors %s (tolerances %s)" % (what, n, {k: "%.3g" % v for k, v in err.items()}, {k: "%.3g" % v for k, v in TOL.items()}))
    for k, v in err.items():
        assert v <= TOL[k], "%s: %s is off by %g, tolerance %g" % (what, k, v, TOL[k])
    return err


def check_limited(objects, p, limits, got, free, what, tab=None):
    """got under `limits` against the model's decision; where found, the answer is the unlimited one (`free`) -> left out"""
    obj, dist, closest = got
    tab = table(objects, p) if tab is None else tab
    found, margin = decide(tab.min(0), limits)
    ok = margin >= THRESHOLD
    left = int((~ok).sum())
    assert left <= MAX_LEFT_OUT * len(ok), "%s: %d of %d decisions lie at the limit, over the %g cap" % (what, left, len(ok), MAX_LEFT_OUT)
    wrong = ok & ((obj >= 0) != found)
    print("%s: %d points, %d found, %d left out" % (what, len(ok), int((ok & found).sum()), left))
    assert not wrong.any(), "%s: %d decisions differ from the model's, first at point %d (margin %g)" % (
        what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]), float(margin[wrong][0]))
    assert 0 < (ok & found).sum() < ok.sum(), what + ": the points are all found or all not"
    hit = obj >= 0
    assert (obj[hit] == free[0][hit]).all() and (dist[hit] == free[1][hit]).all() and (closest[hit] == free[2][hit]).all(), what + ": a limit changed an answer"
    assert (dist[~hit] == FLT_MAX).all() and not closest[~hit].any() and not np.signbit(closest[~hit]).any(), what + ": the no-answer values"
    return left
