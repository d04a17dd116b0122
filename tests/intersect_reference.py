"""A float64 model of the geometric core (intercepts, get_normal, closest hit, any hit), stated geometrically and not in the
reference's formulas, so that an error shared by the kernel and the CPU oracle cannot hide behind their bit parity.

  sphere    the foot of the centre on the ray's line and the half chord: hits at s -+ k for the unit direction; an origin
            outside takes the near one, inside the far one; a sphere behind the ray is a miss.  t in units of d/|d|.
  triangle  the plane by N = (P1-P0) x (P2-P0), then barycentrics of the plane point by edge functions; a hit when
            beta >= 0, gamma >= 0, beta + gamma <= 1 and t >= 1e-4.  t in units of d as given.  Both faces are hit.
  box       per-axis slab intervals, a zero direction component handled by itself (inside the slab: the whole line, else
            nothing); a hit when t0 < t1 and t1 > 1e-4; t = t0, or t1 when t0 < 0.
  plane     t = -((o-A).N)/(N.d); a miss when |N.d| <= 1e-4 or t <= 0.
  normals   sphere (p-c)/|p-c|; triangle and plane their unit normal; box the signed axis of the largest |p - centre|
            component in the reference's tie order (scene.cpp:229-267: x beats y on a strict >, z beats the winner on a
            strict >, a zero component counts as positive).  That is the face normal only for a cube: a flat box answers
            with the axis of its long side, in the reference as here.

Every routine also returns a conditioning MARGIN: how far the case is from flipping a decision, in the relative units given
at each routine.  A case whose margin is under THRESHOLD is ill-conditioned and is left out of a comparison with this model
(the GPU-against-oracle comparisons cover it bit for bit); the tests cap the share left out at MAX_LEFT_OUT.

Deliberately NOT pinned here:
  Q8   a sphere test normalises the traversal's ray in place, so with an unnormalised direction the reference compares t's in
       mixed units.  closest() and occluded() are stated for unit directions (normalised in float32) only.
  Q12  a plane's bounding box is [-1,1]^3, so the grid and the BVH lose planes; scenes with planes go through accel None only.
  BVH any-hit (bvh.cpp:329-334: the pop loop empties the stack and resumes at the bottom entry) depends on the tree's shape: a
       ray can be reported unoccluded although an object is hit.  No margin of this model says when, so occluded() is compared
       with the brute-force and grid back ends only and the BVH's any-hit stays with the oracle parity.
  NaN  payloads, and everything about a ray with a NaN in it: such cases get margin 0.

The objects are read from the .p3f file by load_objects below, not taken from the oracle or the library."""
import numpy as np

SPHERE, TRIANGLE, BOX, PLANE = 0, 1, 2, 3  # P3D_PRIM_* (include/p3d.h) = the oracle's kinds
KINDS = {SPHERE: "sphere", TRIANGLE: "triangle", BOX: "box", PLANE: "plane"}
T_MIN = 1e-4
THRESHOLD = 1e-3     # margins under it: ill-conditioned
MAX_LEFT_OUT = 0.05  # the share of a test's cases that may be ill-conditioned

# Measured: the largest |oracle - model| / max(1, |model|) over the well-conditioned cases of the fixed input sets of
# test_intersect_reference.py (CPU oracle; the GPU must equal its bits, so on these inputs its error is the oracle's).
# The asserted tolerance is 4 x the measured maximum: room for another seed or scene, not for another implementation.
MEASURED = {
    "t_sphere": 3.1e-6, "t_triangle": 4.4e-7, "t_box": 1.5e-7, "t_plane": 3.0e-5,   # Object::intercepts, 2 000 rays per kind
    "normal_sphere": 1.2e-7,                                                          # per component
    "t_closest_none": 1.5e-5, "t_closest_grid": 3.6e-6, "t_closest_bvh": 3.6e-6,      # 2 000 rays per scene; planes only under none
    "p_closest_none": 1.9e-5, "p_closest_grid": 8.0e-6, "p_closest_bvh": 8.0e-6,      # the hit point, per component
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
ULP = float(np.finfo(np.float32).eps)  # the spacing of float32 at 1: the unit of "n ulp" for components of unit vectors
NORMAL_ULPS = 4                        # triangle and plane normals, per component
UNIT_ULPS = 2                          # |direction out of a sphere test| - 1


# ---- scenes ---------------------------------------------------------------------------------------------------------------------

def load_objects(path):
    """The objects of a .p3f file in file order (`s`, `p 3`, `box`, `pl` lines) -> list of dicts of float64 arrays holding the
    float32 values a loader reads."""
    with open(path) as f:
        tok = [w for line in f for w in line.split("#")[0].split()]
    f32 = lambda ws: np.array([np.float32(w) for w in ws], np.float32).astype(np.float64)
    args = {"bclr": 3, "from": 3, "at": 3, "up": 3, "angle": 1, "hither": 1, "resolution": 2, "aperture": 1, "focal": 1,
            "l": 6, "f": 14, "v": 0}
    out, i = [], 0
    while i < len(tok):
        w = tok[i]
        i += 1
        if w == "s":
            v = f32(tok[i:i + 4]); i += 4
            out.append(dict(kind=SPHERE, c=v[:3], r=v[3]))
        elif w == "p":
            assert tok[i] == "3", "only triangles"
            v = f32(tok[i + 1:i + 10]); i += 10
            out.append(dict(kind=TRIANGLE, p0=v[0:3], p1=v[3:6], p2=v[6:9]))
        elif w == "box":
            v = f32(tok[i:i + 6]); i += 6
            out.append(dict(kind=BOX, mn=v[:3], mx=v[3:]))
        elif w == "pl":
            v = f32(tok[i:i + 9]); i += 9
            out.append(dict(kind=PLANE, p0=v[0:3], p1=v[3:6], p2=v[6:9]))
        else:
            i += args[w]
    return out


def unit_normal(ob):
    """Triangle: (P1-P0) x (P2-P0); plane: (P2-P1) x (P0-P1) (scene.cpp:102-113 fixes the side); unit length."""
    n = np.cross(ob["p1"] - ob["p0"], ob["p2"] - ob["p0"]) if ob["kind"] == TRIANGLE else np.cross(ob["p2"] - ob["p1"], ob["p0"] - ob["p1"])
    return n / np.sqrt(n @ n)


def bounding_sphere(ob):
    """(centre, radius); a plane gets a ball of radius 2 about its anchor point."""
    k = ob["kind"]
    if k == SPHERE:
        return ob["c"], float(ob["r"])
    if k == BOX:
        return (ob["mn"] + ob["mx"]) / 2, float(np.linalg.norm(ob["mx"] - ob["mn"]) / 2)
    if k == PLANE:
        return ob["p0"], 2.0
    c = (ob["p0"] + ob["p1"] + ob["p2"]) / 3
    return c, float(max(np.linalg.norm(ob[p] - c) for p in ("p0", "p1", "p2")))


# ---- the four tests -------------------------------------------------------------------------------------------------------------
# Each takes (n, 3) origins and directions and returns (hit, t, margin, t_cand): t is NaN on a miss; t_cand is where the hit
# would be if an ill-conditioned decision fell the other way (0 where that cannot be said), for closest().

def _rows(a):
    return np.atleast_2d(np.asarray(a, np.float64))


def _dot(a, b):
    return (a * b).sum(-1)


def _finish(hit, t, margin, t_cand):
    margin = np.where(np.isnan(margin), 0.0, margin)
    return hit & ~np.isnan(t), np.where(hit, t, np.nan), margin, np.where(np.isfinite(t_cand), t_cand, 0.0)


def sphere(ob, o, d):
    """Margins: |r^2 - p^2| over s^2 + ||m|^2 - r^2| (the discriminant against b^2 + |c|: a tangent ray) where the foot is
    ahead or the origin inside, and ||m|^2 - r^2| over r^2 (the origin on the surface)."""
    o, d = _rows(o), _rows(d)
    c, r = ob["c"], ob["r"]
    with np.errstate(all="ignore"):
        dh = d / np.sqrt(_dot(d, d))[:, None]
        m = c - o
        s = _dot(m, dh)                      # the foot of the centre on the line
        perp = m - s[:, None] * dh
        p2 = _dot(perp, perp)                # its squared distance from the centre
        q = _dot(m, m) - r * r               # > 0: the origin is outside
        k = np.sqrt(np.maximum(r * r - p2, 0.0))
        outside = q > 0
        reaches = r * r - p2 >= 0
        hit = np.where(outside, reaches & (s >= 0), True)
        t = np.where(outside, s - k, s + k)
        tangent = np.abs(r * r - p2) / (s * s + np.abs(q))
        behind = outside & (s < 0)           # (s near 0 from outside: the line misses by |m| > r, a miss either way)
        margin = np.minimum(np.where(behind, np.inf, tangent), np.abs(q) / (r * r))
        on_surface = np.abs(q) / (r * r) < THRESHOLD
    return _finish(hit, t, margin, np.where(on_surface, 0.0, t))


def triangle(ob, o, d):
    """Margins: the smallest of beta, gamma, 1 - beta - gamma and t - 1e-4 (the hit is where all four are >= 0, so their minimum
    decides), and |N.d| over |e1| |e2| |d| (a ray in the plane, or a sliver)."""
    o, d = _rows(o), _rows(d)
    p0 = ob["p0"]
    e1, e2 = ob["p1"] - p0, ob["p2"] - p0
    n = np.cross(e1, e2)
    with np.errstate(all="ignore"):
        nd = _dot(d, n)
        t = _dot(p0 - o, n) / nd
        w = o + t[:, None] * d - p0          # the plane point, from P0: w = beta e1 + gamma e2
        beta = _dot(np.cross(w, e2), n) / (n @ n)
        gamma = _dot(np.cross(e1, w), n) / (n @ n)
        decides = np.minimum(np.minimum(beta, gamma), np.minimum(1 - beta - gamma, t - T_MIN))
        hit = (beta >= 0) & (gamma >= 0) & (beta + gamma <= 1) & (t >= T_MIN)
        flat = np.abs(nd) / (np.sqrt((e1 @ e1) * (e2 @ e2)) * np.sqrt(_dot(d, d)))
        margin = np.minimum(np.abs(decides), flat)
    return _finish(hit, t, margin, np.where(flat < THRESHOLD, 0.0, t))


def box(ob, o, d):
    """Margins, in units of the box's diagonal (t times |d| is a length): the smaller of t1 - t0 and t1 - 1e-4 (a hit is where
    both are > 0); on a hit also |t0| (the origin on a face: t jumps from t0 to t1); for a zero direction component the
    origin's distance to that slab's faces."""
    o, d = _rows(o), _rows(d)
    mn, mx = ob["mn"], ob["mx"]
    size = np.sqrt((mx - mn) @ (mx - mn))
    n = len(o)
    t0, t1 = np.full(n, -np.inf), np.full(n, np.inf)
    edge = np.full(n, np.inf)
    with np.errstate(all="ignore"):
        for k in range(3):
            z = d[:, k] == 0
            dk = np.where(z, 1.0, d[:, k])
            a, b = (mn[k] - o[:, k]) / dk, (mx[k] - o[:, k]) / dk
            inside = (o[:, k] > mn[k]) & (o[:, k] < mx[k])
            lo = np.where(z, np.where(inside, -np.inf, np.inf), np.minimum(a, b))
            hi = np.where(z, np.where(inside, np.inf, -np.inf), np.maximum(a, b))
            t0, t1 = np.maximum(t0, lo), np.minimum(t1, hi)
            edge = np.where(z, np.minimum(edge, np.minimum(np.abs(o[:, k] - mn[k]), np.abs(o[:, k] - mx[k])) / size), edge)
        hit = (t0 < t1) & (t1 > T_MIN)
        t = np.where(t0 < 0, t1, t0)
        scale = np.sqrt(_dot(d, d)) / size
        decides = np.minimum(t1 - t0, t1 - T_MIN)
        margin = np.minimum(np.abs(decides) * scale, edge)
        margin = np.where(hit, np.minimum(margin, np.abs(t0) * scale), margin)
    return _finish(hit, t, margin, np.maximum(t0, 0.0))


def plane(ob, o, d):
    """Margins: the smaller of |N.d| - 1e-4 and t (a hit is where both are > 0), as they are."""
    o, d = _rows(o), _rows(d)
    n = unit_normal(ob)
    with np.errstate(all="ignore"):
        nd = _dot(d, n)
        t = -_dot(o - ob["p0"], n) / nd
        hit = (np.abs(nd) > T_MIN) & (t > 0)
        margin = np.abs(np.minimum(np.abs(nd) - T_MIN, t))
    return _finish(hit, t, margin, np.zeros(len(o)))


_TESTS = {SPHERE: sphere, TRIANGLE: triangle, BOX: box, PLANE: plane}


def intercepts(ob, o, d):
    """-> (hit, t, margin) for (n, 3) rays against one object"""
    return _TESTS[ob["kind"]](ob, o, d)[:3]


def normal(ob, p):
    """-> (normal (n, 3), margin) at the points p.  Box margin: the gap between the two largest |p - centre| components over the
    box's diagonal; a sphere's: |p - c| over r (the centre has no normal); the others have none to lose."""
    p = _rows(p)
    k = ob["kind"]
    if k in (TRIANGLE, PLANE):
        return np.broadcast_to(unit_normal(ob), p.shape).copy(), np.full(len(p), np.inf)
    if k == SPHERE:
        v = p - ob["c"]
        ln = np.sqrt(_dot(v, v))
        with np.errstate(all="ignore"):
            return v / ln[:, None], np.nan_to_num(ln / ob["r"], nan=0.0)
    co = p - (ob["mn"] + ob["mx"]) / 2
    a = np.abs(co)
    axis = np.where(a[:, 0] > a[:, 1], 0, 1)
    axis = np.where(a[:, 2] > a[np.arange(len(p)), axis], 2, axis)
    out = np.zeros_like(p)
    pick = co[np.arange(len(p)), axis]
    out[np.arange(len(p)), axis] = np.where(pick >= 0, 1.0, -1.0)
    srt = np.sort(a, axis=1)
    margin = (srt[:, 2] - srt[:, 1]) / np.sqrt((ob["mx"] - ob["mn"]) @ (ob["mx"] - ob["mn"]))
    return out, np.nan_to_num(margin, nan=0.0)


# ---- all objects ----------------------------------------------------------------------------------------------------------------

def _all(objects, o, d):
    o, d = _rows(o), _rows(d)
    ln = np.sqrt(_dot(d, d))
    res = [_TESTS[ob["kind"]](ob, o, d) for ob in objects]
    # t and t_cand in units of the unit direction (the sphere's already are)
    unit = [1.0 if ob["kind"] == SPHERE else ln for ob in objects]
    hit = np.stack([r[0] for r in res])
    t = np.stack([r[1] * u for r, u in zip(res, unit)])
    margin = np.stack([r[2] for r in res])
    cand = np.stack([r[3] * u for r, u in zip(res, unit)])
    return hit, t, margin, cand


def closest(objects, o, d):
    """The nearest hit over all objects, by brute force, for unit directions -> (index or -1, t, gap, margin).  gap: the
    second-nearest t minus the nearest (inf with fewer than two hits).  margin: the smaller of gap / max(1, t) and the margins
    of every object whose decision matters: the nearest itself, and an ill-conditioned one whose t_cand is not clearly behind
    the nearest hit (with no hit at all, every one)."""
    hit, t, margin, cand = _all(objects, o, d)
    n = hit.shape[1]
    with np.errstate(invalid="ignore"):
        th = np.where(hit, t, np.inf)
        idx = th.argmin(0)
        t_near = th[idx, np.arange(n)]
        none = ~np.isfinite(t_near)
        th2 = th.copy()
        th2[idx, np.arange(n)] = np.inf
        gap = th2.min(0) - t_near
        gap = np.where(none, np.inf, gap)
        slack = THRESHOLD * np.maximum(1.0, np.where(none, 1.0, t_near))
        matters = none[None, :] | (np.where(hit, t, cand) <= (t_near + slack)[None, :])
        m = np.where(matters, margin, np.inf).min(0)
        m = np.minimum(m, np.where(none, np.inf, gap / np.maximum(1.0, np.abs(t_near))))
    return np.where(none, -1, idx), np.where(none, np.nan, t_near), gap, m


def occluded(objects, o, d):
    """Any hit (the brute-force and grid back ends) -> (occluded, margin): the best margin among the hits of an occluded ray,
    the worst of all objects for a free one."""
    hit, _, margin, _ = _all(objects, o, d)
    occ = hit.any(0)
    return occ, np.where(occ, np.where(hit, margin, -np.inf).max(0), margin.min(0))


# ---- the fixed input sets (shared by the CPU and the GPU suite) -----------------------------------------------------------------

def normalize32(v):
    """v / |v|, every step one float32 operation"""
    v = np.asarray(v, np.float32)
    ln = np.sqrt((v * v).sum(-1, dtype=np.float32), dtype=np.float32)
    return (v / ln[..., None]).astype(np.float32)


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _in_ball(rng, n):
    return _unit(rng, n) * np.cbrt(rng.uniform(0, 1, n))[:, None]


def object_rays(ob, seed, n=500):
    """n rays for one object -> (origins, directions) float32.  Half are aimed at a point drawn uniformly in the object's
    bounding sphere from an origin outside it; the other half have random origins (a third of them inside the bounding sphere,
    so inside a sphere or a box) and random directions.  Directions are normalised in float32; for the kinds that use the
    direction as given, the last quarter of each half is then scaled by 0.2 to 5."""
    rng = np.random.default_rng(seed)
    c, r = bounding_sphere(ob)
    h = n // 2
    o_a = (c + r * _unit(rng, h) * rng.uniform(1.5, 6.0, h)[:, None]).astype(np.float32)
    d_a = normalize32((c + r * _in_ball(rng, h)).astype(np.float32) - o_a)
    o_b = rng.uniform(-3, 3, (n - h, 3))
    third = (n - h) // 3
    o_b[:third] = c + 0.9 * r * _in_ball(rng, third)
    o_b = o_b.astype(np.float32)
    d_b = normalize32(_unit(rng, n - h))
    if ob["kind"] != SPHERE:
        for d in (d_a, d_b):
            q = len(d) // 4
            d[-q:] *= np.exp(rng.uniform(np.log(0.2), np.log(5.0), q)).astype(np.float32)[:, None]
    return np.concatenate([o_a, o_b]), np.concatenate([d_a, d_b])


def box_points(ob, seed, n=500):
    """Random points in and around a box (1.5 times its extent about its centre) -> float32"""
    rng = np.random.default_rng(seed)
    c, half = (ob["mn"] + ob["mx"]) / 2, (ob["mx"] - ob["mn"]) / 2
    return (c + 1.5 * half * rng.uniform(-1, 1, (n, 3))).astype(np.float32)


def scene_rays(objects, seed, n=2000):
    """n rays with unit directions (normalised in float32) for a whole scene: three quarters aimed at a point drawn in one
    object's bounding sphere from an origin 1.5 to 4 radii from its centre, the rest from origins among the objects in random
    directions.  The rays are short on purpose: a sphere's tangent margin is relative to the squared distance, so from far
    away a wide ring around every small sphere is ill-conditioned."""
    rng = np.random.default_rng(seed)
    h = 3 * n // 4
    balls = [bounding_sphere(ob) for ob in objects]
    pick = rng.integers(0, len(objects), h)
    c = np.stack([balls[i][0] for i in pick])
    r = np.array([balls[i][1] for i in pick])
    target = c + r[:, None] * _in_ball(rng, h)
    o_a = (c + r[:, None] * _unit(rng, h) * rng.uniform(1.5, 4.0, h)[:, None]).astype(np.float32)
    d_a = normalize32(target.astype(np.float32) - o_a)
    o_b = rng.uniform(-1.5, 1.5, (n - h, 3)).astype(np.float32)
    d_b = normalize32(_unit(rng, n - h))
    return np.concatenate([o_a, o_b]), np.concatenate([d_a, d_b])


# ---- comparing an implementation with the model ---------------------------------------------------------------------------------

def rel_err(got, want):
    """|got - want| / max(1, |want|), elementwise"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.maximum(1.0, np.abs(want))


def well_conditioned(margin, what):
    """The mask of the cases to compare; asserts the 5 % cap on the rest."""
    ok = margin >= THRESHOLD
    left = int((~ok).sum())
    assert left <= MAX_LEFT_OUT * len(ok), "%s: %d of %d cases are ill-conditioned, over the %g cap" % (what, left, len(ok), MAX_LEFT_OUT)
    return ok, left


def scene_paths(tmp):
    """name -> .p3f path of the scenes both suites use: two random ones written under `tmp` (a few dozen objects; planes only
    in the second) and the two authored scenes with planes and with axis-aligned faces."""
    import os
    import fuzz_scenes
    scenes = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scenes")
    return dict(mixed=fuzz_scenes.random_scene(71, os.path.join(str(tmp), "mixed.p3f"), n_spheres=8, n_tris=10, n_boxes=6, n_planes=0),
                mixed_planes=fuzz_scenes.random_scene(72, os.path.join(str(tmp), "mixed_planes.p3f"), n_spheres=6, n_tris=8, n_boxes=4,
                                                      n_planes=2),
                planes=os.path.join(scenes, "planes.p3f"), axis_aligned=os.path.join(scenes, "axis_aligned.p3f"))


NO_PLANES = ("mixed", "axis_aligned")  # every back end; the other two scenes go through accel None only (Q12)
RAYS_PER_OBJECT = 500


def kind_cases(objects, kind, count=4):
    """[(scene, object index)]: the first `count` objects of a kind over mixed_planes, planes, axis_aligned, mixed"""
    found = [(name, i) for name in ("mixed_planes", "planes", "axis_aligned", "mixed") for i, ob in enumerate(objects[name])
             if ob["kind"] == kind]
    per_scene = {}
    for name, i in found:  # at most two of one scene, so that the authored scenes take part
        per_scene.setdefault(name, []).append((name, i))
    out = [c for cs in per_scene.values() for c in cs[:2]]
    return out[:count]


def case_seed(scene, i):
    return 1000 * ("mixed_planes", "planes", "axis_aligned", "mixed").index(scene) + i


# ---- the assertions, the same for the oracle (CPU suite) and the kernels (GPU suite) --------------------------------------------
# Each returns what it measured, and prints it.

def check_intercepts(ob, o, d, got_hit, got_t, got_d, what):
    """Object::intercepts for one object: on well-conditioned rays the decision is the model's and t within TOL; the direction
    comes back as the input bits (a sphere: unit length within UNIT_ULPS).  -> (largest relative t error, cases left out)"""
    hit, t, margin = intercepts(ob, o, d)
    ok, left = well_conditioned(margin, what)
    got_hit = np.asarray(got_hit, bool)
    wrong = ok & (got_hit != hit)
    assert not wrong.any(), "%s: %d decisions differ from the model's, first at ray %d (margin %g)" % (
        what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]), float(margin[wrong][0]))
    both = ok & hit
    err = float(rel_err(np.asarray(got_t)[both], t[both]).max()) if both.any() else 0.0
    key = "t_" + KINDS[ob["kind"]]
    print("%s: %d rays, %d hits, %d left out, max relative t error %.3g (tolerance %.3g)" % (what, len(ok), int(both.sum()), left, err, TOL[key]))
    assert err <= TOL[key], "%s: t is off by %g relative, tolerance %g" % (what, err, TOL[key])
    got_d = np.asarray(got_d, np.float32)
    if ob["kind"] == SPHERE:
        fin = np.isfinite(got_d).all(-1)
        ln = np.sqrt((got_d[fin].astype(np.float64) ** 2).sum(-1))
        assert np.abs(ln - 1).max() <= UNIT_ULPS * ULP, "%s: a direction left with length 1 %+g" % (what, float(np.abs(ln - 1).max()))
        d64 = _rows(d)[fin]
        turned = np.abs(got_d[fin] - d64 / np.sqrt(_dot(d64, d64))[:, None]).max()
        assert turned <= UNIT_ULPS * ULP, "%s: a direction left %g away from d/|d|" % (what, float(turned))
    else:
        assert (got_d.view(np.uint32) == np.asarray(d, np.float32).view(np.uint32)).all(), what + ": the direction was touched"
    return err, left


def surface_points(ob, o, d):
    """float32 points on the object: the model's well-conditioned hits"""
    hit, t, margin = intercepts(ob, o, d)
    o, d = _rows(o), _rows(d)
    if ob["kind"] == SPHERE:
        d = d / np.sqrt(_dot(d, d))[:, None]
    m = hit & (margin >= THRESHOLD)
    return (o[m] + t[m, None] * d[m]).astype(np.float32)


def check_normals(ob, p, got, what):
    """Object::getNormal: a box's equals the model's on well-conditioned points; a sphere's is within TOL, a triangle's and a
    plane's within NORMAL_ULPS per component.  -> (largest component error, cases left out)"""
    want, margin = normal(ob, p)
    ok, left = well_conditioned(margin, what)
    err = float(np.abs(np.asarray(got, np.float64) - want)[ok].max()) if ok.any() else 0.0
    tol = {SPHERE: TOL["normal_sphere"], BOX: 0.0}.get(ob["kind"], NORMAL_ULPS * ULP)
    print("%s: %d points, %d left out, max normal error %.3g (tolerance %.3g)" % (what, len(ok), left, err, tol))
    assert err <= tol, "%s: a normal is off by %g, tolerance %g" % (what, err, tol)
    return err, left


def check_closest(objects, o, d, got_id, got_t, got_p, accel_name, what):
    """Closest hits: the hit id is the model's nearest object wherever the case is well-conditioned (the gap to the second
    nearest included); t and the hit point are within TOL.  -> (t error, point error, cases left out)"""
    idx, t, _, margin = closest(objects, o, d)
    ok, left = well_conditioned(margin, what)
    got_id = np.asarray(got_id)
    wrong = ok & (got_id != idx)
    assert not wrong.any(), "%s: %d hit ids differ from the model's, first at ray %d: %d, the model says %d (margin %g)" % (
        what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]), int(got_id[wrong][0]), int(idx[wrong][0]), float(margin[wrong][0]))
    both = ok & (idx >= 0)
    assert both.sum() > len(ok) // 4, what + ": too few hits to mean anything"
    p = _rows(o)[both] + t[both, None] * _rows(d)[both]
    e_t = float(rel_err(np.asarray(got_t)[both], t[both]).max())
    e_p = float(rel_err(np.asarray(got_p)[both], p).max())
    k_t, k_p = "t_closest_" + accel_name, "p_closest_" + accel_name
    print("%s: %d rays, %d hits, %d left out, max relative error of t %.3g (tolerance %.3g), of the point %.3g (tolerance %.3g)" % (
        what, len(ok), int(both.sum()), left, e_t, TOL[k_t], e_p, TOL[k_p]))
    assert e_t <= TOL[k_t], "%s: t is off by %g relative, tolerance %g" % (what, e_t, TOL[k_t])
    assert e_p <= TOL[k_p], "%s: the hit point is off by %g relative, tolerance %g" % (what, e_p, TOL[k_p])
    return e_t, e_p, left


def check_occluded(objects, o, d, got, what):
    """Any hit: equal to the model's on well-conditioned rays.  -> cases left out"""
    occ, margin = occluded(objects, o, d)
    ok, left = well_conditioned(margin, what)
    wrong = ok & (np.asarray(got, bool) != occ)
    print("%s: %d rays, %d occluded, %d left out" % (what, len(ok), int((ok & occ).sum()), left))
    assert not wrong.any(), "%s: %d rays differ from the model's, first at ray %d" % (what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]))
    assert 0 < (ok & occ).sum() < ok.sum(), what + ": the rays are all occluded or all free"
    return left


# ---- exact cases ----------------------------------------------------------------------------------------------------------------
# A scene of small dyadic numbers and rays on it whose float32 arithmetic is exact (no rounding, no 0 * inf): there the model's
# answer is the answer at margin 0 too, so the ties themselves are pinned: an origin exactly on a sphere counts as inside
# (scene.cpp:149-186, c > 0), a tangent ray hits (discriminant < 0 is the miss), beta = 0 and gamma = 0 are hits, t and
# |N.d| against 1e-4 at the neighbouring floats, an origin on a box's face, and the tie order and the sign of zero of the box normal.

# The camera, light and material in front of every small scene the tests write: the one definition
HEAD = """bclr 0 0 0
v
from 0 0 20
at 0 0 0
up 0 1 0
angle 40
hither 0.01
resolution 32 32
aperture 0
focal 1
l 0 10 10 1 1 1
f 0.8 0.8 0.8 0.9 1 1 1 0.3 20 0 1 0 0 0
"""

EDGES = HEAD + """p 3
0 0 0
2 0 0
0 2 0
s 4 0 0 1
box -1 3 -1 1 5 1
box -1 -5 0.5 1 -3 0.5
pl 0 -8 0  1 -8 0  0 -8 1
box -1 -1 9 1 1 11
"""
TRI, SPH, BOX_, FLAT, PLANE_, BOX0 = range(6)  # the objects of EDGES

_T4 = np.float32(1e-4)  # the float just under 1e-4
_T4_UP = np.nextafter(_T4, np.float32(1))
EXACT_RAYS = [  # (object, origin, direction, hit, t)
    (SPH, [5, 0, 0], [1, 0, 0], True, 0.0), (SPH, [5, 0, 0], [-1, 0, 0], True, 2.0), (SPH, [5, 0, 0], [0, 1, 0], True, 0.0),
    (SPH, [4, 0, 0], [0, 1, 0], True, 1.0), (SPH, [4, 1, -3], [0, 0, 1], True, 3.0), (SPH, [4, 1, 3], [0, 0, 1], False, None),
    (SPH, [0, 0, 0], [1, 0, 0], True, 3.0), (SPH, [0, 0, 0], [-1, 0, 0], False, None),
    (TRI, [0, 0, 1], [0, 0, -1], True, 1.0), (TRI, [2, 0, 1], [0, 0, -1], True, 1.0), (TRI, [0, 2, 1], [0, 0, -2], True, 0.5),
    (TRI, [1, 0, 1], [0, 0, -1], True, 1.0), (TRI, [1, 1, 1], [0, 0, -1], True, 1.0), (TRI, [0, 1, -1], [0, 0, 1], True, 1.0),
    (TRI, [0.5, 0.5, _T4], [0, 0, -1], False, None), (TRI, [0.5, 0.5, _T4_UP], [0, 0, -1], True, float(_T4_UP)),
    (TRI, [1.25, 1, 1], [0, 0, -1], False, None), (TRI, [0.5, 0.5, 1], [0, 0, 1], False, None),
    (BOX_, [1, 4, 0], [1, 0.5, 0.5], False, None), (BOX_, [1, 4, 0], [-1, 0.25, 0.25], True, 0.0), (BOX_, [0, 4, 0], [2, 0.5, 0.5], True, 0.5),
    (BOX_, [-3, 4, 0], [2, 0.25, 0.25], True, 1.0), (BOX_, [-3, 5, 0], [1, 1, 0.125], False, None),
    (FLAT, [0, -4, 2], [0.25, 0.25, -1], False, None),
    (PLANE_, [0, 0, 0], [1, -_T4, 0], False, None), (PLANE_, [0, 0, 0], [1, -_T4_UP, 0], True, 8.0 / float(_T4_UP)),
    (PLANE_, [3, -8, 2], [0, -1, 0], False, None), (PLANE_, [3, -8, 2], [0, 1, 0], False, None),
    (PLANE_, [0, -9, 0], [0, 1, 0], True, 1.0), (PLANE_, [0, -9, 0], [0, -1, 0], False, None), (PLANE_, [0, 0, 0], [0, -2, 0], True, 4.0),
]
EXACT_NORMALS = [  # (object, point, normal)
    (BOX_, [0, 4, 0], [0, 1, 0]), (BOX_, [0.5, 4.5, 0.25], [0, 1, 0]), (BOX_, [0.5, 4.25, 0.5], [1, 0, 0]), (BOX_, [0.5, 4.5, 0.5], [0, 1, 0]),
    (BOX_, [-0.5, 3.5, -0.5], [0, -1, 0]), (BOX_, [-0.5, 4.25, 0.5], [-1, 0, 0]), (BOX_, [0.25, 4, -0.5], [0, 0, -1]),
    (BOX_, [-1, 4.5, 0.5], [-1, 0, 0]), (BOX_, [0, 4, -0.25], [0, 0, -1]),
    (BOX0, [0, -0.0, 10], [0, 1, 0]), (BOX0, [-0.0, -0.0, 10], [0, 1, 0]), (BOX0, [-0.0, 0, 9], [0, 0, -1]), (BOX0, [-0.5, 0.5, 10.5], [0, 1, 0]),
    (SPH, [4, 0, 2], [0, 0, 1]), (SPH, [3.5, 0, 0], [-1, 0, 0]), (TRI, [9, 9, 9], [0, 0, 1]), (PLANE_, [9, 9, 9], [0, -1, 0]),
]


def check_exact(objects, intercepts_fn, normal_fn):
    """intercepts_fn(i, o, d) -> (hit, t, ...) and normal_fn(i, p) -> normals, of an oracle or a device scene of EDGES, on the
    exact cases: the decisions, t (a hit at t = 0 may be -0.0) and the normals equal the listed ones, which are the model's."""
    for i in sorted({c[0] for c in EXACT_RAYS}):
        cases = [c for c in EXACT_RAYS if c[0] == i]
        o, d = np.array([c[1] for c in cases], np.float32), np.array([c[2] for c in cases], np.float32)
        want_hit = np.array([c[3] for c in cases])
        want_t = np.array([np.nan if c[4] is None else c[4] for c in cases])
        hit, t, _ = intercepts(objects[i], o, d)
        with np.errstate(invalid="ignore"):  # the list is the model's, up to float64 rounding where t is not dyadic
            assert (hit == want_hit).all() and (np.abs(t - want_t)[hit] <= 1e-12 * np.maximum(1.0, want_t[hit])).all(), "the model, object %d" % i
        got = intercepts_fn(i, o, d)
        g_hit, g_t = np.asarray(got[0], bool), np.asarray(got[1], np.float32)
        assert (g_hit == want_hit).all(), "object %d: decisions %s, the exact answer is %s" % (i, g_hit.tolist(), want_hit.tolist())
        assert (g_t[want_hit] == want_t[want_hit].astype(np.float32)).all(), "object %d: t %s, the exact answer is %s" % (i, g_t.tolist(), want_t.tolist())
    for i in sorted({c[0] for c in EXACT_NORMALS}):
        cases = [c for c in EXACT_NORMALS if c[0] == i]
        p, want = np.array([c[1] for c in cases], np.float32), np.array([c[2] for c in cases], np.float64)
        assert (normal(objects[i], p)[0] == want).all(), "the model's normals, object %d" % i
        got = np.asarray(normal_fn(i, p))
        assert (got == want).all(), "object %d: normals %s, the exact answer is %s" % (i, got.tolist(), want.tolist())
