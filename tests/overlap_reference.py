"""A float64 model of the overlap query (p3d_host_scene_overlap_box, p3d_overlap_box_device, include/p3d_overlap.h), stated
differently from the rule of host/overlap_rule.hpp so that a mistake shared by the host form and the kernel cannot hide behind
their bit parity.  The model knows no separating axis:

  triangle  the triangle as a polygon, clipped against the six half-spaces of the box (Sutherland-Hodgman, the closed side
            kept, a crossing put exactly on the face it was cut by): overlap = something is left
  sphere    the smallest and the largest |x - c| over the box: the shell overlaps when min <= r <= max, the solid when min <= r
  box       intervals per axis: the solids overlap when all three pairs of intervals do; the faces unless the query box lies
            strictly inside the open interior
  plane     the heights of the eight corners: min <= 0 <= max

A box with lo > hi on some axis, or with a NaN, overlaps nothing.  A pair of a box and an object is WELL-CONDITIONED when the
model gives the same answer for the query box grown and shrunk by delta times the largest |coordinate| of the pair (a box that
is a point or a slab is not shrunk past its middle: it stays what it is); the others are left out of a comparison with this
model, at most MAX_LEFT_OUT of the pairs whose boxes overlap by comparison, per scene.  The GPU suite's bit comparisons cover
those too.

Also here: the boxes both suites draw for a scene, and a hand-built table of exact touching cases.

A reference module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import os

import numpy as np

import intersect_reference as ref
import nearest_reference as near

SPHERE, TRIANGLE, BOX, PLANE = ref.SPHERE, ref.TRIANGLE, ref.BOX, ref.PLANE
MAX_LEFT_OUT = 0.05
RUNGS = (1e-7, 1e-6, 1e-5, 1e-4)
# Measured: the smallest rung of RUNGS at which host_overlap_box has no disagreement with the model on the well-conditioned pairs
# of the fixed sets of test_overlap_reference.py (test_the_measured_rung prints the count per rung).  The test uses 4 x that: the
# project's usual margin over an error measured once.
MEASURED_DELTA = 1e-7
DELTA = 4.0 * MEASURED_DELTA
N_BOXES = 500
SPREAD = 1.75  # of a box's side, per axis: measured, 34 % to 63 % of a scene's boxes then find something


# ---- the model ------------------------------------------------------------------------------------------------------------------

def _clip(poly, axis, bound, keep_above):
    """One Sutherland-Hodgman step: the part of the polygon (a list of points) with x[axis] >= bound (or <=), closed"""
    out = []
    inside = lambda p: p[axis] >= bound if keep_above else p[axis] <= bound
    for a, b in zip(poly, poly[1:] + poly[:1]):
        if inside(a):
            out.append(a)
        if inside(a) != inside(b):
            t = (bound - a[axis]) / (b[axis] - a[axis])
            x = a + t * (b - a)
            x[axis] = bound  # exactly on the face: the next faces see no rounding of this one
            out.append(x)
    return out


def _triangle(ob, lo, hi):
    poly = [ob["p0"].copy(), ob["p1"].copy(), ob["p2"].copy()]
    for axis in range(3):
        for bound, above in ((lo[axis], True), (hi[axis], False)):
            poly = _clip(poly, axis, bound, above)
            if not poly:
                return False
    return True


def _sphere(ob, lo, hi, solid):
    c, r = ob["c"], abs(ob["r"])
    nearest = np.linalg.norm(c - np.clip(c, lo, hi))
    farthest = np.linalg.norm(np.maximum(np.abs(c - lo), np.abs(hi - c)))
    return bool(nearest <= r and (solid or farthest >= r))


def _box(ob, lo, hi, solid):
    mn, mx = ob["mn"], ob["mx"]
    if not ((lo <= mx).all() and (hi >= mn).all()):
        return False
    return bool(solid or not ((lo > mn).all() and (hi < mx).all()))


def _plane(ob, lo, hi):
    n = ref.unit_normal(ob)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    h = (corners - ob["p0"]) @ n
    return bool(h.min() <= 0 <= h.max())


def overlaps(ob, lo, hi, solid=False):
    """One object against one box (float64 (3,) each) -> bool"""
    if not (lo <= hi).all():  # inverted, or a NaN
        return False
    k = ob["kind"]
    if k == TRIANGLE:
        return _triangle(ob, lo, hi)
    if k == SPHERE:
        return _sphere(ob, lo, hi, solid)
    if k == BOX:
        return _box(ob, lo, hi, solid)
    return _plane(ob, lo, hi)


def extent(ob):
    """The object's own box (a plane has none: everything) and the largest |coordinate| it is given by"""
    k = ob["kind"]
    if k == SPHERE:
        return ob["c"] - abs(ob["r"]), ob["c"] + abs(ob["r"]), max(np.abs(ob["c"]).max(), abs(ob["r"]))
    if k == BOX:
        return ob["mn"], ob["mx"], max(np.abs(ob["mn"]).max(), np.abs(ob["mx"]).max())
    p = np.stack([ob["p0"], ob["p1"], ob["p2"]])
    if k == PLANE:
        return np.full(3, -np.inf), np.full(3, np.inf), np.abs(p).max()
    return p.min(0), p.max(0), np.abs(p).max()


def table(objects, lo, hi, solid=False, delta=DELTA):
    """(objects, boxes) -> (overlap bool, well-conditioned bool, the boxes overlap by comparison bool).  Only pairs whose own
    boxes come within the margin of each other are clipped: the others are a well-conditioned "no" """
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    n = len(lo)
    ans, ok, near_by = np.zeros((len(objects), n), bool), np.ones((len(objects), n), bool), np.zeros((len(objects), n), bool)
    valid = (lo <= hi).all(1)
    mid = (lo + hi) / 2
    for j, ob in enumerate(objects):
        olo, ohi, size = extent(ob)
        for i in np.nonzero(valid)[0]:
            eps = delta * max(size, np.abs(lo[i]).max(), np.abs(hi[i]).max())
            glo, ghi = lo[i] - eps, hi[i] + eps
            if not ((glo <= ohi).all() and (ghi >= olo).all()):
                continue
            near_by[j, i] = bool((lo[i] <= ohi).all() and (hi[i] >= olo).all())
            slo, shi = np.minimum(lo[i] + eps, mid[i]), np.maximum(hi[i] - eps, mid[i])
            ans[j, i] = overlaps(ob, lo[i], hi[i], solid)
            ok[j, i] = overlaps(ob, glo, ghi, solid) == overlaps(ob, slo, shi, solid) == ans[j, i]
    return ans, ok, near_by


# ---- the fixed inputs (shared by the CPU and the GPU suite) -----------------------------------------------------------------------

def scene_boxes(objects, seed, n=N_BOXES):
    """n query boxes for a scene -> (lo, hi) float32.  Sides of 2 % to 20 % of the scene's diagonal per axis; box i is centred
    near a random point of the surface of object i mod len(objects), up to SPREAD of its side away per axis, so that
    roughly half the boxes find something.  Every 16th box is degenerate, a point and a flat slab in turn; and in every 50 one box
    has lo > hi on an axis and one has a NaN"""
    rng = np.random.default_rng(seed)
    blo, bhi = near.scene_bounds(objects)
    diag = float(np.linalg.norm(bhi - blo))
    side = diag * rng.uniform(0.02, 0.20, (n, 3))
    on = np.stack([near.surface_point(objects[i % len(objects)], rng) for i in range(n)])
    centre = on + side * rng.uniform(-SPREAD, SPREAD, (n, 3))
    half = side / 2
    point, slab = np.nonzero(np.arange(n) % 32 == 7)[0], np.nonzero(np.arange(n) % 32 == 23)[0]
    half[point] = 0.0
    half[slab, rng.integers(0, 3, len(slab))] = 0.0
    lo, hi = (centre - half).astype(np.float32), (centre + half).astype(np.float32)  # (half 0: lo == hi, the same rounding)
    inverted = np.nonzero(np.arange(n) % 50 == 13)[0]
    axis = rng.integers(0, 3, len(inverted))
    lo[inverted, axis], hi[inverted, axis] = hi[inverted, axis] + np.float32(0.01 * diag), lo[inverted, axis]
    nan = np.nonzero(np.arange(n) % 50 == 37)[0]
    (lo if seed % 2 else hi)[nan, rng.integers(0, 3, len(nan))] = np.nan
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


BOXES_SCENE = (86, 10, 12, 10, 0)  # seed, spheres, triangles, boxes, planes: sweep_reference.SCENES has no box


def scene_paths(tmp):
    """name -> .p3f path: the seeded scenes of sweep_reference.scene_paths and one that holds boxes"""
    import fuzz_scenes
    import sweep_reference as sw
    paths = dict(sw.scene_paths(tmp))
    seed, s, t, b, p = BOXES_SCENE
    paths["boxes"] = fuzz_scenes.random_scene(seed, os.path.join(str(tmp), "overlap_boxes.p3f"), n_spheres=s, n_tris=t, n_boxes=b, n_planes=p)
    return paths


# ---- the exact table ------------------------------------------------------------------------------------------------------------
# Touching cases with small dyadic coordinates, for which every float32 product and sum of the rule is exact: the rule must
# answer "overlap" with no tolerance at all.  EXACT_SCENE is the .p3f body (after intersect_reference.HEAD); EXACT: (what, object
# index, lo, hi, solid, overlap).  The objects lie far apart, so each case is about one of them.

EXACT_SCENE = ("p 3\n1 0 0\n3 0 0\n1 2 0\n"               # 0: a triangle in the plane z = 0
               "s 10 0 0 1\n"                             # 1: a sphere of radius 1 at (10, 0, 0)
               "box 20 0 0 24 4 4\n"                      # 2: a box
               "p 3\n30 0 0\n32 0 2\n30 2 2\n")           # 3: a tilted triangle, normal (-4, -4, 4)
EXACT = (
    ("a face through a vertex", 0, (-1, -1, -1), (1, 1, 1), False, True),          # x = 1 holds the vertices (1, 0, 0) and (1, 2, 0)
    ("a face through one vertex only", 0, (3, -1, -1), (4, 1, 1), False, True),    # x = 3 holds (3, 0, 0)
    ("an edge of the box through a vertex", 0, (3, -2, -1), (4, 0, 1), False, True),
    ("a face along an edge", 0, (0, -2, -1), (4, 0, 1), False, True),              # y = 0 holds the edge A B
    ("a face flush with the triangle's plane", 0, (1.25, 0.25, 0), (1.5, 0.5, 1), False, True),
    ("flush from below", 0, (1.25, 0.25, -1), (1.5, 0.5, 0), False, True),
    ("a corner on the hypotenuse", 0, (2, 1, -1), (3, 2, 1), False, True),         # (2, 1, 0) lies on B C
    ("just off the hypotenuse", 0, (2.25, 1, -1), (3, 2, 1), False, False),
    ("a slab in the triangle's plane", 0, (0, 0, 0), (4, 4, 0), False, True),
    ("a point on the triangle", 0, (1.5, 0.5, 0), (1.5, 0.5, 0), False, True),
    ("the tilted triangle, two corners on its plane", 3, (30.5, 0.5, 1), (31, 1, 2), False, True),   # z = x - 30 + y at (30.5, 0.5, 1) and (31, 1, 2)
    ("the tilted triangle, just above", 3, (30, 0, 1.25), (30.5, 0.5, 2), False, False),
    ("a sphere tangent to a face from outside", 1, (11, -1, -1), (12, 1, 1), False, True),
    ("tangent from outside, solid", 1, (11, -1, -1), (12, 1, 1), True, True),
    ("a sphere tangent to the farthest corner from inside", 1, (10, 0, 0), (11, 0, 0), False, True),  # the corner (11, 0, 0) is on the shell
    ("wholly inside the shell", 1, (9.75, -0.25, -0.25), (10.25, 0.25, 0.25), False, False),
    ("wholly inside, solid", 1, (9.75, -0.25, -0.25), (10.25, 0.25, 0.25), True, True),
    ("apart from the sphere", 1, (11.25, -1, -1), (12, 1, 1), True, False),
    ("a box in a box", 2, (21, 1, 1), (23, 3, 3), False, False),
    ("a box in a box, solid", 2, (21, 1, 1), (23, 3, 3), True, True),
    ("a box in a box, one face shared", 2, (20, 1, 1), (23, 3, 3), False, True),
    ("a box touching a box's corner", 2, (24, 4, 4), (25, 5, 5), False, True),
    ("a box apart from a box", 2, (24.5, 0, 0), (25, 1, 1), True, False),
)
EXACT_PLANES = "pl 0 0 1\n1 0 1\n0 1 1\n" "pl 0 0 0\n0 1 1\n1 0 0\n"  # 0: z = 1;  1: through the origin, normal along (0, 1, -1) / sqrt 2
EXACT_PLANE_CASES = (
    ("a plane through a corner", 0, (2, 2, 1), (3, 3, 2), True),
    ("a plane through the top face", 0, (2, 2, 0), (3, 3, 1), True),
    ("a plane above the box", 0, (2, 2, -1), (3, 3, 0.5), False),
    ("a diagonal plane through a corner", 1, (1, 2, 1), (2, 3, 2), True),   # y - z = 0 at (x, 2, 2)
    ("a diagonal plane past the box", 1, (1, 2.5, 1), (2, 3, 2), False),
)
