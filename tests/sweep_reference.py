"""A float64 model of the sphere sweep (p3d_host_scene_sweep_sphere, p3d_sweep_sphere_device, include/p3d_sweep.h), stated
differently from the rule of host/sweep_rule.hpp so that a mistake shared by the host form and the kernel cannot hide behind
their bit parity.  The model solves no quadratic and knows no face, edge or vertex: it only evaluates
nearest_reference.distance along the centre line c(t) = o + t d and searches.

  triangle, plane   the distance to a convex set along a line is convex in t: a ternary search over [0, t_end] finds its
                    minimum; a minimum above r is a miss; otherwise the first t with distance = r is found by bisection on
                    [0, t*], where the distance decreases
  sphere shell      | |c(t) - m| - R | is not convex, but monotone on at most four pieces, cut where the distance to the CENTRE
                    (a sphere of radius 0: distance again) is smallest, by ternary search, and where it crosses R, by bisection;
                    the same two steps on each piece in turn
  all kinds         T = the smallest T_j, the object that has it

t_end is the limit; without one a window that ends outside the scene's bounds grown by the ball (scene_window).  The MARGIN
of a case is the smallest | min_t dist_j - r | / max(1, r) over the objects: how far the case is from flipping a hit / miss
decision (a grazing contact).  A case under THRESHOLD is ill-conditioned and may be left out of the decision checks, at most
MAX_LEFT_OUT of a test's cases; the GPU suite's bit comparisons cover those too.  A ball that still approaches an object (a
plane: the others lie inside the window) when an unlimited window ends, without having met it, gets margin 0.

A reference module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import functools
import os

import numpy as np

import intersect_reference as ref
import nearest_reference as near

SPHERE, TRIANGLE, BOX, PLANE = ref.SPHERE, ref.TRIANGLE, ref.BOX, ref.PLANE
THRESHOLD = ref.THRESHOLD
MAX_LEFT_OUT = ref.MAX_LEFT_OUT
FACTORS = (0.5, 0.9, 1.1, 2.0)  # segment_reference.FACTORS: of the model's distance or T; never within 10 % of what they decide
FLOOR = 1e-3                    # a centre line nearer than this to its target gets a radius from the target's size instead
N_RAYS = 2000
FLT_MAX = np.finfo(np.float32).max
WINDOW = 100.0
TERNARY, BISECT = 120, 60       # (2/3)^120 and 2^-60 of the window: below float64's spacing

# Measured: the largest error of HostScene's sweep (host_sweep_sphere on the CPU; the GPU must equal its bits, so on these inputs
# its error is the host form's) over the fixed sets of test_sweep_api.py, as intersect_reference.rel_err counts it:
# |got - want| / max(1, |want|).  The asserted tolerance is 4 x the measured maximum: room for another seed or scene, not for
# another implementation.  All are far under 1e-4, the project's colour tolerance.
MEASURED = {
    "t": 1.02e-5,           # (a) t against the model's T (worst: mixed_planes, a plane met far away; without planes 1.44e-6)
    "at_radius": 4.85e-6,   # (b) the model's distance from the reported centre to the reported object against r (T = 0: not above r)
    "on_surface": 3.58e-6,  # (c) the model's distance from the reported contact point to the reported object, against 0
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}


# ---- the model ------------------------------------------------------------------------------------------------------------------

def _ternary(f, lo, hi):
    """argmin of a convex (or monotone) f over [lo, hi], elementwise"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(TERNARY):
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        left = f(m1) <= f(m2)
        lo, hi = np.where(left, lo, m1), np.where(left, m2, hi)
    return (lo + hi) / 2


def _first_at(f, lo, hi, level):
    """f decreasing on [lo, hi] with f(lo) > level >= f(hi): the first t with f(t) <= level, elementwise"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(BISECT):
        mid = (lo + hi) / 2
        above = f(mid) > level
        lo, hi = np.where(above, mid, lo), np.where(above, hi, mid)
    return hi


def _convex(ob, o, d, r, t_end):
    """-> (T or NaN, the smallest distance over the window, whether that lies at the window's end)"""
    f = lambda t: near.distance(ob, o + t[:, None] * d)
    zero = np.zeros(len(o))
    ts = _ternary(f, zero, t_end)
    f0, fs, fe = f(zero), f(ts), f(t_end)
    t_star = np.where(f0 <= fs, zero, ts)
    t_star = np.where(fe < np.minimum(f0, fs), t_end, t_star)
    f_min = np.minimum(np.minimum(f0, fs), fe)
    with np.errstate(invalid="ignore"):
        T = np.where(f0 <= r, 0.0, _first_at(f, zero, t_star, r))
        return np.where(f_min <= r, T, np.nan), f_min, (t_star >= t_end * (1 - 1e-9)) & (t_end > 0)


def _shell(ob, o, d, r, t_end):
    centre = dict(kind=SPHERE, c=ob["c"], r=0.0)
    u = lambda t: near.distance(centre, o + t[:, None] * d)
    g = lambda t: near.distance(ob, o + t[:, None] * d)
    R = ob["r"]
    zero = np.zeros(len(o))
    t0 = _ternary(u, zero, t_end)
    t0 = np.where(u(zero) <= u(t0), zero, t0)
    t0 = np.where(u(t_end) < u(t0), t_end, t0)
    down = (u(zero) > R) & (u(t0) <= R)
    up = (u(t0) < R) & (u(t_end) >= R)
    ca = np.where(down, _first_at(u, zero, t0, R), zero)
    cb = np.where(up, _first_at(lambda t: -u(t), t0, t_end, -R), t0)
    cuts = [zero, ca, t0, cb, t_end]
    T = np.full(len(o), np.nan)
    g_min = g(zero)
    for a, b in zip(cuts[:-1], cuts[1:]):
        ga, gb = g(a), g(b)
        g_min = np.minimum(g_min, np.minimum(ga, gb))
        here = np.where(ga <= r, a, np.where(gb <= r, _first_at(g, a, b, r), np.nan))
        T = np.where(np.isnan(T), here, T)
    return T, g_min, np.zeros(len(o), bool)


def scene_window(objects, o, d, r):
    """The end of an unlimited search: WINDOW times the way to where the centre is surely farther than r outside the scene's
    bounds (a plane has none: a ball that creeps up on one may meet it later than that)"""
    lo, hi = near.scene_bounds(objects)
    mid, half = (lo + hi) / 2, np.linalg.norm(hi - lo) / 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t = WINDOW * (np.linalg.norm(o - mid, axis=1) + half + r + 1.0) / np.linalg.norm(d, axis=1)
    return np.where(np.isfinite(t), t, 1.0)  # (a zero direction: the ball stands still, any window)


def table(objects, o, d, r, t_max=None):
    """-> (T (objects, rays), NaN where object j is not met; margin (rays,))"""
    o, d, r = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(r, np.float64)
    limited = t_max is not None
    t_end = np.asarray(t_max, np.float64) if limited else scene_window(objects, o, d, r)
    T = np.empty((len(objects), len(o)))
    margin = np.full(len(o), np.inf)
    for j, ob in enumerate(objects):
        assert ob["kind"] != BOX, "a box is not swept"
        T[j], f_min, at_end = (_shell if ob["kind"] == SPHERE else _convex)(ob, o, d, r, t_end)
        m = np.abs(f_min - r) / np.maximum(1.0, r)
        if not limited:
            m = np.where(at_end & (f_min > r), 0.0, m)  # still approaching when the window ends
        margin = np.minimum(margin, m)
    return T, margin


def first_contact(T):
    """-> (object or -1, T or NaN) from a table"""
    with np.errstate(invalid="ignore"):
        filled = np.where(np.isnan(T), np.inf, T)
    obj = filled.argmin(0)
    best = filled[obj, np.arange(T.shape[1])]
    none = ~np.isfinite(best)
    return np.where(none, -1, obj), np.where(none, np.nan, best)


# ---- the fixed inputs (shared by the CPU and the GPU suite) -----------------------------------------------------------------------

def balls(objects, seed, n=N_RAYS):
    """n moving balls for a scene -> (origin, direction, radius) float32.  Ball i is aimed near target object i mod len(objects)
    as intersect_reference.object_rays aims its rays, and by i mod 4:
      0, 1  r = a factor from FACTORS times the model's smallest distance from the centre line to the target (never within
            10 % of it, so the target's decision is well conditioned by construction); a line that meets the target gets 0.05
            to 0.25 of the target's size times the factor instead.  Every 32nd ball is a point, r = 0: its line meets the
            target (margin 0 by the definition above) or the margin is the miss distance
      2     the start overlaps: the origin is moved to within r / 2 of a point of the target's surface (T = 0); other objects
            in the way of the other balls add to this quarter
      3     a sphere: the start lies inside the shell; the others: as 0, 1"""
    rng = np.random.default_rng(seed)
    per = -(-n // len(objects))
    o, d = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
    r = np.empty(n, np.float32)
    for j, ob in enumerate(objects):
        idx = np.arange(j, n, len(objects))
        oj, dj = ref.object_rays(ob, seed + 17 * j, per)
        oj, dj = oj[:len(idx)].copy(), dj[:len(idx)].copy()
        size = ref.bounding_sphere(ob)[1]
        sort = idx % 4
        if ob["kind"] == SPHERE:
            inside = sort == 3
            oj[inside] = (ob["c"] + 0.9 * ob["r"] * ref._in_ball(rng, int(inside.sum()))).astype(np.float32)
        o64, d64 = oj.astype(np.float64), dj.astype(np.float64)
        _, reach, _ = (_shell if ob["kind"] == SPHERE else _convex)(ob, o64, d64, np.zeros(len(idx)), scene_window(objects, o64, d64, 0.0))
        factor = np.array(FACTORS)[rng.integers(0, len(FACTORS), len(idx))]
        rj = np.where(reach < FLOOR, factor * size * rng.uniform(0.05, 0.25, len(idx)), factor * reach)
        if ob["kind"] == SPHERE:  # inside a shell the line always meets it: a share of the room to the shell, 1.1 and 2.0 overlap at the start
            room = np.abs(np.linalg.norm(o64 - ob["c"], axis=1) - ob["r"])
            rj = np.where(sort == 3, 0.6 * factor * room, rj)
        rj = np.where(idx % 32 == 1, 0.0, rj)
        touch = sort == 2
        rj = np.where(touch, size * rng.uniform(0.05, 0.5, len(idx)), rj)
        on = np.stack([near.surface_point(ob, rng) for _ in range(int(touch.sum()))]) if touch.any() else np.zeros((0, 3))
        oj[touch] = (on + 0.5 * rj[touch, None] * ref._unit(rng, len(on))).astype(np.float32)
        o[idx], d[idx], r[idx] = oj, dj, rj.astype(np.float32)
    return o, d, r


def draw_limits(T, window, seed):
    """One float32 limit per ball: 0.5 or 2 times the model's T (never within a factor of 2 of it); where nothing is met, or at the
    start, a quarter of the unlimited window; then every 25th a zero, a negative number or a NaN in turn"""
    rng = np.random.default_rng(seed)
    factor = np.array((0.5, 2.0))[rng.integers(0, 2, len(T))]
    with np.errstate(invalid="ignore"):
        lim = np.where(T > FLOOR, factor * T, 0.25 * window).astype(np.float32)
    lim[0::75], lim[25::75], lim[50::75] = 0.0, -1.5, np.nan
    return lim


def box_balls(lo, hi, seed, n=N_RAYS):
    """n balls for a scene known by its bounds only (the large meshes) -> (origin, direction, radius) float32: origins in the
    bounds grown by half, directions of length 0.2 to 5, radii log-uniform from 1e-5 to 0.3 of the diagonal, every 16th a point
    (r = 0) and every 16th larger than the scene, so that the grown box of every node holds the start"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    mid, half, diag = (lo + hi) / 2, (hi - lo) / 2, float(np.linalg.norm(hi - lo))
    o = mid + 1.5 * half * rng.uniform(-1, 1, (n, 3))
    d = ref._unit(rng, n) * np.exp(rng.uniform(np.log(0.2), np.log(5.0), n))[:, None]
    r = diag * np.exp(rng.uniform(np.log(1e-5), np.log(0.3), n))
    r[0::16], r[8::16] = 0.0, diag * rng.uniform(1.5, 3.0, len(r[8::16]))
    return o.astype(np.float32), d.astype(np.float32), r.astype(np.float32)


SCENES = {  # name -> (seed, spheres, triangles, planes): no boxes; planes go through accel None only (Q12)
    "spheres": (81, 12, 0, 0), "triangles": (82, 0, 14, 0), "planes": (83, 0, 0, 3), "mixed": (84, 6, 8, 0), "mixed_planes": (85, 4, 6, 2),
}
NO_PLANES = ("spheres", "triangles", "mixed")


def scene_paths(tmp):
    """name -> .p3f path of the random scenes both suites use, written under `tmp`"""
    import fuzz_scenes
    return {name: fuzz_scenes.random_scene(seed, os.path.join(str(tmp), "sweep_%s.p3f" % name), n_spheres=s, n_tris=t, n_boxes=0, n_planes=p)
            for name, (seed, s, t, p) in SCENES.items()}


class Cases:
    """The fixed set of one scene, and the model's answers for it (computed once per path and shared)"""

    def __init__(self, path, seed, n=N_RAYS):
        self.objects = ref.load_objects(path)
        self.o, self.d, self.r = balls(self.objects, seed, n)
        self.free_T, self.free_margin = table(self.objects, self.o, self.d, self.r)
        window = scene_window(self.objects, self.o.astype(np.float64), self.d.astype(np.float64), self.r.astype(np.float64))
        self.limits = draw_limits(first_contact(self.free_T)[1], window, seed + 50)
        usable = np.where(self.limits > 0, self.limits, 1.0).astype(np.float64)  # (a zero, negative or NaN limit decides by itself)
        self.lim_T, self.lim_margin = table(self.objects, self.o, self.d, self.r, usable)
        dead = ~(self.limits > 0)
        self.lim_T[:, dead] = np.nan
        self.lim_margin[dead] = np.inf


@functools.lru_cache(maxsize=None)
def cases(path, seed, n=N_RAYS):
    return Cases(path, seed, n)


# ---- the assertions, the same for host_sweep_sphere (CPU suite) and the kernel's outputs (GPU suite) ------------------------------

def check_sweep(objects, o, d, r, T, margin, got, what, mixed=True):
    """got = (object, t, centre, contact) against a table of the model -> the three measured errors and the cases left out"""
    obj, t, centre, contact = got
    want_obj, want_t = first_contact(T)
    ok = margin >= THRESHOLD
    left = int((~ok).sum())
    assert left <= MAX_LEFT_OUT * len(ok), "%s: %d of %d decisions are grazing, over the %g cap" % (what, left, len(ok), MAX_LEFT_OUT)
    hit = want_obj >= 0
    wrong = ok & ((obj >= 0) != hit)
    assert not wrong.any(), "%s: %d decisions differ from the model's, first at ball %d (margin %g)" % (
        what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]), float(margin[wrong][0]))
    if mixed:
        assert 0 < (ok & hit).sum() < ok.sum(), what + ": the balls all meet something or all nothing"
    none = obj < 0
    assert (t[none] == FLT_MAX).all() and not centre[none].any() and not contact[none].any(), what + ": the no-answer values"
    both = ok & hit & ~none
    n = len(obj)
    err = {"t": float(ref.rel_err(t[both], want_t[both]).max()) if both.any() else 0.0}
    r64 = np.asarray(r, np.float64)
    off, on = np.zeros(n), np.zeros(n)
    for j in np.unique(obj[~none]):
        m = obj == j
        dist = near.distance(objects[j], centre[m])
        off[m] = np.where(t[m] == 0, np.maximum(dist - r64[m], 0.0), np.abs(dist - r64[m])) / np.maximum(1.0, r64[m])
        on[m] = near.distance(objects[j], contact[m])
    err["at_radius"], err["on_surface"] = float(off.max()), float(on.max())
    o64, step = np.asarray(o, np.float64), np.asarray(t, np.float64)[:, None] * np.asarray(d, np.float64)
    # centre = o + d * t in float32: a product and a sum, each within half an ulp of a value no larger than |o| + |d t|
    assert (np.abs(centre - (o64 + step))[both] <= 2.0 ** -23 * (np.abs(o64) + np.abs(step))[both]).all(), what + ": centre is not o + t d"
    print("%s: %d balls, %d met, %d at the start, %d left out, errors %s (tolerances %s)" % (
        what, n, int((ok & hit).sum()), int((ok & hit & (want_t == 0)).sum()), left, {k: "%.3g" % v for k, v in err.items()},
        {k: "%.3g" % v for k, v in TOL.items()}))
    return err, left


def assert_within(err, what):
    for k, v in err.items():
        assert v <= TOL[k], "%s: %s is off by %g, tolerance %g" % (what, k, v, TOL[k])
