"""A float64 model of the Whitted shading chain (rayTracing, main.cpp:92-309), built on the geometric model of
intersect_reference.py and stated in formulas of its own, so that a misreading shared by the kernels and the CPU oracle cannot
hide behind their bit parity.  Plain numpy, vectorised over pixels, one batch per chain level.

The configuration: antialiasing = 0, no soft shadows, no lens, no skybox, debug_view = 0: one ray through each pixel centre.

  primary   eye = from, f = (at - from) / |at - from|, r = (up x -f) normalised, v = -f x r; the ray through pixel (x, y), row 0
            at the bottom, goes along f + tan(angle / 2) ((2 (x + .5) / rx - 1) (rx / ry) r + (2 (y + .5) / ry - 1) v).
  hit       the nearest hit over all objects at P; the shading point S is P moved 1e-4 along the geometric normal at P (towards
            the normal's side, whichever side the ray came from); N is the normal at S.
  lights    only outside an object (Q7).  A light at L counts unless ANY object is hit along the feeler from S towards L, at
            any distance, beyond the light too (Q5).  With l the unit vector to the light and h the unit bisector of l and -d, a
            counted light adds  Kd cd col max(0, N.l)  +  Ks cs col max(0, N.h)^shine.
  clamp     the colour of every level is clamped to [0, 1] (Q4).
  opaque    (T == 0)  + Ks x the colour along d - 2 (d.N) N from S (no ray when Ks == 0).
  glass     (T != 0)  + 1 x the colour along the Snell direction, no Fresnel term (Q3); the index ratio is ior_1 / ior when
            entering and ior_1 / 1 when leaving, ior_1 being the index of the medium the ray is in (1 at the eye, the
            material's after entering); the normal faces the ray (flipped inside); the refracted ray starts at P moved 1e-4
            along its own direction; inside becomes outside and the other way round.  Total internal reflection adds nothing.
  miss      the background colour, unclamped.
  depth     a level with no depth left returns its clamped local term.

Q3 makes the recursion a chain: trace() follows it once to the largest depth asked for and keeps every level's local term and
weight; fold() then gives the frame of any smaller maximum depth from the same chain.

MARGINS.  Every pixel gets the smallest margin met along its chain, in the units of intersect_reference (under THRESHOLD =
1e-3: ill-conditioned, left out of a comparison, the share left out capped at MAX_LEFT_OUT per frame): the closest() margin of
every level, the occluded() margin of every feeler whose light could add anything, |1 - sin^2(theta_t)| at a Snell decision, and
the margin of the box normal at a hit on a box.

A ray that starts ON an object - feeler, reflection, refraction - needs a margin of its own for that object.  Its origin is 1e-4
off the surface, so the generic margin of that object's test ("the origin is on the surface": 2e-4 / r for a sphere) calls every
such ray ill-conditioned.  But 1e-4 is two orders of magnitude above the float32 noise of a hit point at these scene sizes
(an ulp at 8 is 1e-6), so which side the origin is on is safe, and the decision "does the ray meet its own object again"
can flip only when the ray grazes: from 1e-4 outside a sphere of radius r the rays within sqrt(2e-4 / r) of the tangent plane
(0.02 at r = 0.5) still miss it, and noise moves that cone's edge by about a hundredth of itself.  The model therefore answers
the ray's own object by the exact test and gives that answer the margin |N.dir| / GRAZE x THRESHOLD with GRAZE = 0.05: under
0.05 from the tangent plane the ray is left out.  Two cases get margin 0: a ray that crosses the triangle or plane it starts on
(t there is 1e-4 / |N.dir| against the test's own 1e-4 bound), and a shading point on a box that the box's normal (the axis of
the largest |p - centre| component: the face normal only on a cube) has not lifted off the surface.  Every other object keeps
its generic margin.

Deliberately NOT stated here: anti-aliasing, soft shadows, the lens, the skybox, the path tracer; Q1 / Q2 (the BVH's any-hit can
lose an occluder, depending on the tree's shape and the stack's history: frames over a BVH are held to the model where the model
finds every feeler free, and from below elsewhere); Q8's ulps (directions here are exact unit vectors)."""
import numpy as np

import intersect_reference as geo

THRESHOLD = geo.THRESHOLD
MAX_LEFT_OUT = 0.15  # the share of a frame's pixels that may be ill-conditioned
GRAZE = 0.05         # |N.dir| under which a ray leaving a surface is taken to graze it
OFFSET = 1e-4
MIN_BRANCH_PIXELS = 50

MISS, OPAQUE, ENTER, LEAVE, TIR = 0, 1, 2, 3, 4  # the branch of a chain level; NONE: the chain has ended above
NONE = -1
BRANCHES = ("lit", "shadowed", "opaque bounce", "enter", "leave", "TIR", "miss after a bounce", "inner-level clamp")

# Measured: the largest |oracle - model| of a colour component over the well-conditioned pixels of the fixed frames of
# test_shading_reference.py (CPU oracle, accel None, grid and - where the model finds every feeler free - BVH), for frames of
# maximum depth 0 and for deeper ones.  The asserted tolerance is 4 x the measured maximum: room for another compiler's
# contraction choices and for moved float32 geometry, not for another formula.
MEASURED = {"depth0": 1.8e-5, "deeper": 8.6e-5}  # on the CPU oracle (x86-64, g++ -O2); the largest are glossy highlights, shine 100
TOL = {k: 4.0 * v for k, v in MEASURED.items()}


# ---- the scene file ---------------------------------------------------------------------------------------------------------------

def load_scene(path):
    """-> dict(objects, material (index per object), materials (n, 14: cd Kd cs Ks shine T ior em), lights (n, 6: position,
    colour), bclr, camera(from_, at, up, angle, res)), every number the float32 a loader reads, held in float64."""
    with open(path) as f:
        tok = [w for line in f for w in line.split("#")[0].split()]
    f32 = lambda ws: np.array([np.float32(w) for w in ws], np.float32).astype(np.float64)
    skip = {"s": 4, "p": 10, "box": 6, "pl": 9, "hither": 1, "aperture": 1, "focal": 1, "v": 0}
    materials, lights, material, cam, bclr = [], [], [], {}, np.zeros(3)
    i = 0
    while i < len(tok):
        w = tok[i]
        i += 1
        if w == "f":
            materials.append(f32(tok[i:i + 14])); i += 14
        elif w == "l":
            lights.append(f32(tok[i:i + 6])); i += 6
        elif w == "bclr":
            bclr = f32(tok[i:i + 3]); i += 3
        elif w in ("from", "at", "up"):
            cam["from_" if w == "from" else w] = f32(tok[i:i + 3]); i += 3
        elif w == "angle":
            cam["angle"] = float(np.float32(tok[i])); i += 1
        elif w == "resolution":
            cam["res"] = (int(tok[i]), int(tok[i + 1])); i += 2
        else:
            if w in ("s", "p", "box", "pl"):
                material.append(len(materials) - 1)
            i += skip[w]
    objects = geo.load_objects(path)
    assert len(objects) == len(material)
    return dict(objects=objects, material=np.array(material), materials=np.array(materials).reshape(-1, 14),
                lights=np.array(lights).reshape(-1, 6), bclr=bclr, camera=cam)


def camera(from_, at, up, angle, res):
    """A camera for trace(): the numbers of a `v` block, rounded to float32 as a loader or look_at takes them"""
    r32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    return dict(from_=r32(from_), at=r32(at), up=r32(up), angle=float(np.float32(angle)), res=(int(res[0]), int(res[1])))


def primary_rays(cam):
    """-> (origins, unit directions), (ry * rx, 3), row 0 at the bottom"""
    rx, ry = cam["res"]
    f = cam["at"] - cam["from_"]
    f = f / np.sqrt(f @ f)
    r = np.cross(cam["up"], -f)
    r = r / np.sqrt(r @ r)
    v = np.cross(-f, r)
    half = np.tan(np.radians(cam["angle"]) / 2)
    sx = (2 * (np.arange(rx) + 0.5) / rx - 1) * half * rx / ry
    sy = (2 * (np.arange(ry) + 0.5) / ry - 1) * half
    d = f[None, None, :] + sx[None, :, None] * r[None, None, :] + sy[:, None, None] * v[None, None, :]
    d = d.reshape(-1, 3)
    d = d / np.sqrt((d * d).sum(-1))[:, None]
    return np.broadcast_to(cam["from_"], d.shape).copy(), d


# ---- queries that know the object a ray starts on ---------------------------------------------------------------------------------

def _dot(a, b):
    return (a * b).sum(-1)


def _chunks(n, size=24):
    return [np.arange(a, min(a + size, n)) for a in range(0, n, size)]


def _groups(ids):
    """[(id, positions)] of the distinct values of `ids`"""
    order = np.argsort(ids, kind="stable")
    vals, starts = np.unique(ids[order], return_index=True)
    return [(int(v), order[a:b]) for v, a, b in zip(vals, starts, list(starts[1:]) + [len(ids)])]


def _own(objects, o, d, own, own_p, own_n):
    """The object each ray starts on (own < 0: none), by the exact test -> (hit, t, margin): see MARGINS above."""
    n = len(o)
    hit, t, margin = np.zeros(n, bool), np.full(n, np.inf), np.full(n, np.inf)
    for s, at in _groups(own):
        if s < 0:
            continue
        ob = objects[s]
        idx, ts, _, _ = geo.closest([ob], o[at], d[at])
        hit[at], t[at] = idx >= 0, np.where(idx >= 0, ts, np.inf)
        nd = _dot(own_n[at], d[at])
        m = np.abs(nd) / GRAZE * THRESHOLD
        if ob["kind"] in (geo.TRIANGLE, geo.PLANE):
            leaving = _dot(o[at] - own_p[at], own_n[at]) * nd > 0
            m = np.where(leaving, m, 0.0)
        margin[at] = m
    return hit, t, margin


def closest(objects, o, d, own=None, own_p=None, own_n=None):
    """geo.closest over all objects, the ray's own object answered by _own -> (index or -1, t, margin)"""
    n = len(o)
    own = np.full(n, -1) if own is None else own
    idx, t, margin = np.full(n, -1), np.full(n, np.inf), np.full(n, np.inf)
    second = np.full(n, np.inf)

    def offer(i_new, t_new):  # keeps the nearest and the second nearest t
        nonlocal idx, t, second
        nearer = t_new < t
        second = np.where(nearer, t, np.minimum(second, t_new))
        idx, t = np.where(nearer, i_new, idx), np.where(nearer, t_new, t)

    for ch in _chunks(len(objects)):
        mine = (own >= ch[0]) & (own <= ch[-1])
        sets = [(-1, np.nonzero(~mine)[0])] + [(s, np.nonzero(mine)[0][at]) for s, at in _groups(own[mine])]
        c_idx, c_t, c_gap, c_m = np.full(n, -1), np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf)
        for s, at in sets:
            keep = np.array([k for k in ch if k != s])
            if len(at) and len(keep):
                i, tt, gap, m = geo.closest([objects[k] for k in keep], o[at], d[at])
                c_idx[at], c_t[at], c_gap[at], c_m[at] = np.where(i >= 0, keep[np.maximum(i, 0)], -1), np.where(i >= 0, tt, np.inf), gap, m
        offer(c_idx, c_t)
        second = np.minimum(second, c_t + c_gap)
        margin = np.minimum(margin, c_m)
    if (own >= 0).any():
        hit, t_own, m_own = _own(objects, o, d, own, own_p, own_n)
        offer(np.where(hit, own, -1), t_own)
        margin = np.minimum(margin, m_own)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(t), (second - t) / np.maximum(1.0, np.abs(t)), np.inf)
    return idx, t, np.minimum(margin, np.nan_to_num(gap, nan=0.0))


def occluded(objects, o, d, own, own_p, own_n):
    """geo.occluded over all objects, the ray's own object answered by _own -> (occluded, margin): the best margin among the
    hits of an occluded ray, the worst of all objects for a free one."""
    n = len(o)
    occ, best, worst = np.zeros(n, bool), np.full(n, -np.inf), np.full(n, np.inf)
    for ch in _chunks(len(objects)):
        mine = (own >= ch[0]) & (own <= ch[-1])
        sets = [(-1, np.nonzero(~mine)[0])] + [(s, np.nonzero(mine)[0][at]) for s, at in _groups(own[mine])]
        for s, at in sets:
            obs = [objects[k] for k in ch if k != s]
            if len(at) and obs:
                c, m = geo.occluded(obs, o[at], d[at])
                occ[at] |= c
                best[at] = np.where(c, np.maximum(best[at], m), best[at])
                worst[at] = np.where(c, worst[at], np.minimum(worst[at], m))
    hit, _, m_own = _own(objects, o, d, own, own_p, own_n)
    occ |= hit
    best = np.where(hit, np.maximum(best, m_own), best)
    worst = np.where(hit, worst, np.minimum(worst, m_own))
    return occ, np.where(occ, best, worst)


def normals(objects, idx, p):
    """The geometric normal of object idx[k] at p[k] -> (normals, margins)"""
    n, m = np.zeros_like(p), np.full(len(p), np.inf)
    for s, at in _groups(idx):
        n[at], m[at] = geo.normal(objects[s], p[at])
    return n, m


def _off_the_box(objects, idx, s):
    """For shading points on boxes: inf where the point is clear of the box's surface, else 0"""
    out = np.full(len(s), np.inf)
    for k, at in _groups(idx):
        ob = objects[k]
        if ob["kind"] == geo.BOX:
            c, half = (ob["mn"] + ob["mx"]) / 2, (ob["mx"] - ob["mn"]) / 2
            out[at] = np.where((np.abs(s[at] - c) - half).max(-1) > OFFSET / 2, np.inf, 0.0)
    return out


# ---- the chain ----------------------------------------------------------------------------------------------------------------------

def trace(scene, objects=None, cam=None, max_depth=4):
    """Follows every pixel's chain for max_depth + 1 levels -> dict(res, bclr, hit (primary hit IDs), levels: a list of dicts
    of per-pixel arrays: branch, local (the unclamped local term), weight (of the level below), margin, lit, shadowed)."""
    objects = scene["objects"] if objects is None else objects
    cam = scene["camera"] if cam is None else cam
    mats, lights = scene["materials"], scene["lights"]
    o, d = primary_rays(cam)
    n = len(o)
    at = np.arange(n)  # the pixels whose chain is still going
    inside, ior_1 = np.zeros(n, bool), np.ones(n)
    own, own_p, own_n = np.full(n, -1), np.zeros((n, 3)), np.zeros((n, 3))
    levels, first_hit = [], None
    for _ in range(max_depth + 1):
        lv = dict(branch=np.full(n, NONE), local=np.zeros((n, 3)), weight=np.zeros(n), margin=np.full(n, np.inf),
                  lit=np.zeros(n, int), shadowed=np.zeros(n, int))
        levels.append(lv)
        if not len(at):
            continue
        idx, t, margin = closest(objects, o, d, own, own_p, own_n)
        if first_hit is None:
            first_hit = idx.copy()
        lv["branch"][at] = np.where(idx < 0, MISS, OPAQUE)
        lv["margin"][at] = margin
        h = idx >= 0  # from here on: the rays that hit
        at, idx, o, d, inside, ior_1, margin = at[h], idx[h], o[h], d[h], inside[h], ior_1[h], margin[h]
        if not len(at):
            continue
        p = o + t[h, None] * d
        n0, m0 = normals(objects, idx, p)
        s = p + OFFSET * n0
        nrm, m1 = normals(objects, idx, s)
        margin = np.minimum(np.minimum(margin, _off_the_box(objects, idx, s)), np.minimum(m0, m1))
        mat = mats[scene["material"][idx]]
        cd, kd, cs, ks, shine, tr, ior = mat[:, 0:3], mat[:, 3], mat[:, 4:7], mat[:, 7], mat[:, 8], mat[:, 9], mat[:, 10]
        local = np.zeros((len(at), 3))
        lit, shadowed = np.zeros(len(at), int), np.zeros(len(at), int)
        out = np.nonzero(~inside)[0]
        for light in lights if len(out) else []:
            l = light[:3] - s[out]
            l = l / np.sqrt(_dot(l, l))[:, None]
            occ, m_f = occluded(objects, s[out], l, idx[out], p[out], nrm[out])
            b = l - d[out]
            with np.errstate(all="ignore"):
                b = b / np.sqrt(_dot(b, b))[:, None]
            diff = np.maximum(0.0, _dot(nrm[out], l))
            spec = np.nan_to_num(np.maximum(0.0, _dot(nrm[out], b))) ** shine[out]
            term = (kd[out] * diff)[:, None] * cd[out] * light[3:] + (ks[out] * spec)[:, None] * cs[out] * light[3:]
            local[out] += np.where(occ[:, None], 0.0, term)
            matters = term.max(-1) > 1e-7  # a feeler whose light adds nothing either way decides nothing
            margin[out] = np.minimum(margin[out], np.where(matters, m_f, np.inf))
            lit[out] += ~occ & matters
            shadowed[out] += occ & matters
        lv["local"][at], lv["lit"][at], lv["shadowed"][at] = local, lit, shadowed
        # the ray of the next level
        glass = tr != 0
        nf = np.where(inside[:, None], -nrm, nrm)  # the normal that faces the ray
        ratio = np.where(inside, ior_1, ior_1 / ior)
        cos_i = -_dot(d, nf)
        tang = d + cos_i[:, None] * nf             # the part of d along the surface
        k = 1 - ratio * ratio * _dot(tang, tang)   # 1 - sin^2 of the refracted angle
        refr = ratio[:, None] * tang - np.sqrt(np.maximum(k, 0.0))[:, None] * nf
        refr = refr / np.sqrt(_dot(refr, refr))[:, None]
        refl = d - 2 * _dot(d, nrm)[:, None] * nrm
        refl = refl / np.sqrt(_dot(refl, refl))[:, None]
        branch = np.where(glass, np.where(k < 0, TIR, np.where(inside, LEAVE, ENTER)), OPAQUE)
        margin = np.where(glass, np.minimum(margin, np.abs(k)), margin)
        weight = np.where(glass, np.where(k < 0, 0.0, 1.0), ks)
        lv["branch"][at], lv["weight"][at], lv["margin"][at] = branch, weight, margin
        go = weight > 0
        g = glass[go]
        d_next = np.where(g[:, None], refr[go], refl[go])
        o_next = np.where(g[:, None], p[go] + OFFSET * refr[go], s[go])
        own, own_p, own_n = idx[go], p[go], nrm[go]
        inside = np.where(g, ~inside[go], inside[go])
        ior_1 = np.where(g, np.where(inside, ior[go], 1.0), ior_1[go])
        at, o, d = at[go], o_next, d_next
    return dict(res=cam["res"], bclr=scene["bclr"], hit=first_hit, levels=levels)


def fold(chain, max_depth):
    """The frame of maximum depth `max_depth` from a chain at least that long -> dict(rgb (ry, rx, 3), hit (ry, rx), margin,
    free (every feeler of the chain free), has (BRANCHES name -> mask), levels (levels reached)), per pixel."""
    lv = chain["levels"][:max_depth + 1]
    assert len(lv) == max_depth + 1
    rx, ry = chain["res"]
    n = len(lv[0]["branch"])
    colour = np.zeros((n, 3))
    clamped = np.zeros(n, bool)
    for k in range(max_depth, -1, -1):
        L = lv[k]
        below = colour * L["weight"][:, None] if k < max_depth else 0.0
        raw = L["local"] + below
        if k >= 1:
            clamped = (clamped & (L["weight"] > 0)) | ((raw > 1).any(-1) & (L["branch"] > MISS))
        colour = np.where((L["branch"] == MISS)[:, None], chain["bclr"][None, :], np.clip(raw, 0.0, 1.0))
        colour = np.where((L["branch"] == NONE)[:, None], 0.0, colour)
    margin = np.min([L["margin"] for L in lv], axis=0)
    branch = np.stack([L["branch"] for L in lv])
    bounced = branch[:-1] if max_depth else branch[:0]  # the levels whose branch was followed
    has = {"lit": np.any([L["lit"] > 0 for L in lv], axis=0), "shadowed": np.any([L["shadowed"] > 0 for L in lv], axis=0),
           "opaque bounce": ((bounced == OPAQUE) & (np.stack([L["weight"] for L in lv])[:len(bounced)] > 0)).any(0),
           "enter": (bounced == ENTER).any(0), "leave": (bounced == LEAVE).any(0), "TIR": (bounced == TIR).any(0),
           "miss after a bounce": (branch[1:] == MISS).any(0), "inner-level clamp": clamped}
    shape = lambda a: a.reshape(ry, rx, *a.shape[1:])
    return dict(rgb=shape(colour), hit=shape(chain["hit"]), margin=shape(margin), free=shape(~has["shadowed"]),
                has={k: shape(v) for k, v in has.items()}, levels=shape((branch != NONE).sum(0)))


# ---- comparing an implementation with the model -------------------------------------------------------------------------------------

def well_conditioned(frame, what):
    """The mask of the pixels to compare; asserts the 15 % cap on the rest -> (mask, share left out)"""
    ok = frame["margin"] >= THRESHOLD
    share = float((~ok).mean())
    assert share <= MAX_LEFT_OUT, "%s: %.1f %% of the pixels are ill-conditioned, over the %g %% cap" % (what, 100 * share, 100 * MAX_LEFT_OUT)
    return ok, share


def check_frame(frame, rgb, hit, max_depth, what, lossy_any_hit=False):
    """An implementation's frame against the model's: on well-conditioned pixels the primary hit ID is equal and every colour
    component within TOL.  lossy_any_hit (a BVH: its any-hit can lose an occluder, never invent one): that holds where the
    model finds every feeler of the chain free; elsewhere every component is at least the model's minus TOL - every weight of
    the chain is non-negative and the clamp is monotone.  -> (largest two-sided error, share left out)"""
    ok, share = well_conditioned(frame, what)
    rgb, hit = np.asarray(rgb, np.float64), np.asarray(hit)
    tol = TOL["depth0" if max_depth == 0 else "deeper"]
    wrong = ok & (hit != frame["hit"])
    assert not wrong.any(), "%s: %d primary hit IDs differ from the model's, first at pixel %s" % (what, int(wrong.sum()), np.argwhere(wrong)[0].tolist())
    diff = rgb - frame["rgb"]
    both = ok & frame["free"] if lossy_any_hit else ok
    err = float(np.abs(diff[both]).max())
    low = float(-diff[ok & ~both].min()) if (ok & ~both).any() else 0.0
    print("%s: %.1f %% left out, %d pixels compared, max |colour - model| %.3g (tolerance %.3g)%s" % (
        what, 100 * share, int(both.sum()), err, tol, ", %d pixels held from below, lowest %.3g under the model" % (int((ok & ~both).sum()), low) if lossy_any_hit else ""))
    worst = np.unravel_index(np.argmax(np.where(both[..., None], np.abs(diff), 0.0)), diff.shape)
    assert err <= tol, "%s: colour off by %g at pixel (row %d, column %d), tolerance %g" % (what, err, worst[0], worst[1], tol)
    assert low <= tol, "%s: a colour is %g under the model's where only an occluder can have been lost, tolerance %g" % (what, low, tol)
    return err, share


def branch_counts(frames):
    """BRANCHES name -> the number of well-conditioned pixels over `frames` (fold() results) whose chain has it"""
    return {b: int(sum((f["has"][b] & (f["margin"] >= THRESHOLD)).sum() for f in frames)) for b in BRANCHES}


def check_coverage(frames, what):
    counts = branch_counts(frames)
    print("%s: well-conditioned pixels per branch: %s" % (what, counts))
    short = {b: c for b, c in counts.items() if c < MIN_BRANCH_PIXELS}
    assert not short, "%s: branches seen in fewer than %d well-conditioned pixels: %s" % (what, MIN_BRANCH_PIXELS, short)
    return counts


# ---- the scenes -------------------------------------------------------------------------------------------------------------------
# Near cameras, objects that fill the frame, two or three lights whose colours add up to more than 1 (so that lit surfaces
# saturate the clamp, also where a mirror shows them).  Triangles face the camera and the lights with their normal's side.
# Materials: f  cd(3) Kd  cs(3) Ks  shine  T  ior  emission(3).

_VIEW = """bclr %s
v
from %s
at %s
up 0 1 0
angle %s
hither 0.01
resolution 64 64
aperture 0
focal 1
"""

# floor and back wall of two triangles each; a mirror, a glossy (shine 100) and a glass sphere; a matte cube (Ks = 0); a low light
# at (0.3, 3, -0.6) with a sphere ABOVE it: the floor around (0.3, 0, -0.6) is in that sphere's shadow only because feelers do
# not end at the light (Q5)
_STUDIO_BODY = """l 4 6 5 0.8 0.8 0.8
l -5 5 3 0.6 0.6 0.7
l 0.3 3 -0.6 0.6 0.5 0.4
f 0.9 0.9 0.8 0.9 1 1 1 0.15 20 0 1 0 0 0
p 3 -7 0 -5 -7 0 8 7 0 8
p 3 -7 0 -5 7 0 8 7 0 -5
f 0.7 0.5 0.4 0.8 1 1 1 0 1 0 1 0 0 0
p 3 -7 0 -5 7 0 -5 7 7 -5
p 3 -7 0 -5 7 7 -5 -7 7 -5
f 1 1 1 0.05 1 1 1 0.9 50 0 1 0 0 0
s -1.7 1.1 -1.2 1
f 0.9 0.2 0.2 0.7 1 1 1 0.5 100 0 1 0 0 0
s 1.6 0.8 0.2 0.7
f 0.9 0.9 1 0.05 1 1 1 0.4 60 0.9 1.5 0 0 0
s 0.1 0.95 2.2 0.8
f 0.3 0.8 0.3 0.9 1 1 1 0 1 0 1 0 0 0
box 0.2 0.02 -3 1.4 1.22 -1.8
f 0.8 0.8 0.2 0.8 1 1 1 0 1 0 1 0 0 0
s 0.3 5.5 -0.6 1
"""
STUDIO = _VIEW % ("0.2 0.3 0.5", "0 2.5 5.4", "0 0.9 0", "56") + _STUDIO_BODY

# a glass cube seen from a skew angle: rays that enter through one face and meet an adjacent one are reflected totally; behind
# it a matte sphere, a glossy sphere and a slanted triangle; a small matte cube in front
GLASSBOX = _VIEW % ("0.05 0.05 0.1", "4 3.2 5.5", "0 0.9 0", "40") + """l 6 7 2 0.9 0.9 0.9
l -4 6 6 0.7 0.7 0.6
f 0.8 0.8 0.9 0.8 1 1 1 0.3 100 0 1 0 0 0
p 3 -8 0 -8 -8 0 8 8 0 8
p 3 -8 0 -8 8 0 8 8 0 -8
f 1 1 1 0.02 1 1 1 0.3 80 0.95 1.5 0 0 0
box -1 0.05 -1 1 2.05 1
f 0.9 0.15 0.1 0.9 1 1 1 0 1 0 1 0 0 0
s -2.5 1.05 -2.5 1
f 0.2 0.3 0.9 0.7 1 1 1 0.5 100 0 1 0 0 0
s 1.2 0.85 -3 0.8
f 0.9 0.8 0.2 0.8 1 1 1 0.2 30 0 1 0 0 0
p 3 -5 0 -5 5 0 -5 0 5 -6
f 0.6 0.6 0.6 0.9 1 1 1 0 1 0 1 0 0 0
box 2 0.02 1 2.8 0.82 1.8
"""

# planes (accel None only, Q12): a floor and a back wall; the light at z = -2 reaches nothing in front of it, because its feelers
# go on to the wall plane behind it (Q5)
PLANES = _VIEW % ("0.3 0.4 0.6", "0.5 2.4 7", "0 0.8 0", "42") + """l 3 6 8 0.8 0.8 0.8
l -4 5 7 0.6 0.6 0.6
l 0 4 -2 0.5 0.5 0.5
f 0.8 0.8 0.8 0.9 1 1 1 0.2 30 0 1 0 0 0
pl 0 0 0 0 0 1 1 0 0
f 0.5 0.6 0.8 0.8 1 1 1 0 1 0 1 0 0 0
pl 0 0 -6 1 0 -6 0 1 -6
f 1 1 1 0.05 1 1 1 0.9 50 0 1 0 0 0
s -1.5 1.1 -0.5 1
f 0.9 0.9 1 0.05 1 1 1 0.4 60 0.9 1.5 0 0 0
s 1.2 0.9 1.5 0.8
f 0.8 0.3 0.2 0.9 1 1 1 0 1 0 1 0 0 0
box 1 0.02 -2.5 2.2 1.22 -1.3
f 1 1 1 0.02 1 1 1 0.3 80 0.95 1.5 0 0 0
box -0.6 0.05 2.4 0.2 0.85 3.2
"""


def _hall():
    """Too big for LDS (a floor of 12 x 12 x 2 triangles): the kernels traverse it from L2, and per-level launches take it.
    A ring of mirror, glossy and matte spheres around a glass sphere and a glass cube (Ks = 0: no zero-weight reflection rays,
    which per-level launches refuse under the literal stack)."""
    out = [_VIEW % ("0.2 0.3 0.5", "0.4 4.2 4.6", "0 0.5 -0.4", "60"), "l 5 7 6 0.8 0.8 0.8\nl -6 6 2 0.6 0.6 0.7\nl 0.5 4 -3 0.5 0.5 0.4\n",
           "f 0.9 0.9 0.8 0.9 1 1 1 0.15 20 0 1 0 0 0\n"]
    for i in range(-6, 6):
        for k in range(-6, 6):
            out.append("p 3 %d 0 %d %d 0 %d %d 0 %d\np 3 %d 0 %d %d 0 %d %d 0 %d\n" % (i, k, i, k + 1, i + 1, k + 1, i, k, i + 1, k + 1, i + 1, k))
    mats = ["f 1 1 1 0.05 1 1 1 0.9 50 0 1 0 0 0\n", "f 0.9 0.2 0.2 0.7 1 1 1 0.5 100 0 1 0 0 0\n", "f 0.2 0.7 0.3 0.9 1 1 1 0 1 0 1 0 0 0\n"]
    for j in range(4):
        a = 2 * np.pi * j / 4 + 0.5
        out.append(mats[j % 3] + "s %.3f 1.05 %.3f 1\n" % (3.3 * np.cos(a) + 0.013, 3.3 * np.sin(a) - 0.4 + 0.007))
    out.append("f 0.9 0.9 1 0.1 1 1 1 0 1 0.9 1.5 0 0 0\ns -0.9 1.05 0.2 1\n")
    out.append("f 1 1 1 0.1 1 1 1 0 1 0.95 1.5 0 0 0\nbox 0.5 0.05 -1.5 1.9 1.45 -0.1\n")
    out.append("f 0.8 0.8 0.2 0.8 1 1 1 0 1 0 1 0 0 0\ns 0.5 6.5 -3 1\n")
    return "".join(out)


HALL = _hall()
HALL_FIRST_SPHERE = 288  # four ring spheres, the glass sphere, the glass cube, the sphere above the low light
SCENES = dict(studio=STUDIO, glassbox=GLASSBOX, hall=HALL, planes=PLANES)
NO_PLANES = ("studio", "glassbox", "hall")  # every back end; `planes` goes through accel None only (Q12)
DEPTHS = (0, 1, 2, 4)
SECOND_VIEW = dict(from_=(-3.5, 2.5, 3.5), at=(0.25, 0.75, -0.5), up=(0, 1, 0), angle=56.0)  # of studio, for set_camera
STUDIO_SECOND_VIEW = _VIEW % ("0.2 0.3 0.5", "-3.5 2.5 3.5", "0.25 0.75 -0.5", "56") + _STUDIO_BODY  # the same, as a file


def write_scenes(tmp):
    """name -> path of the scene files written under `tmp`"""
    import os
    paths = {}
    for name, text in SCENES.items():
        paths[name] = os.path.join(str(tmp), name + ".p3f")
        with open(paths[name], "w") as f:
            f.write(text)
    return paths


def with_resolution(cam, res):
    return dict(cam, res=(int(res[0]), int(res[1])))


# ---- moved geometry -----------------------------------------------------------------------------------------------------------------

def moved(objects, ranges, xforms, sphere_scale=None):
    """The objects after DeviceScene.transform_prims(ranges, xforms, sphere_scale=...), in float64 from the same float32
    numbers: a point goes to M p + t; the vertices of a triangle, the centre of a sphere (radius x sphere_scale) and min and
    max of a box are points.  -> a new list; objects outside the ranges are shared."""
    m = np.asarray(xforms, np.float32).astype(np.float64).reshape(-1, 3, 4)
    sc = np.ones(len(m)) if sphere_scale is None else np.asarray(sphere_scale, np.float32).astype(np.float64)
    out = list(objects)
    for first, count, x in ranges:
        pt = lambda p: m[x][:, :3] @ p + m[x][:, 3]
        for i in range(first, first + count):
            ob = dict(objects[i])
            if ob["kind"] == geo.SPHERE:
                ob["c"], ob["r"] = pt(ob["c"]), ob["r"] * sc[x]
            elif ob["kind"] == geo.TRIANGLE:
                ob["p0"], ob["p1"], ob["p2"] = pt(ob["p0"]), pt(ob["p1"]), pt(ob["p2"])
            elif ob["kind"] == geo.BOX:
                ob["mn"], ob["mx"] = pt(ob["mn"]), pt(ob["mx"])
            else:
                raise ValueError("planes do not move")
            out[i] = ob
    return out


def rigid(axis, degrees, pivot, shift):
    """(3, 4) float32: a rotation about `axis` through `pivot`, then a translation"""
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    rot = np.eye(3) + s * k + (1 - c) * (k @ k)
    pivot = np.asarray(pivot, np.float64)
    return np.concatenate([rot, (pivot - rot @ pivot + np.asarray(shift, np.float64))[:, None]], axis=1).astype(np.float32)


def scale(factors, shift):
    """(3, 4) float32: a positive scale per axis, then a translation (what a box takes)"""
    return np.concatenate([np.diag(np.asarray(factors, np.float64)), np.asarray(shift, np.float64)[:, None]], axis=1).astype(np.float32)


# the move of the update tests, on studio: the three spheres turn about a vertical axis, rise a little and grow; the back wall
# is stretched and the cube squeezed, each by another factor per axis (the cube stops being a cube: its shading points near
# the long sides' ends now get the normal of the wrong axis, which the margins leave out)
STUDIO_MOVE = dict(ranges=[(4, 3, 0), (2, 2, 1), (7, 1, 2)],
                   xforms=np.stack([rigid((0, 1, 0), 25.0, (0, 0, 0.5), (0.1, 0.15, -0.2)), scale((1.1, 0.9, 1.0), (0.3, 0.0, 0.0)),
                                    scale((1.2, 0.8, 1.1), (-0.2, 0.01, 0.3))]),
                   sphere_scale=np.array([1.1, 1.0, 1.0], np.float32))


def geometry_rows(objects, ids):
    """The nine geometry floats of objects `ids` as HostScene.set_geometry and write_moved_p3f take them, rounded to float32"""
    rows = np.zeros((len(ids), 9), np.float32)
    for row, i in zip(rows, ids):
        ob = objects[i]
        v = {geo.SPHERE: lambda: np.r_[ob["c"], ob["r"]], geo.BOX: lambda: np.r_[ob["mn"], ob["mx"]]}.get(
            ob["kind"], lambda: np.r_[ob["p0"], ob["p1"], ob["p2"]])()
        row[:len(v)] = v
    return rows
