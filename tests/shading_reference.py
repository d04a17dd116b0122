"""A float64 model of the Whitted shading chain (rayTracing, main.cpp:92-309), built on the geometric model of
intersect_reference.py and stated in formulas of its own, so that a misreading shared by the kernels and the CPU oracle cannot
hide behind their bit parity.  Plain numpy, vectorised over pixels, one batch per chain level.

The configuration: debug_view = 0; either antialiasing = 0 (one ray through each pixel centre, no lens, no skybox, hard
shadows) or, with a sampler(), the mean over a pixel's spp x spp samples, stated under SAMPLES below.

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

SAMPLES.  Sample s = i spp + j (i, j in 0 .. spp - 1) of pixel (x, y) of a frame rx wide has a stream of draws of its own, seeded
with (the frame's seed, pixel index y rx + x - of the whole frame, also in a tile of it -, s): rng_reference restates its integers
n.  A draw is an input of the model, like a scene's float32 numbers: a = float32(n) / 2^31, or e = n / (2^31 - 1) where the
kernels draw a double (the tent filter); everything from there is float64.  The draws of a sample, in order:

  position  jitter: (x + (i + a1) / spp, y + (j + a2) / spp): cell (i, j) of the pixel's spp x spp cells.  tent: with r = 2 e and
            t(r) = sqrt(r) - 1 for r < 1, 1 - sqrt(2 - r) otherwise: (x + (.5 + t(r1)) / spp, y + (.5 + t(r2)) / spp) - every sample
            around the first cell's centre, whatever (i, j).  The ray goes through that position of the image plane as `primary`
            says for x + .5, y + .5.
  lens      (only with one) P = |at - from|; the ray starts at from + A (lx r + ly v), A = aperture x the width of a pixel on the
            image plane at distance P (2 P tan(angle / 2) / ry), and goes towards from + focal P (f + the position's r and v
            terms): every lens point sees the position's point of the plane in focus.  square: (lx, ly) = ((i + a3) / spp,
            (j + a4) / spp), the quadrant [0, 1)^2, not centred.  disk: pairs of draws, the FIRST of a pair 2 a - 1 = ly, the second
            lx, until lx^2 + ly^2 < 1.
  lights    soft shadows: at every shading point OUTSIDE an object, at every level of the chain (the last too), every light in
            scene order takes two draws, the first jy, the second jx, and is sampled at L + side ((i + jx) / spp, (j + jy) / spp, 0):
            cell (i, j) of a square in the xy plane with its corner at the light.  A shading point inside glass draws nothing.
            The zero-weight reflection rays of glass (Q3) are traced after the chain has ended and do not touch its draws.
  skybox    a miss - primary, after a bounce or after a refraction - along d (as it is, any length) takes the face of the largest
            |component| of d (x over y and z over both only when strictly larger), faces in the order -x +x +y -y +z -z; with m that
            component's size, (u, v) = (sign(dx) dz, dy) on an x face, (-dx, -sign(dy) dz) on a y face, (-sign(dz) dx, dy) on a
            z face; s = (u / m + 1) / 2, t likewise; the texel is column floor((w - 1) s), row floor((h - 1) t) from the bottom,
            and the colour its bytes / 255.99, unclamped.
  pixel     the float64 mean of its samples' chain colours; after k samples of an accumulator, of the first k.  The hit ID is
            the first sample's.  fold() works per sample, so one trace serves every smaller depth and every k.

A sample inherits the smallest margin along its chain, a pixel the smallest of its samples': a pixel is ill-conditioned when any
of its samples is.  Three decisions of the sampled modes get margins, compared with THRESHOLD as they are: |lx^2 + ly^2 - 1| of
every pair the disk draws (a flipped rejection would shift every later draw of the stream: such a sample is left out, not
compared loosely); |r - 1| at the tent's branch; at a skybox miss (m - the second largest |component|) / m and the distance of
(w - 1) s and (h - 1) t from the nearest integer.

Deliberately NOT stated here: the path tracer (its roulette and glass choice are random decisions, not a chain); soft shadows
without anti-aliasing (replicated lights); Q1 / Q2 (the BVH's any-hit can
lose an occluder, depending on the tree's shape and the stack's history: frames over a BVH are held to the model where the model
finds every feeler free, and from below elsewhere); Q8's ulps (directions here are exact unit vectors)."""
import numpy as np

import intersect_reference as geo
import rng_reference as rng

THRESHOLD = geo.THRESHOLD
MAX_LEFT_OUT = 0.15  # the share of a frame's pixels that may be ill-conditioned
GRAZE = 0.05         # |N.dir| under which a ray leaving a surface is taken to graze it
OFFSET = 1e-4
MIN_BRANCH_PIXELS = 50

MISS, OPAQUE, ENTER, LEAVE, TIR = 0, 1, 2, 3, 4  # the branch of a chain level; NONE: the chain has ended above
NONE = -1
BRANCHES = ("lit", "shadowed", "opaque bounce", "enter", "leave", "TIR", "miss after a bounce", "inner-level clamp",
            # of the sampled modes: counted in chains (samples), `penumbra` in pixels
            "penumbra", "inside glass, no soft-shadow draws", "disk sample after a rejection", "tent, lower branch", "tent, upper branch",
            "skybox face 0", "skybox face 1", "skybox face 2", "skybox face 3", "skybox face 4", "skybox face 5",
            "skybox after a bounce", "skybox after a refraction")

# Measured: the largest |oracle - model| of a colour component over the well-conditioned pixels of the fixed frames of
# test_shading_reference.py (CPU oracle, accel None, grid and - where the model finds every feeler free - BVH), for frames of
# maximum depth 0 and for deeper ones.  The asserted tolerance is 4 x the measured maximum: room for another compiler's
# contraction choices and for moved float32 geometry, not for another formula.
MEASURED = {"depth0": 1.8e-5, "deeper": 8.6e-5,  # on the CPU oracle (x86-64, g++ -O2); the largest are glossy highlights, shine 100
            # the sampled modes and those with the skybox on, every depth, same platform: 7.63e-5 and 7.31e-5, both at one pixel of
            # calm at depth 4, one of whose nine samples is off by 6.6e-4: it leaves the mirror sphere near its rim, crosses the
            # glass ball and lands on the floor - two curved surfaces widen the float32 noise of its direction, and the floor's
            # shading turns the moved point into colour.  Every frame of depth <= 2 is within 2e-5.
            "sampled": 7.7e-5, "skybox": 7.4e-5}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}


# ---- the scene file ---------------------------------------------------------------------------------------------------------------

def load_scene(path):
    """-> dict(objects, material (index per object), materials (n, 14: cd Kd cs Ks shine T ior em), lights (n, 6: position,
    colour), bclr, camera(from_, at, up, angle, res, aperture, focal)), every number the float32 a loader reads, held in float64."""
    with open(path) as f:
        tok = [w for line in f for w in line.split("#")[0].split()]
    f32 = lambda ws: np.array([np.float32(w) for w in ws], np.float32).astype(np.float64)
    skip = {"s": 4, "p": 10, "box": 6, "pl": 9, "hither": 1, "v": 0, "env": 1}
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
        elif w in ("angle", "aperture", "focal"):
            cam[w] = float(np.float32(tok[i])); i += 1
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


def camera(from_, at, up, angle, res, aperture=0.0, focal=1.0):
    """A camera for trace(): the numbers of a `v` block, rounded to float32 as a loader or look_at takes them"""
    r32 = lambda v: np.asarray(v, np.float32).astype(np.float64)
    return dict(from_=r32(from_), at=r32(at), up=r32(up), angle=float(np.float32(angle)), res=(int(res[0]), int(res[1])),
                aperture=float(np.float32(aperture)), focal=float(np.float32(focal)))


def _window(cam):
    """(x0, y0, w, h): the pixels a chain covers, the whole frame unless the camera has a `window`"""
    return cam.get("window") or (0, 0) + tuple(cam["res"])


def camera_rays(cam, px, py, lens=None):
    """The rays through the image positions (px, py), in pixels from the bottom left corner -> (origins, unit directions).
    lens = (lx, ly): from the lens point of those coordinates towards the position's point of the plane in focus."""
    rx, ry = cam["res"]
    f = cam["at"] - cam["from_"]
    dist = np.sqrt(f @ f)
    f = f / dist
    r = np.cross(cam["up"], -f)
    r = r / np.sqrt(r @ r)
    v = np.cross(-f, r)
    half = np.tan(np.radians(cam["angle"]) / 2)
    sx = (2 * px / rx - 1) * half * rx / ry
    sy = (2 * py / ry - 1) * half
    d = f[None, :] + sx[:, None] * r[None, :] + sy[:, None] * v[None, :]
    o = np.broadcast_to(cam["from_"], d.shape).copy()
    if lens is not None:
        width = cam.get("aperture", 0.0) * 2 * dist * half / ry  # the lens coordinates' unit: `aperture` pixel widths of the image plane
        o = o + width * (lens[0][:, None] * r[None, :] + lens[1][:, None] * v[None, :])
        d = cam["from_"][None, :] + cam.get("focal", 1.0) * dist * d - o
    return o, d / np.sqrt((d * d).sum(-1))[:, None]


def primary_rays(cam):
    """One ray through each pixel centre -> (origins, unit directions), (ry * rx, 3), row 0 at the bottom"""
    x0, y0, w, h = _window(cam)
    y, x = np.mgrid[y0:y0 + h, x0:x0 + w]
    return camera_rays(cam, x.reshape(-1) + 0.5, y.reshape(-1) + 0.5)


# ---- the samples of a pixel -----------------------------------------------------------------------------------------------------------

def sampler(spp, tent=False, lens=None, light_side=None, skybox=None, seed=0):
    """What trace() needs to know of an anti-aliased configuration: spp x spp samples a pixel; tent: the tent filter, else
    jitter; lens: None, "square" or "disk"; light_side: the side of the soft-shadow square, None = hard shadows; skybox: six
    faces (skybox_faces()) or None = the background colour; seed: the frame's."""
    assert lens in (None, "square", "disk")
    return dict(spp=int(spp), tent=bool(tent), lens=lens, light_side=None if light_side is None else float(np.float32(light_side)),
                skybox=skybox, seed=int(seed))


class _Draws:
    """One stream per ray; rand(at) and erand(at) draw once for the rays `at` and give the number the kernels make of it"""
    def __init__(self, seed, pixel, sample):
        self.state, self.inc = rng.seed_stream_v(seed, pixel, sample)

    def _next(self, at):
        self.state[at], n = rng.next31_v(self.state[at], self.inc[at])
        return n

    def rand(self, at):
        return (self._next(at).astype(np.float32) / np.float32(2.0 ** 31)).astype(np.float64)

    def erand(self, at):
        return self._next(at) / (2.0 ** 31 - 1)


def sample_rays(cam, smp):
    """The primary rays of every (pixel, sample), pixel-major, sample s = i * spp + j -> dict(o, d, draws, i, j, margin,
    retries (rejected disk pairs), tent_low, tent_high (a tent draw took that branch))."""
    x0, y0, w, h = _window(cam)
    n_s = smp["spp"]
    y, x, i, j = [a.reshape(-1) for a in np.mgrid[y0:y0 + h, x0:x0 + w, 0:n_s, 0:n_s]]
    n = len(x)
    every = np.arange(n)
    draws = _Draws(smp["seed"], y * cam["res"][0] + x, i * n_s + j)
    margin, retries = np.full(n, np.inf), np.zeros(n, int)
    low, high = np.zeros(n, bool), np.zeros(n, bool)
    if smp["tent"]:
        pos = []
        for _ in range(2):
            r = 2 * draws.erand(every)
            margin = np.minimum(margin, np.abs(r - 1))
            low, high = low | (r < 1), high | (r >= 1)
            pos.append(np.where(r < 1, np.sqrt(r) - 1, 1 - np.sqrt(np.maximum(2 - r, 0.0))))
        px, py = x + (0.5 + pos[0]) / n_s, y + (0.5 + pos[1]) / n_s
    else:
        px = x + (i + draws.rand(every)) / n_s
        py = y + (j + draws.rand(every)) / n_s
    lens = None
    if smp["lens"] == "square":
        lx = (i + draws.rand(every)) / n_s
        lens = (lx, (j + draws.rand(every)) / n_s)
    elif smp["lens"] == "disk":
        lx, ly, todo = np.zeros(n), np.zeros(n), every
        while len(todo):
            b = 2 * draws.rand(todo) - 1
            a = 2 * draws.rand(todo) - 1
            r2 = a * a + b * b
            margin[todo] = np.minimum(margin[todo], np.abs(r2 - 1))
            lx[todo], ly[todo] = a, b
            retries[todo] += r2 >= 1
            todo = todo[r2 >= 1]
        lens = (lx, ly)
    o, d = camera_rays(cam, px, py, lens)
    return dict(o=o, d=d, draws=draws, i=i, j=j, margin=margin, retries=retries, tent_low=low, tent_high=high)


# ---- the skybox -------------------------------------------------------------------------------------------------------------------------

def skybox_faces():
    """A cubemap for the tests: six faces of different sizes (one of them RGBA), row 0 the bottom row, in the order
    -x +x +y -y +z -z; no two neighbouring texels and no two faces alike, neighbours at least 20 / 255 apart in a channel."""
    faces = []
    for k, (w, h, bpp) in enumerate([(24, 24, 3), (32, 16, 3), (11, 19, 4), (24, 24, 3), (40, 8, 3), (17, 17, 3)]):
        y, x = np.mgrid[0:h, 0:w]
        f = np.full((h, w, bpp), 255, np.uint8)
        f[..., 0] = (x * 37 + 11 * k) % 256
        f[..., 1] = (y * 53 + 29 * k) % 256
        f[..., 2] = (x * 71 + y * 113 + 40 * k) % 256
        faces.append(f)
    return faces


def skybox_lookup(faces, d):
    """The colour of the cubemap along d (any length) -> (colours, face, margin)"""
    a = np.abs(d)
    axis = np.where(a[:, 2] > np.maximum(a[:, 0], a[:, 1]), 2, np.where(a[:, 0] > a[:, 1], 0, 1))
    k = np.arange(len(d))
    m = a[k, axis]
    positive = d[k, axis] >= 0
    face = np.where(axis == 0, np.where(positive, 1, 0), np.where(axis == 1, np.where(positive, 2, 3), np.where(positive, 4, 5)))
    sign = np.where(positive, 1.0, -1.0)
    u = np.where(axis == 0, sign * d[:, 2], np.where(axis == 1, -d[:, 0], -sign * d[:, 0]))
    v = np.where(axis == 1, -sign * d[:, 2], d[:, 1])
    with np.errstate(all="ignore"):
        s, t = (u / m + 1) / 2, (v / m + 1) / 2
        second = np.sort(a, axis=-1)[:, 1]
        margin = np.nan_to_num((m - second) / m, nan=0.0)
    colour = np.zeros((len(d), 3))
    for f, at in _groups(face):
        h, w = faces[f].shape[:2]
        cs, ct = (w - 1) * s[at], (h - 1) * t[at]
        col, row = np.clip(np.floor(cs), 0, w - 1).astype(int), np.clip(np.floor(ct), 0, h - 1).astype(int)
        colour[at] = faces[f][row, col, :3] / np.float64(np.float32(255.99))
        edge = np.minimum(np.abs(cs - np.round(cs)), np.abs(ct - np.round(ct)))
        margin[at] = np.minimum(margin[at], edge)
    return colour, face, margin


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

def trace(scene, objects=None, cam=None, max_depth=4, smp=None):
    """Follows every chain for max_depth + 1 levels: one chain per pixel, or with smp (a sampler()) one per (pixel, sample)
    -> dict(res, samples (chains per pixel), bclr, hit (primary hit IDs), levels: a list of dicts of per-chain arrays: branch,
    local (the unclamped local term), weight (of the level below), margin, lit, shadowed, inside (a shading point inside an
    object), sky (the colour of a miss), face (its cubemap face or -1); level 0 also lit_by and shadowed_by, per light)."""
    objects = scene["objects"] if objects is None else objects
    cam = scene["camera"] if cam is None else cam
    mats, lights = scene["materials"], scene["lights"]
    first = sample_rays(cam, smp) if smp else None
    o, d = (first["o"], first["d"]) if smp else primary_rays(cam)
    soft = smp["light_side"] if smp else None
    faces = smp["skybox"] if smp else None
    n = len(o)
    at = np.arange(n)  # the pixels whose chain is still going
    inside, ior_1 = np.zeros(n, bool), np.ones(n)
    own, own_p, own_n = np.full(n, -1), np.zeros((n, 3)), np.zeros((n, 3))
    levels, first_hit = [], None
    for _ in range(max_depth + 1):
        lv = dict(branch=np.full(n, NONE), local=np.zeros((n, 3)), weight=np.zeros(n), margin=np.full(n, np.inf),
                  lit=np.zeros(n, int), shadowed=np.zeros(n, int), inside=np.zeros(n, bool),
                  sky=np.broadcast_to(scene["bclr"], (n, 3)).copy(), face=np.full(n, -1))
        if not levels:
            lv.update(lit_by=np.zeros((n, len(lights)), bool), shadowed_by=np.zeros((n, len(lights)), bool))
            if smp:
                lv["margin"] = first["margin"].copy()
        levels.append(lv)
        if not len(at):
            continue
        idx, t, margin = closest(objects, o, d, own, own_p, own_n)
        if first_hit is None:
            first_hit = idx.copy()
        lv["branch"][at] = np.where(idx < 0, MISS, OPAQUE)
        lv["margin"][at] = np.minimum(lv["margin"][at], margin)
        if faces is not None and (idx < 0).any():
            gone = idx < 0
            lv["sky"][at[gone]], lv["face"][at[gone]], m_sky = skybox_lookup(faces, d[gone])
            lv["margin"][at[gone]] = np.minimum(lv["margin"][at[gone]], m_sky)
        h = idx >= 0  # from here on: the rays that hit
        at, idx, o, d, inside, ior_1 = at[h], idx[h], o[h], d[h], inside[h], ior_1[h]
        margin = lv["margin"][at]
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
        lv["inside"][at] = inside
        out = np.nonzero(~inside)[0]
        for li, light in enumerate(lights) if len(out) else []:
            pos = light[None, :3]
            if soft is not None:  # the first draw moves the sample along y, the second along x
                jy = first["draws"].rand(at[out])
                jx = first["draws"].rand(at[out])
                shift = np.stack([first["i"][at[out]] + jx, first["j"][at[out]] + jy, 0 * jx], axis=-1)
                pos = pos + soft * shift / smp["spp"]
            l = pos - s[out]
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
            if len(levels) == 1:
                lv["lit_by"][at[out], li], lv["shadowed_by"][at[out], li] = ~occ & matters, occ & matters
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
    chain = dict(res=_window(cam)[2:], samples=smp["spp"] ** 2 if smp else 1, bclr=scene["bclr"], hit=first_hit, levels=levels, smp=smp)
    if smp:
        chain.update(retries=first["retries"], tent_low=first["tent_low"], tent_high=first["tent_high"])
    return chain


def fold(chain, max_depth, samples=None):
    """The frame of maximum depth `max_depth` from a chain at least that long -> dict(rgb (ry, rx, 3), hit (ry, rx), margin,
    free (every feeler free), has (BRANCHES name -> the number of the pixel's chains that have it), levels (levels reached)),
    per pixel: the mean colour, the smallest margin and the largest level count of the pixel's first `samples` chains (None:
    all of them), the hit ID of its first."""
    lv = chain["levels"][:max_depth + 1]
    assert len(lv) == max_depth + 1
    rx, ry = chain["res"]
    per, smp = chain["samples"], chain["smp"]
    use = per if samples is None else samples
    assert 1 <= use <= per
    n = len(lv[0]["branch"])
    colour = np.zeros((n, 3))
    clamped = np.zeros(n, bool)
    for k in range(max_depth, -1, -1):
        L = lv[k]
        below = colour * L["weight"][:, None] if k < max_depth else 0.0
        raw = L["local"] + below
        if k >= 1:
            clamped = (clamped & (L["weight"] > 0)) | ((raw > 1).any(-1) & (L["branch"] > MISS))
        colour = np.where((L["branch"] == MISS)[:, None], L["sky"], np.clip(raw, 0.0, 1.0))
        colour = np.where((L["branch"] == NONE)[:, None], 0.0, colour)
    margin = np.min([L["margin"] for L in lv], axis=0)
    branch = np.stack([L["branch"] for L in lv])
    bounced = branch[:-1] if max_depth else branch[:0]  # the levels whose branch was followed
    has = {"lit": np.any([L["lit"] > 0 for L in lv], axis=0), "shadowed": np.any([L["shadowed"] > 0 for L in lv], axis=0),
           "opaque bounce": ((bounced == OPAQUE) & (np.stack([L["weight"] for L in lv])[:len(bounced)] > 0)).any(0),
           "enter": (bounced == ENTER).any(0), "leave": (bounced == LEAVE).any(0), "TIR": (bounced == TIR).any(0),
           "miss after a bounce": (branch[1:] == MISS).any(0), "inner-level clamp": clamped}
    none = np.zeros(n, bool)
    face = np.max([L["face"] for L in lv], axis=0)  # a chain misses once
    after = lambda kinds: (np.isin(branch[:-1], kinds) & (branch[1:] == MISS)).any(0) if max_depth else none
    has["inside glass, no soft-shadow draws"] = np.any([L["inside"] for L in lv], axis=0) if smp and smp["light_side"] is not None else none
    has["disk sample after a rejection"] = chain["retries"] > 0 if smp else none
    has["tent, lower branch"], has["tent, upper branch"] = (chain["tent_low"], chain["tent_high"]) if smp else (none, none)
    for f in range(6):
        has["skybox face %d" % f] = face == f
    has["skybox after a bounce"], has["skybox after a refraction"] = (after([OPAQUE]), after([ENTER, LEAVE])) if smp and smp["skybox"] is not None else (none, none)
    group = lambda a: a.reshape(ry * rx, per, *a.shape[1:])[:, :use]
    shape = lambda a: a.reshape(ry, rx, *a.shape[1:])
    counts = {k: shape(group(v).sum(1)) for k, v in has.items()}
    lit0, dark0 = group(lv[0]["lit_by"]).any(1), group(lv[0]["shadowed_by"]).any(1)
    counts["penumbra"] = shape((lit0 & dark0).any(-1).astype(int)) if smp and smp["light_side"] is not None else shape(np.zeros(ry * rx, int))
    return dict(rgb=shape(group(colour).mean(1)), hit=shape(group(chain["hit"])[:, 0]), margin=shape(group(margin).min(1)),
                free=shape(~group(has["shadowed"]).any(1)), has=counts, levels=shape(group((branch != NONE).sum(0)).max(1)))


# ---- comparing an implementation with the model -------------------------------------------------------------------------------------

def well_conditioned(frame, what):
    """The mask of the pixels to compare; asserts the 15 % cap on the rest -> (mask, share left out)"""
    ok = frame["margin"] >= THRESHOLD
    share = float((~ok).mean())
    assert share <= MAX_LEFT_OUT, "%s: %.1f %% of the pixels are ill-conditioned, over the %g %% cap" % (what, 100 * share, 100 * MAX_LEFT_OUT)
    return ok, share


def check_frame(frame, rgb, hit, max_depth, what, lossy_any_hit=False, kind=None):
    """An implementation's frame against the model's: on well-conditioned pixels the primary hit ID is equal and every colour
    component within TOL.  lossy_any_hit (a BVH: its any-hit can lose an occluder, never invent one): that holds where the
    model finds every feeler of the chain free; elsewhere every component is at least the model's minus TOL - every weight of
    the chain is non-negative and the clamp is monotone.  -> (largest two-sided error, share left out)"""
    ok, share = well_conditioned(frame, what)
    rgb, hit = np.asarray(rgb, np.float64), np.asarray(hit)
    tol = TOL[kind or ("depth0" if max_depth == 0 else "deeper")]  # kind: "sampled" or "skybox" (kind_of()) for a sampled chain's frame
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
    return {b: int(sum((f["has"][b] * (f["margin"] >= THRESHOLD)).sum() for f in frames)) for b in BRANCHES}


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


# the scenes of the sampled frames: few and large objects, so that few pixels have a sample near an edge (a pixel is left out when
# any of its samples is).  The floor is ONE triangle (no diagonal between two), its tip on the horizon; a tinted mirror sphere, a
# glass sphere (Ks = 0) and a matte cube, whose shadows on the floor have wide penumbrae under a light square of side 1.
_CALM_BODY = """l 1 5 7 0.8 0.8 0.8
l -5 5 3 0.6 0.6 0.7
f 0.9 0.6 0.3 0.5 1 1 1 0.6 50 0 1 0 0 0
s -1 0.7 0 0.7
f 0.9 0.9 1 0.1 1 1 1 0 1 0.9 1.5 0 0 0
s 1 0.55 0.8 0.55
"""
_CALM_FLOOR = """f 0.9 0.9 0.8 0.9 1 1 1 0 1 0 1 0 0 0
p 3 0 0 -60 -60 0 40 60 0 40
"""
_LENS_VIEW = _VIEW.replace("aperture 0", "aperture 2")  # a lens two pixels of the image plane wide, focused on `at`
CALM = _LENS_VIEW % ("0.2 0.3 0.5", "0 2.2 6", "0 0.9 0", "40") + _CALM_BODY + _CALM_FLOOR
# the same objects with nothing under them, seen from nearer: the mirror sphere shows every face of a cubemap
ADRIFT = _LENS_VIEW % ("0.2 0.3 0.5", "0 1.6 5", "0 0.9 0", "44") + _CALM_BODY
# calm with 288 small triangles under the floor, where no ray goes: too big for LDS, so the kernels traverse it from L2
CALM_BIG = CALM + "".join("p 3 %g -4 %g %g -4 %g %g -4 %g\np 3 %g -4 %g %g -4 %g %g -4 %g\n" % (
    i / 2, k / 2, i / 2, (k + 1) / 2, (i + 1) / 2, (k + 1) / 2, i / 2, k / 2, (i + 1) / 2, (k + 1) / 2, (i + 1) / 2, k / 2)
    for i in range(-6, 6) for k in range(-6, 6))
SAMPLED_SCENES = dict(calm=CALM, adrift=ADRIFT, calm_big=CALM_BIG)
BIG_RES, BIG_WINDOW = (96, 80), (13, 9, 43, 37)  # calm_big is rendered as this Tile of a 96 x 80 frame: no whole 4x4 or 8x8 tiles
SEED = 20240607
LIGHT_SIDE = 1.0


def sampled_modes():
    """name -> sampler() of the anti-aliased configurations held to the model (the skybox ones get their faces here)"""
    faces = skybox_faces()
    return {"jitter 2x2": sampler(2, seed=SEED), "jitter 3x3": sampler(3, seed=SEED), "tent": sampler(3, tent=True, seed=SEED),
            "soft shadows": sampler(3, light_side=LIGHT_SIDE, seed=SEED), "soft shadows 2x2": sampler(2, light_side=LIGHT_SIDE, seed=SEED),
            "lens square": sampler(3, lens="square", seed=SEED), "lens disk": sampler(3, lens="disk", seed=SEED),
            "tent with lens": sampler(2, tent=True, lens="disk", seed=SEED),
            "soft shadows with lens": sampler(2, lens="disk", light_side=LIGHT_SIDE, seed=SEED),
            "skybox": sampler(3, skybox=faces, seed=SEED), "skybox, one sample": sampler(1, skybox=faces, seed=SEED)}


SAMPLED_FRAMES = [("calm", m) for m in ("jitter 2x2", "jitter 3x3", "tent", "soft shadows", "lens square", "lens disk", "tent with lens",
                                         "soft shadows with lens", "skybox")] + [
    ("adrift", "skybox"), ("adrift", "skybox, one sample"), ("calm_big", "jitter 2x2"), ("calm_big", "soft shadows 2x2")]


def config_fields(smp):
    """The fields of a Whitted configuration (the oracle's or the library's: the names are the same) that select `smp`"""
    return dict(antialiasing=1, spp_sqrt=smp["spp"], sample_mode=1 if smp["tent"] else 0, depth_of_field=int(smp["lens"] is not None),
                sample_disk=int(smp["lens"] == "disk"), soft_shadows=int(smp["light_side"] is not None),
                light_side=smp["light_side"] or 0.0, skybox=int(smp["skybox"] is not None), seed=smp["seed"])


def sampled_camera(scene, name):
    """The camera trace() takes for a frame of SAMPLED_FRAMES over the loaded `scene`"""
    return with_window(with_resolution(scene["camera"], BIG_RES), *BIG_WINDOW) if name == "calm_big" else scene["camera"]


def kind_of(smp):
    """The key of MEASURED / TOL for a frame of `smp`"""
    return "skybox" if smp["skybox"] is not None else "sampled"

HALL = _hall()
HALL_FIRST_SPHERE = 288  # four ring spheres, the glass sphere, the glass cube, the sphere above the low light
SCENES = dict(studio=STUDIO, glassbox=GLASSBOX, hall=HALL, planes=PLANES)
NO_PLANES = ("studio", "glassbox", "hall")  # every back end; `planes` goes through accel None only (Q12)
DEPTHS = (0, 1, 2, 4)
SECOND_VIEW = dict(from_=(-3.5, 2.5, 3.5), at=(0.25, 0.75, -0.5), up=(0, 1, 0), angle=56.0)  # of studio, for set_camera
STUDIO_SECOND_VIEW = _VIEW % ("0.2 0.3 0.5", "-3.5 2.5 3.5", "0.25 0.75 -0.5", "56") + _STUDIO_BODY  # the same, as a file


def write_scenes(tmp, scenes=None):
    """name -> path of the scene files written under `tmp` (scenes: SCENES, or SAMPLED_SCENES)"""
    import os
    paths = {}
    for name, text in (SCENES if scenes is None else scenes).items():
        paths[name] = os.path.join(str(tmp), name + ".p3f")
        with open(paths[name], "w") as f:
            f.write(text)
    return paths


def with_resolution(cam, res):
    return dict(cam, res=(int(res[0]), int(res[1])))


def with_window(cam, x0, y0, w, h):
    """The camera of a chain over the pixels of Tile(x0, y0, w, h, ...) only"""
    return dict(cam, window=(int(x0), int(y0), int(w), int(h)))


def with_lens(cam, aperture, focal):
    """The camera after HostScene.set_lens(aperture, focal)"""
    return dict(cam, aperture=float(np.float32(aperture)), focal=float(np.float32(focal)))


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
