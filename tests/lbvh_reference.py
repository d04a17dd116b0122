"""A plain model of the device BVH builder (csrc/lbvh.hpp) and of the numbering p3d_scene_export_bvh gives its tree, written
from their description: DESIGN.md ("BVH builders", "Geometry updates"), the header comment of lbvh.hpp, Karras 2012.

The tree is a function of the object boxes alone.  Every object gets a 64-bit key: the 30-bit Morton code of its box centre
inside the bounds of all centres, and below it the object's index, which makes the keys unique.  Karras' hierarchy over the
sorted keys is their binary radix tree: a node is a range [lo, hi] of sorted keys, and it splits where the highest bit in
which keys[lo] and keys[hi] differ turns from 0 to 1.  That is how build() states it: no direction, no binary search for a
range's other end.  A range of two keys is emitted as one leaf of two objects, a single key as a leaf of one.

Also here: check_boxes (the invariants of any tree over a set of boxes), refit (the boxes of a tree recomputed from moved
object boxes) and writers for the synthetic .p3f scenes the tests of the builder use."""
import numpy as np

LEAF = 0x80000000
TREE_KEYS = ("bvh_bmin", "bvh_index", "bvh_bmax", "bvh_count_leaf", "bvh_order")


def _spread3(q):
    """Bit i of the 10-bit value q goes to bit 3 i"""
    q = q.astype(np.uint64)
    out = np.zeros_like(q)
    for i in range(10):
        out |= ((q >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i)
    return out


def quantised(bmin, bmax):
    """The cell of every box centre on the 1024^3 lattice over the bounds of the centres -> (n, 3) uint32.  Every step is one
    float32 operation."""
    lo, hi = np.asarray(bmin, np.float32).reshape(-1, 3), np.asarray(bmax, np.float32).reshape(-1, 3)
    c = (lo + hi) * np.float32(0.5)
    mn, mx = c.min(0), c.max(0)
    ext = mx - mn
    with np.errstate(divide="ignore", invalid="ignore"):
        u = np.where(ext > 0, (c - mn) / ext, np.float32(0)).astype(np.float32)
    u = np.minimum(np.maximum(u, np.float32(0)), np.float32(1))
    s = u * np.float32(1024)
    return np.where(s >= np.float32(1023), 1023, s.astype(np.int64)).astype(np.uint32)


def morton_codes(bmin, bmax):
    """30 bits, x in the highest bit of each triple"""
    q = quantised(bmin, bmax)
    return (_spread3(q[:, 0]) << np.uint64(2)) | (_spread3(q[:, 1]) << np.uint64(1)) | _spread3(q[:, 2])


def sorted_keys(bmin, bmax):
    code = morton_codes(bmin, bmax)
    return np.sort((code << np.uint64(32)) | np.arange(len(code), dtype=np.uint64))


def _split(keys, lo, hi):
    """First position of [lo, hi] whose key has the highest bit set in which keys[lo] and keys[hi] differ"""
    a, b = int(keys[lo]), int(keys[hi])
    bit = (a ^ b).bit_length() - 1
    assert bit >= 0, "the keys are unique"
    first_with_bit = (b >> bit) << bit
    m = lo + int(np.searchsorted(keys[lo:hi + 1], np.uint64(first_with_bit), side="left"))
    assert lo < m <= hi
    return m


def refit(tree, bmin, bmax):
    """The tree with the same topology and order over other object boxes: every box the float32 min / max of what lies below
    it, from the leaves up (children are numbered behind their parent)"""
    bmin, bmax = np.asarray(bmin, np.float32).reshape(-1, 3), np.asarray(bmax, np.float32).reshape(-1, 3)
    index, count_leaf, order = tree["bvh_index"], tree["bvh_count_leaf"], tree["bvh_order"]
    n = len(index)
    lo, hi = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    for i in range(n - 1, -1, -1):
        k = int(index[i])
        if count_leaf[i] & LEAF:
            objs = order[k:k + int(count_leaf[i] & 0x7fffffff)]
            lo[i], hi[i] = bmin[objs].min(0), bmax[objs].max(0)
        else:
            lo[i], hi[i] = np.minimum(lo[k], lo[k + 1]), np.maximum(hi[k], hi[k + 1])
    out = dict(tree)
    out["bvh_bmin"], out["bvh_bmax"] = lo, hi
    return out


def build(bmin, bmax):
    """The tree DeviceScene(hs, bvh="device").export_bvh() returns for objects with these boxes (prim_bmin, prim_bmax of
    HostScene.arrays()), as the same dict.  No object: no tree (empty arrays, depth 0)."""
    bmin, bmax = np.asarray(bmin, np.float32).reshape(-1, 3), np.asarray(bmax, np.float32).reshape(-1, 3)
    n = len(bmin)
    if n == 0:
        return dict(bvh_bmin=np.zeros((0, 3), np.float32), bvh_bmax=np.zeros((0, 3), np.float32), bvh_index=np.zeros(0, np.uint32),
                    bvh_count_leaf=np.zeros(0, np.uint32), bvh_order=np.zeros(0, np.uint32), bvh_max_depth=0)
    keys = sorted_keys(bmin, bmax)
    index, count_leaf = [0], [0]
    max_depth = 0
    todo = [(0, n - 1, 0, 1)]  # (first key, last key, node, nodes on the path from the root to this one)
    while todo:
        lo, hi, node, depth = todo.pop()
        if hi - lo <= 1:  # one key, or two single keys under one node: a leaf
            index[node], count_leaf[node] = lo, LEAF | (hi - lo + 1)
            max_depth = max(max_depth, depth + (hi - lo))  # the two single keys are nodes of the unmerged tree
            continue
        m = _split(keys, lo, hi)
        index[node] = len(index)
        index += [0, 0]
        count_leaf += [0, 0]
        todo.append((m, hi, index[node] + 1, depth + 1))
        todo.append((lo, m - 1, index[node], depth + 1))  # on top: the left subtree is numbered first
    tree = dict(bvh_index=np.array(index, np.uint32), bvh_count_leaf=np.array(count_leaf, np.uint32),
                bvh_order=(keys & np.uint64(0xffffffff)).astype(np.uint32), bvh_max_depth=max_depth)
    return refit(tree, bmin, bmax)


def measured_depth(tree):
    """Nodes on the longest path from the root to an object, walking the arrays: a leaf of two objects stands for a node with
    two single-object leaves below it"""
    if len(tree["bvh_index"]) == 0:
        return 0
    deepest = 0
    todo = [(0, 1)]
    while todo:
        i, depth = todo.pop()
        k = int(tree["bvh_index"][i])
        if tree["bvh_count_leaf"][i] & LEAF:
            count = int(tree["bvh_count_leaf"][i] & 0x7fffffff)
            assert count in (1, 2)
            deepest = max(deepest, depth + count - 1)
        else:
            todo += [(k, depth + 1), (k + 1, depth + 1)]
    return deepest


def check_boxes(tree, a, what):
    """Every leaf box is the union of its objects' boxes, every inner box the union of its two children: float32 equality"""
    leaf = (tree["bvh_count_leaf"] & 0x80000000) != 0
    count = tree["bvh_count_leaf"] & 0x7fffffff
    index = tree["bvh_index"]
    seen = np.zeros(len(tree["bvh_order"]), np.int32)
    for i in range(len(index)):
        if leaf[i]:
            objs = tree["bvh_order"][index[i]:index[i] + count[i]]
            assert len(objs) == count[i] and count[i] >= 1
            seen[index[i]:index[i] + count[i]] += 1
            lo, hi = a["prim_bmin"][objs].min(0), a["prim_bmax"][objs].max(0)
        else:
            assert index[i] > i and index[i] + 1 < len(index)
            lo = np.minimum(tree["bvh_bmin"][index[i]], tree["bvh_bmin"][index[i] + 1])
            hi = np.maximum(tree["bvh_bmax"][index[i]], tree["bvh_bmax"][index[i] + 1])
        assert np.array_equal(tree["bvh_bmin"][i], lo) and np.array_equal(tree["bvh_bmax"][i], hi), "%s: box of node %d" % (what, i)
    assert (seen == 1).all(), "%s: the leaves do not partition the leaf order" % what
    assert sorted(tree["bvh_order"].tolist()) == list(range(a["n_prims"]))


def assert_same_tree(got, want, what):
    """Byte equality of the five arrays, and the depth"""
    for k in TREE_KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if g.shape != w.shape:
            raise AssertionError("%s: %s has shape %r, the model's %r" % (what, k, g.shape, w.shape))
        if g.tobytes() != w.tobytes():
            rows = np.nonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(len(g), -1).any(1))[0]
            raise AssertionError("%s: %s differs in %d of %d rows, first at %d: %r, the model's %r" % (
                what, k, len(rows), len(g), rows[0], g[rows[0]], w[rows[0]]))
    assert int(got["bvh_max_depth"]) == int(want["bvh_max_depth"]), "%s: bvh_max_depth %d, the model's %d" % (
        what, got["bvh_max_depth"], want["bvh_max_depth"])


# ---- synthetic scenes -------------------------------------------------------------------------------------------------------

HEADER = ["bclr 0.1 0.2 0.3", "v", "from 0 -6 1", "at 0 0 0", "up 0 0 1", "angle 40", "hither 0.01", "resolution 64 64",
          "aperture 0", "focal 1", "l 3 -4 5 1 1 1", "f 0.8 0.3 0.3 0.7 1 1 1 0.3 20 0 1 0 0 0"]


def _num(x):
    return "%.9g" % float(np.float32(x))  # nine significant digits: a float32 survives them


def sphere(c, r):
    return "s %s %s" % (" ".join(_num(x) for x in c), _num(r))


def triangle(a, b, c):
    return "p 3\n" + "\n".join(" ".join(_num(x) for x in p) for p in (a, b, c))


def box(lo, hi):
    return "box %s %s" % (" ".join(_num(x) for x in lo), " ".join(_num(x) for x in hi))


def plane(a, b, c):
    return "pl " + "  ".join(" ".join(_num(x) for x in p) for p in (a, b, c))


def write_p3f(path, objects, view=None):
    """A scene of the object lines `objects` (sphere, triangle, box, plane above) under the header, light and material of
    test_device_built_bvh_tiny_scenes; `view`: (from, at) in place of the header's"""
    lines = list(HEADER)
    if view is not None:
        lines[2] = "from " + " ".join(_num(x) for x in view[0])
        lines[3] = "at " + " ".join(_num(x) for x in view[1])
    with open(path, "w") as f:
        f.write("\n".join(lines + list(objects)) + "\n")
    return path


def counts_scene(n, seed=1):
    """n small spheres at seeded random positions"""
    rng = np.random.default_rng(1000 * seed + n)
    c = rng.uniform(-1, 1, (n, 3))
    return [sphere(p, 0.05) for p in c]


def coincident_scene(n=1000):
    """Concentric spheres: one centre, every extent 0; the index half of the key decides everything"""
    return [sphere((0.25, -0.5, 0.125), 0.5 + k / 1024.0) for k in range(n)]


def duplicates_scene(n=600):
    return [triangle((-0.5, 0.25, -0.5), (0.75, 0.25, -0.25), (0, 0.5, 0.5))] * n


def flat_triangles_scene(n=1500, seed=2):
    """Triangles whose boxes all span z in [0.25, 0.75]: every centre has z = 0.5"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        p = rng.uniform(-1, 1, (3, 3))
        p[:, 2] = rng.permutation([0.25, 0.75, rng.choice([0.25, 0.5, 0.75])])
        out.append(triangle(*p))
    return out


def line_scene(n=700, seed=3):
    """Spheres at seeded places on the line y = 0.5, z = -0.25, -2 <= x <= 2, with seeded radii between 0.05 and 0.5 (multiples
    of 1/1024, so that the box centres have exactly that y and z).
    Why the radii differ: spheres of one radius crowded on a line are met broadside at almost one t by a dozen neighbours, and
    since every sphere test re-normalises the ray (Q8) the order of the tests then decides the object: the reference's own
    BVH and its own object loop named different objects on 2e-3 of scene_rays' rays over such a line, whatever its spacing.
    With radii that differ the nearest sphere is the locally largest, by a margin: they disagree on 0 or 1 ray of 20 000."""
    rng = np.random.default_rng(seed)
    return [sphere((x, 0.5, -0.25), k / 1024.0) for x, k in zip(rng.uniform(-2, 2, n), rng.integers(52, 513, n))]


def lattice_scene(scale=1.0, shift=(0.0, 0.0, 0.0)):
    """16 x 16 x 8 small boxes whose centres lie on multiples of 1/1024 of the extent of the centres (the unit cube before
    `scale` and `shift`), both corners among them: cells 0, 1, 2, 3 and 1020 .. 1024 of the scale are all met on some axis.
    The half-width 1/4096 is a power of two, so before scale and shift centre -/+ half-width and their mean are exact."""
    ticks = {16: [0, 1, 2, 3, 64, 255, 256, 511, 512, 513, 767, 1020, 1021, 1022, 1023, 1024], 8: [0, 1, 511, 512, 1021, 1022, 1023, 1024]}
    h = 1.0 / 4096
    out = []
    for i in ticks[16]:
        for j in ticks[16]:
            for k in ticks[8]:
                c = np.array([i, j, k]) / 1024.0
                out.append(box((c - h) * scale + np.array(shift), (c + h) * scale + np.array(shift)))
    return out


def outlier_scene(n=3000, seed=4):
    """n objects in the unit cube, one at distance 1e6: the others share Morton cell 0"""
    rng = np.random.default_rng(seed)
    out = []
    for i, c in enumerate(rng.uniform(0.05, 0.95, (n, 3))):
        if i % 3 == 0:
            out.append(sphere(c, 0.02))
        elif i % 3 == 1:
            out.append(triangle(*(c + rng.uniform(-0.04, 0.04, (3, 3)))))
        else:
            out.append(box(c - 0.02, c + 0.02))
    out.insert(n // 2, sphere((6e5, 6e5, 5.2e5), 1.0))  # |c| = 1e6 to three digits
    return out


def chain_scene(n_origin=2048):
    """A deep skewed tree: on each axis spheres centred at 2^m / 1024 (m = 0 .. 9) and at 1, which peel one Morton bit each off
    the cell of the origin, and n_origin concentric spheres at the origin, which the index bits split eleven times more.  All
    radii near 1e-3 and distinct."""
    out, k = [], 0

    def radius():
        nonlocal k
        k += 1
        return 1e-3 * (1 + k / 2081.0)

    for axis in range(3):
        for m in list(range(10)) + [None]:
            c = [0.0, 0.0, 0.0]
            c[axis] = 1.0 if m is None else 2.0 ** m / 1024
            out.append(sphere(c, radius()))
    out += [sphere((0, 0, 0), radius()) for _ in range(n_origin)]
    return out


def scene_rays(a, n=20000, seed=5):
    """Unit rays into a scene with the arrays `a`, in the style of rays() of test_gpu_scene_update.py.  The first half is
    scaled to the scene: origins up to three half-extents from the middle of the box around the objects, aimed at a point
    of that box, a quarter of them with one direction component 0.  (That box leaves out the extreme thousandth of each
    side: an outlier does not make every ray miss the rest.)  The second half is scaled to an object each, so that small
    and far objects are met too: aimed at a point of the box of a seeded object, from 2 to 8 diagonals of that box away,
    again a quarter with one component 0.
    Why not from further away: the sphere test's discriminant b * b - c carries an error of about 2^-23 d^2 at distance d,
    so at d = 1000 r a tenth of r^2 is noise, and since every sphere test re-normalises the traversal's ray (Q8) two back
    ends of the REFERENCE then disagree on hit or miss for a visible share of the rays that come near such a sphere.  At
    d <= 8 diagonals = 28 r the noise is 1e-4 r^2, and the rays it can flip are 1e-4 of those that hit."""
    rng = np.random.default_rng(seed)
    bmin, bmax = a["prim_bmin"].astype(np.float64), a["prim_bmax"].astype(np.float64)
    lo, hi = np.quantile(bmin, 0.001, axis=0, method="lower"), np.quantile(bmax, 0.999, axis=0, method="higher")
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    half = np.maximum(half, 0.05 * half.max())
    h = n // 2
    o = mid + rng.uniform(-3, 3, (n, 3)) * half
    d = mid + rng.uniform(-1, 1, (n, 3)) * half - o
    obj = rng.integers(0, len(bmin), n - h)
    size = bmax[obj] - bmin[obj]
    target = bmin[obj] + rng.uniform(0, 1, (n - h, 3)) * size
    d[h:] = rng.standard_normal((n - h, 3))
    d[: h // 4, rng.integers(0, 3)] = 0
    d[h: h + h // 4, rng.integers(0, 3)] = 0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o[h:] = target - d[h:] * (rng.uniform(2, 8, (n - h, 1)) * np.linalg.norm(size, axis=1, keepdims=True))
    return o.astype(np.float32), d.astype(np.float32)


# (name, object lines, (from, at) of a camera that sees them).  Every box is finite.
def synthetic_scenes():
    return [("coincident", coincident_scene(), None), ("duplicates", duplicates_scene(), None),
            ("flat_triangles", flat_triangles_scene(), None), ("line", line_scene(), None),
            ("lattice", lattice_scene(), ((0.5, -3, 0.5), (0.5, 0.5, 0.5))),
            ("lattice_scaled", lattice_scene(3.0, (1000.0, -2000.0, 0.5)), ((1001.5, -2010, 2), (1001.5, -1998.5, 2))),
            ("outlier", outlier_scene(), ((0.5, -2, 0.5), (0.5, 0.5, 0.5))),
            ("chain", chain_scene(), ((0, -0.02, 0.004), (0, 0, 0)))]  # close up: the spheres at the origin are ten pixels wide
