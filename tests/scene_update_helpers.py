"""Shared by test_scene_update_api.py and test_gpu_scene_update.py: deterministic object moves, and the same moves written
into a .p3f so that the loader (and the oracle, which has no setter) sees the moved scene."""
import re

import numpy as np

SPHERE, TRIANGLE, BOX, PLANE = 0, 1, 2, 3
_ARGS = {"s": 4, "box": 6, "p": 10, "pl": 9}  # numbers behind the object keywords of a .p3f (`p`: the vertex count first)


def translated(prim_type, prim_v, objects, offsets):
    """prim_v rows of `objects` moved by `offsets` (n x 3), in float32 arithmetic: sphere centre, the three vertices of a
    triangle, min and max of a box."""
    out = np.array(prim_v[objects], np.float32)
    off = np.asarray(offsets, np.float32).reshape(len(objects), 3)
    for row, (o, d) in enumerate(zip(objects, off)):
        kind = int(prim_type[o])
        assert kind != PLANE
        cols = {SPHERE: (0,), TRIANGLE: (0, 3, 6), BOX: (0, 3)}[kind]
        for c in cols:
            out[row, c:c + 3] = out[row, c:c + 3] + d
    return out


def random_moves(arrays, seed, fraction=1.0 / 3.0, reach=0.05, include=()):
    """A `fraction` of the non-plane objects (plus `include`), each moved by at most `reach` x the diagonal of the box around
    all of them -> (objects, new prim_v rows)."""
    rng = np.random.default_rng(seed)
    movable = np.nonzero(arrays["prim_type"] != PLANE)[0]
    lo = arrays["prim_bmin"][movable].min(0).astype(np.float64)
    hi = arrays["prim_bmax"][movable].max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    k = max(1, int(round(len(movable) * fraction)))
    chosen = set(int(x) for x in rng.choice(movable, k, replace=False)) | set(int(x) for x in include)
    objects = np.array(sorted(chosen), np.uint32)
    direction = rng.standard_normal((len(objects), 3))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    offsets = (direction * rng.uniform(0.2, 1.0, (len(objects), 1)) * reach * diag).astype(np.float32)
    return objects, translated(arrays["prim_type"], arrays["prim_v"], objects, offsets)


def write_moved_p3f(src, dst, prim_type, objects, new_v):
    """A copy of the scene file `src` in which the numbers of the objects `objects` are those of `new_v`, printed with nine
    significant digits (a float32 survives that)."""
    text = open(src).read()
    new = {int(o): np.asarray(v, np.float32) for o, v in zip(objects, new_v)}
    tokens = [(m.group(0), m.start(), m.end()) for m in re.finditer(r"\S+", text)]
    edits = []
    obj = 0
    i = 0
    while i < len(tokens):
        word = tokens[i][0]
        if word in _ARGS:
            args = tokens[i + 1:i + 1 + _ARGS[word]]
            if obj in new:
                kind = int(prim_type[obj])
                assert {"s": SPHERE, "p": TRIANGLE, "box": BOX}[word] == kind
                nums = args[1:] if word == "p" else args
                vals = new[obj][:len(nums)]
                for (_, a, b), x in zip(nums, vals):
                    edits.append((a, b, "%.9g" % float(x)))
            obj += 1
            i += 1 + _ARGS[word]
        else:
            i += 1
    assert obj == len(prim_type), "object count of %s: %d parsed, %d loaded" % (src, obj, len(prim_type))
    for a, b, s in sorted(edits, reverse=True):
        text = text[:a] + s + text[b:]
    with open(dst, "w") as f:
        f.write(text)
    return dst
