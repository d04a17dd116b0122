"""Sphere sweeps (include/p3d_sweep.h) without a GPU: the entry points are declared, exported and wrapped as functions; the
wrappers refuse what cannot be swept with the library's code before the library is called; host_sweep_sphere, the statement of
the semantics, is held to the float64 model of sweep_reference.py on sphere, triangle, plane and mixed scenes; and cases worked
out by hand, in numbers whose float32 arithmetic is exact, pin the contact times, the ties and the inputs that find nothing."""
import json
import os
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
from device_query_contract import FLT_MAX, INVALID, UNSUPPORTED
from intersect_reference import HEAD
import p3d_amd as p3d
import sweep_reference as sw



def test_the_header_declares_them():
    code, main = header_code("p3d_sweep.h"), header_code()
    assert re.search(r'#include\s+"p3d_sweep.h"', main) and re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)
    cf, f, i32, u32 = r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,", r"\s*uint32_t\s+\w+\s*,"
    assert re.search(r"\bint\s+p3d_sweep_sphere_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 + u32 + cf * 4 + i32 + f * 4 + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_host_scene_sweep_sphere\s*\(\s*const\s+p3d_host_scene\s*\*\s*\w+," + u32 + cf * 4 + i32 + f * 2 + r"\s*float\s*\*\s*\w+\s*\)", code)


def test_the_library_exports_them_and_python_wraps_them_as_functions():
    names = ("p3d_sweep_sphere_device", "p3d_host_scene_sweep_sphere")
    lib = p3d.lib()
    for name in names:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    assert [len(p3d.PROTOTYPES[name][1]) for name in names] == [13, 10]
    assert lib.p3d_abi_version() == 4
    record = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "python_api_surface.json")))
    classes = [k for k, v in record["names"].items() if v["kind"] in ("class", "structure")]
    assert "DeviceScene" in classes and "HostScene" in classes
    for fn in ("sweep_sphere_device", "host_sweep_sphere"):
        assert callable(getattr(p3d, fn)), fn
        for cls in classes:
            assert not hasattr(getattr(p3d, cls), fn), "%s is a member of the recorded class %s" % (fn, cls)
    assert list(p3d._SWEEP_OUTPUTS) == ["object", "t", "centre", "contact", "normal"]
    # a null scene is refused by name before anything else
    assert lib.p3d_sweep_sphere_device(None, p3d.ACCEL_BVH, 4, *([None] * 10)) == INVALID
    assert b"p3d_sweep_sphere_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_host_scene_sweep_sphere(None, 0, *([None] * 8)) == INVALID
    assert b"p3d_host_scene_sweep_sphere" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def scene(tmp_path, name, body):
    path = tmp_path / (name + ".p3f")
    path.write_text(HEAD + body)
    return p3d.HostScene(str(path))


def test_the_wrappers_refuse_with_the_right_code(tmp_path):
    import torch
    raw = (0x1000, 6)  # a raw (address, rows) pair is taken at its word
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    boxed = scene(tmp_path, "boxed", "s 0 0 0 1\nbox -1 3 -1 1 5 1\n")
    plane = scene(tmp_path, "plane", "s 0 0 0 1\npl 0 -8 0  1 -8 0  0 -8 1\n")
    plain = scene(tmp_path, "plain", "s 0 0 0 1\n")

    def dev(host):
        d = scene_without_a_library()
        d.host = host
        return d

    q = p3d.sweep_sphere_device
    cases = [
        ("a scene with a box", UNSUPPORTED, "box", lambda: q(dev(boxed), p3d.ACCEL_NONE, raw, raw, raw)),
        ("a scene with a box under the tree", UNSUPPORTED, "box", lambda: q(dev(boxed), p3d.ACCEL_BVH, raw, raw, raw)),
        ("the grid", UNSUPPORTED, "grid", lambda: q(dev(plain), p3d.ACCEL_GRID, raw, raw, raw)),
        ("the grid, host scene unknown", UNSUPPORTED, "grid", lambda: q(dev(None), p3d.ACCEL_GRID, raw, raw, raw)),
        ("the tree over a scene with a plane", UNSUPPORTED, "plane", lambda: q(dev(plane), p3d.ACCEL_BVH, raw, raw, raw)),
        ("a short radius", INVALID, "6 origins, 5 radii", lambda: q(dev(plain), p3d.ACCEL_BVH, raw, raw, (0x2000, 5))),
        ("a short limit", INVALID, "6 origins, 6 directions, 5 limits", lambda: q(dev(plain), p3d.ACCEL_BVH, raw, raw, raw, t_max=(0x2000, 5))),
        ("fewer directions", INVALID, "6 origins, 5 directions", lambda: q(dev(plain), p3d.ACCEL_BVH, raw, (0x2000, 5), raw)),
        ("a short output", INVALID, "5 rows for 6 balls", lambda: q(dev(plain), p3d.ACCEL_NONE, raw, raw, raw, want=(), out={"object": (0x4000, 5)})),
        ("a missing output", INVALID, "out has no 't'", lambda: q(dev(plain), p3d.ACCEL_NONE, raw, raw, raw, out={"object": raw})),
        ("an unknown output", INVALID, "unknown output 'hit_point'", lambda: q(dev(plain), p3d.ACCEL_BVH, raw, raw, raw, want=("hit_point",))),
        ("numpy origins", INVALID, "origin: a CUDA/HIP torch.Tensor", lambda: q(dev(plain), p3d.ACCEL_BVH, np.zeros((6, 3), np.float32), raw, raw)),
        ("a CPU radius", INVALID, "radius: the tensor is in host memory", lambda: q(dev(plain), p3d.ACCEL_BVH, raw, raw, f32(6))),
        ("a 2-d radius", INVALID, "radius: shape", lambda: q(dev(plain), p3d.ACCEL_BVH, raw, raw, f32(6, 1))),
        ("a float object", INVALID, "out['object']: dtype", lambda: q(dev(plain), p3d.ACCEL_BVH, raw, raw, raw, want=(), out={"object": f32(6)})),
        ("host form: shapes", INVALID, "needed: (n, 3) both", lambda: p3d.host_sweep_sphere(plain, np.zeros((4, 3)), np.zeros((5, 3)), 1.0)),
        ("host form: radii", INVALID, "4 origins, 3 radii", lambda: p3d.host_sweep_sphere(plain, np.zeros((4, 3)), np.zeros((4, 3)), np.ones(3))),
        ("host form: limits", INVALID, "4 origins, 5 limits", lambda: p3d.host_sweep_sphere(plain, np.zeros((4, 3)), np.zeros((4, 3)), 1.0, t_max=np.ones(5))),
        ("host form: a box", UNSUPPORTED, "object 1 is a box", lambda: p3d.host_sweep_sphere(boxed, np.zeros((4, 3)), np.ones((4, 3)), 1.0)),
    ]
    for what, code, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == code and word in str(e.value), "%s: %s" % (what, e.value)
    # the plane is there for the brute force, and a box is refused whatever n
    assert p3d.host_sweep_sphere(plane, [[0, 0, 0]], [[0, -1, 0]], 1.0)[0][0] == 0
    with pytest.raises(p3d.P3DError):
        p3d.host_sweep_sphere(boxed, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0))


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    return sw.scene_paths(tmp_path_factory.mktemp("sweep"))


@pytest.mark.parametrize("name", list(sw.SCENES))
def test_the_host_form_is_the_float64_model(name, paths):
    c = sw.cases(paths[name], sw.SCENES[name][0] + 500)
    hs = p3d.HostScene(paths[name])
    free = p3d.host_sweep_sphere(hs, c.o, c.d, c.r)
    err, _ = sw.check_sweep(c.objects, c.o, c.d, c.r, c.free_T, c.free_margin, free, name)
    sw.assert_within(err, name)
    lim = p3d.host_sweep_sphere(hs, c.o, c.d, c.r, t_max=c.limits)
    err, _ = sw.check_sweep(c.objects, c.o, c.d, c.r, c.lim_T, c.lim_margin, lim, name + ", limits")
    sw.assert_within(err, name + ", limits")
    dead = ~(c.limits > 0)
    assert dead.sum() >= 3 * (len(c.o) // 75) and (lim[0][dead] == -1).all(), name + ": a zero, negative or NaN limit found something"
    # a limit takes answers away and changes none: where something is still met it is the unlimited answer, bit for bit
    kept = lim[0] >= 0
    assert 0 < kept.sum() < (free[0] >= 0).sum()
    for a, b in zip(lim, free):
        assert a[kept].tobytes() == b[kept].tobytes(), name + ": a limit changed an answer"
    assert (free[1][kept] <= c.limits[kept]).all()
    # the sets hold what they are said to hold
    assert (c.r == 0).sum() >= len(c.o) // 40 and (free[1] == 0).sum() >= len(c.o) // 4
    assert ((free[0] >= 0) & (free[1] > 0)).sum() >= len(c.o) // 5


# ---- by hand: dyadic numbers, 3-4-5 triangles ---------------------------------------------------------------------------------------
# object 0: the triangle (0,-1,0) (0,1,0) (-2,0,0) in the plane z = 0, an edge on the y axis, normal (0,0,-1) x ... = +z side up
# object 1: a shell of radius 8 about (40, 0, 0)
# object 2: the plane y = -8 (normal as the loader turns it)
# objects 3, 4: two unit spheres at (0, 30, 4) and (0, 30, -4): a ball between them meets both at once
BY_HAND = """p 3
0 -1 0
0 1 0
-2 0 0
s 40 0 0 8
pl 0 -8 0  1 -8 0  0 -8 1
s 0 30 4 1
s 0 30 -4 1
"""
TRI, SHELL, PLANE, TWIN_A, TWIN_B = range(5)
NAN = float("nan")
EXACT = [  # (what, origin, direction, radius, t_max or None, object, t)
    ("dropped on the middle of the face", [-0.5, 0, 5], [0, 0, -1], 1, None, TRI, 4.0),              # height - r
    ("the same with a direction twice as long", [-0.5, 0, 5], [0, 0, -2], 1, None, TRI, 2.0),         # t is in units of d
    ("from below", [-0.5, 0, -5], [0, 0, 1], 1, None, TRI, 4.0),
    ("onto an edge", [3, 0, 10], [0, 0, -1], 5, None, TRI, 6.0),                                      # 3-4-5 about the y axis
    ("onto a vertex", [0, 4, 10], [0, 0, -1], 5, None, TRI, 6.0),                                     # 3-4-5 about (0, 1, 0)
    ("a point onto the face", [-0.5, 0, 5], [0, 0, -1], 0, None, TRI, 5.0),
    ("a point past the edge", [0.5, 0, 5], [0, 0, -1], 0, None, -1, None),
    ("inside the shell", [42, 0, 0], [1, 0, 0], 2, None, SHELL, 4.0),                                 # (R - r - offset) / |d|
    ("inside the shell, d twice as long", [42, 0, 0], [2, 0, 0], 2, None, SHELL, 2.0),
    ("inside the shell, the other way", [42, 0, 0], [-1, 0, 0], 2, None, SHELL, 8.0),
    ("onto the shell from outside", [20, 0, 0], [1, 0, 0], 2, None, SHELL, 10.0),
    ("touching at the start", [-0.5, 0, 1], [0, 0, 1], 1, None, TRI, 0.0),                            # moving away, but already there
    ("overlapping at the start", [-0.5, 0, 0.5], [1, 0, 0], 1, None, TRI, 0.0),
    ("standing still and touching", [-0.5, 0, 0.5], [0, 0, 0], 1, None, TRI, 0.0),
    ("standing still and free", [-0.5, 0, 3], [0, 0, 0], 1, None, -1, None),
    ("towards the plane", [0, -4, 40], [0, -1, 0], 1, None, PLANE, 3.0),
    ("away from the plane", [0, -4, 40], [0, 1, 0], 1, None, -1, None),
    ("along the plane", [0, -4, 40], [1, 0, 0], 1, None, -1, None),
    ("from under the plane", [0, -12, 40], [0, 2, 0], 1, None, PLANE, 1.5),
    ("a limit before the contact", [-0.5, 0, 5], [0, 0, -1], 1, 3.5, -1, None),
    ("a limit at the contact", [-0.5, 0, 5], [0, 0, -1], 1, 4.0, TRI, 4.0),                           # t in [0, t_max], closed
    ("a limit behind the contact", [-0.5, 0, 5], [0, 0, -1], 1, 4.5, TRI, 4.0),
    ("equal T on two objects", [0, 20, 0], [0, 1, 0], 4, None, TWIN_A, 7.0),                          # 3-4-5 twice: the lower index
    ("a negative radius", [-0.5, 0, 5], [0, 0, -1], -1, None, -1, None),
    ("a NaN radius", [-0.5, 0, 5], [0, 0, -1], NAN, None, -1, None),
    ("a zero limit", [-0.5, 0, 0.5], [0, 0, -1], 1, 0.0, -1, None),                                   # even when touching
    ("a negative limit", [-0.5, 0, 5], [0, 0, -1], 1, -2.0, -1, None),
    ("a NaN limit", [-0.5, 0, 5], [0, 0, -1], 1, NAN, -1, None),
    ("a NaN origin", [NAN, 0, 5], [0, 0, -1], 1, None, -1, None),
    ("a NaN direction", [-0.5, 0, 0.5], [0, NAN, -1], 1, None, -1, None),                             # even when touching
]


def test_cases_by_hand(tmp_path):
    hs = scene(tmp_path, "by_hand", BY_HAND)
    for limited in (False, True):
        rows = [c for c in EXACT if (c[4] is not None) == limited]
        o, d = np.array([c[1] for c in rows], np.float32), np.array([c[2] for c in rows], np.float32)
        r = np.array([c[3] for c in rows], np.float32)
        lim = np.array([c[4] for c in rows], np.float32) if limited else None
        obj, t, centre, contact = p3d.host_sweep_sphere(hs, o, d, r, t_max=lim)
        for i, c in enumerate(rows):
            assert obj[i] == c[5], "%s: object %d, the answer is %d" % (c[0], obj[i], c[5])
            if c[5] < 0:
                assert t[i] == FLT_MAX and not centre[i].any() and not contact[i].any(), c[0] + ": the no-answer values"
            else:
                assert t[i] == np.float32(c[6]), "%s: t %r, the answer is %r" % (c[0], t[i], c[6])
                assert (centre[i] == o[i] + d[i] * t[i]).all(), c[0] + ": centre"
    # where the ball touches: under the centre on the face; on the edge and at the vertex, 5 away
    at = {c[0]: i for i, c in enumerate([c for c in EXACT if c[4] is None])}
    rows = [c for c in EXACT if c[4] is None]
    o, d, r = (np.array([c[k] for c in rows], np.float32) for k in (1, 2, 3))
    obj, t, centre, contact = p3d.host_sweep_sphere(hs, o, d, r)
    assert contact[at["dropped on the middle of the face"]].tolist() == [-0.5, 0, 0] and centre[at["dropped on the middle of the face"]].tolist() == [-0.5, 0, 1]
    assert contact[at["onto an edge"]].tolist() == [0, 0, 0] and centre[at["onto an edge"]].tolist() == [3, 0, 4]
    assert contact[at["onto a vertex"]].tolist() == [0, 1, 0] and centre[at["onto a vertex"]].tolist() == [0, 4, 4]
    assert contact[at["inside the shell"]].tolist() == [48, 0, 0] and contact[at["towards the plane"]].tolist() == [0, -8, 40]
    # m + (c - m) R / |c - m| with |c - m| = 5: (0, 29.4, 3.2), not dyadic: within an ulp of 32 per rounding
    assert np.abs(contact[at["equal T on two objects"]] - np.array([0, 29.4, 3.2])).max() <= 2.0 ** -18
    # one number for every radius, and the optional outputs may be left out at the C level
    same = p3d.host_sweep_sphere(hs, o[:3], d[:3], 1.0)
    assert (same[0] == obj[:3]).all() and (same[1] == t[:3]).all()
    only = np.full(3, 77, np.int32)
    assert p3d.lib().p3d_host_scene_sweep_sphere(hs._h, 3, o.ctypes.data, d.ctypes.data, r.ctypes.data, None, only.ctypes.data, None, None, None) == 0
    assert (only == obj[:3]).all()
    assert p3d.lib().p3d_host_scene_sweep_sphere(hs._h, 3, None, d.ctypes.data, r.ctypes.data, None, only.ctypes.data, None, None, None) == INVALID
    assert b"null array" in p3d.lib().p3d_last_error()
