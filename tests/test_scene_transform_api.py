"""Transforms of a live scene's objects (p3d_scene_transform_prims, include/p3d.h) without a GPU: the entry point and its two
structures are declared, exported and wrapped, and p3d.transformed - the numpy float32 statement of the point arithmetic the
device kernel runs - returns the input bits for the identity, equals scene_update_helpers.translated for a pure translation,
stays within 4 ulp of the largest term of a float64 evaluation, and produces rows HostScene.set_geometry accepts."""
import ctypes as C
import re

import numpy as np
import pytest

from api_checks import header_code
from conftest import scene_path
import p3d_amd as p3d
from scene_update_helpers import BOX, PLANE, SPHERE, TRIANGLE, translated

LEGACY = ("tri_low.p3f", "box.p3f", "balls_box.p3f")  # 11-number `f` lines (P3D_LOAD_LEGACY_F11)
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


def _load(scene):
    hs = p3d.HostScene(scene_path(scene), legacy_f11=scene in LEGACY)
    return hs, hs.arrays()


def _runs(kinds, wanted):
    """Maximal runs of consecutive objects whose kind is in `wanted` -> [(first, count)]"""
    out, start = [], None
    for i, k in enumerate(list(kinds) + [None]):
        if k in wanted and start is None:
            start = i
        elif k not in wanted and start is not None:
            out.append((start, i - start))
            start = None
    return out


def _rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_header_declares_the_entry_point_and_its_structures():
    code = header_code()
    assert re.search(r"typedef\s+struct\s+p3d_xform\s*\{\s*float\s+m\[12\]\s*;\s*float\s+sphere_scale\s*;\s*uint32_t\s+reserved\[3\]\s*;\s*\}\s*p3d_xform\s*;", code)
    assert re.search(r"typedef\s+struct\s+p3d_xform_range\s*\{\s*uint32_t\s+first\s*,\s*count\s*,\s*xform\s*,\s*reserved\s*;\s*\}\s*p3d_xform_range\s*;", code)
    assert re.search(r"\bint\s+p3d_scene_transform_prims\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*const\s+p3d_xform_range\s*\*\s*\w+,\s*uint32_t\s+\w+,"
                     r"\s*const\s+p3d_xform\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*float\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)
    # 12 + 1 floats and 3 words; 4 words
    assert C.sizeof(p3d.Xform) == 64 and C.sizeof(p3d.XformRange) == 16


def test_library_exports_it_and_python_wraps_it():
    lib = p3d.lib()
    assert hasattr(lib, "p3d_scene_transform_prims")
    assert "p3d_scene_transform_prims" in p3d.EXPORTS
    assert lib.p3d_abi_version() == 4
    assert hasattr(p3d.DeviceScene, "transform_prims") and callable(p3d.transformed)
    ms = C.c_float(7.0)
    assert lib.p3d_scene_transform_prims(None, 0, None, 0, None, p3d.UPDATE_REBUILD, C.byref(ms)) == -1  # P3D_ERR_INVALID
    assert b"null" in lib.p3d_last_error()


@pytest.mark.parametrize("scene,kind", [("balls_low.p3f", SPHERE), ("tri_low.p3f", TRIANGLE), ("balls_box.p3f", BOX), ("box.p3f", BOX)])
def test_identity_returns_the_input_bits(scene, kind):
    _, a = _load(scene)
    ranges = [(f, c, 0) for f, c in _runs(a["prim_type"], (kind,))]
    assert ranges, "%s has no object of kind %d" % (scene, kind)
    objs, new_v = p3d.transformed(a["prim_type"], a["prim_v"], ranges, IDENTITY[None])
    assert len(objs) == sum(c for _, c, _ in ranges) and (a["prim_type"][objs] == kind).all()
    assert new_v.dtype == np.float32 and new_v.tobytes() == a["prim_v"][objs].tobytes()


@pytest.mark.parametrize("scene", ["balls_low.p3f", "tri_low.p3f", "balls_box.p3f"])
def test_pure_translation_equals_translated(scene):
    """(1 x + 0 y) + 0 z + d is x + d: one range per object, each with its own offset"""
    _, a = _load(scene)
    movable = np.nonzero(a["prim_type"] != PLANE)[0]
    rng = np.random.default_rng(3)
    offsets = rng.uniform(-2, 2, (len(movable), 3)).astype(np.float32)
    m = np.repeat(IDENTITY[None], len(movable), 0)
    m[:, :, 3] = offsets
    objs, new_v = p3d.transformed(a["prim_type"], a["prim_v"], [(int(o), 1, i) for i, o in enumerate(movable)], m)
    assert np.array_equal(objs, movable)
    assert new_v.tobytes() == translated(a["prim_type"], a["prim_v"], movable, offsets).tobytes()


@pytest.mark.parametrize("scene", ["balls_low.p3f", "tri_low.p3f"])
def test_rotation_is_within_4_ulp_of_the_largest_term(scene):
    """Against the same float32 inputs evaluated in float64.  Three products rounded to half an ulp of themselves and three
    sums rounded to half an ulp of partial sums: the issue's bound, 4 ulp of the largest of |m0 x|, |m1 y|, |m2 z|, |m3|."""
    _, a = _load(scene)
    rng = np.random.default_rng(17)
    m = np.zeros((3, 4))
    m[:, :3] = _rotation(rng)
    m[:, 3] = rng.uniform(-1, 1, 3)
    m32 = m.astype(np.float32)
    ranges = [(f, c, 0) for f, c in _runs(a["prim_type"], (SPHERE, TRIANGLE))]
    objs, new_v = p3d.transformed(a["prim_type"], a["prim_v"], ranges, m32[None], sphere_scale=[1.25])
    m64 = m32.astype(np.float64)
    checked = 0
    for o, row in zip(objs, new_v):
        kind = int(a["prim_type"][o])
        for c in {SPHERE: (0,), TRIANGLE: (0, 3, 6)}[kind]:
            p = a["prim_v"][o, c:c + 3].astype(np.float64)
            terms = np.abs(np.concatenate([m64[:, :3] * p, m64[:, 3:]], axis=1))  # (3 rows, 4 terms)
            exact = (m64[:, :3] * p).sum(1) + m64[:, 3]
            bound = 4 * np.spacing(terms.max(1).astype(np.float32)).astype(np.float64)
            assert (np.abs(row[c:c + 3].astype(np.float64) - exact) <= bound).all(), (int(o), c)
            checked += 1
        if kind == SPHERE:
            assert row[3] == np.float32(a["prim_v"][o, 3] * np.float32(1.25))
            assert row[4:].tobytes() == a["prim_v"][o, 4:].tobytes()
    assert checked >= len(objs) > 0


@pytest.mark.parametrize("scene", ["tri_low.p3f", "balls_box.p3f"])
def test_set_geometry_takes_its_output(scene):
    hs, a = _load(scene)
    rng = np.random.default_rng(5)
    rot = np.zeros((3, 4), np.float32)
    rot[:, :3] = _rotation(rng)
    rot[:, 3] = (0.25, -0.5, 0.125)
    scale = np.array([[1.5, 0, 0, 0.25], [0, 0.75, 0, -0.5], [0, 0, 2.0, 0.125]], np.float32)
    ranges = [(f, c, 0) for f, c in _runs(a["prim_type"], (SPHERE, TRIANGLE))] + [(f, c, 1) for f, c in _runs(a["prim_type"], (BOX,))]
    objs, new_v = p3d.transformed(a["prim_type"], a["prim_v"], ranges, np.stack([rot, scale]), sphere_scale=[1.25, 1.0])
    assert len(objs) == int((a["prim_type"] != PLANE).sum())
    hs.set_geometry(objs, new_v)
    b = hs.arrays()
    assert b["prim_v"][objs].tobytes() == new_v.tobytes()
    assert b["prim_v"].tobytes() != a["prim_v"].tobytes()
    assert np.isfinite(b["prim_bmin"]).all() and (b["prim_bmin"] <= b["prim_bmax"]).all()


def test_transformed_refuses_planes_and_rotated_boxes():
    _, a = _load("balls_box.p3f")
    rot = np.zeros((3, 4), np.float32)
    rot[:, :3] = _rotation(np.random.default_rng(1))
    box = int(np.nonzero(a["prim_type"] == BOX)[0][0])
    with pytest.raises(ValueError):
        p3d.transformed(a["prim_type"], a["prim_v"], [(box, 1, 0)], rot[None])
    planes = np.nonzero(a["prim_type"] == PLANE)[0]
    if len(planes):
        with pytest.raises(ValueError):
            p3d.transformed(a["prim_type"], a["prim_v"], [(int(planes[0]), 1, 0)], IDENTITY[None])
    with pytest.raises(ValueError):
        p3d.transformed(a["prim_type"], a["prim_v"], [(len(a["prim_type"]), 1, 0)], IDENTITY[None])
