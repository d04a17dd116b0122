"""Geometry updates of a live scene (p3d_scene_update_prims / p3d_scene_export_bvh / p3d_host_scene_set_geometry,
include/p3d.h) without a GPU: the entry points are declared, exported and wrapped, the ABI version is untouched,
p3d_host_scene_set_geometry gives byte for byte what the loader gives for a scene file with the same numbers (objects, boxes,
normals and the host BVH built afterwards), and bad arguments are refused without a change."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from api_checks import header_code
from conftest import ROOT, scene_path
import p3d_amd as p3d
from scene_update_helpers import PLANE, translated, write_moved_p3f

SYMBOLS = ["p3d_scene_update_prims", "p3d_scene_export_bvh", "p3d_host_scene_set_geometry"]
PRIM_KEYS = ("prim_v", "prim_type", "prim_material", "prim_n", "prim_bmin", "prim_bmax")
BVH_KEYS = ("bvh_bmin", "bvh_index", "bvh_bmax", "bvh_count_leaf", "bvh_order")
LEGACY = ("tri_low.p3f", "box.p3f")  # 11-number `f` lines (P3D_LOAD_LEGACY_F11): the shipped parser would load no objects


def _same_bytes(a, b, keys, what):
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    code = header_code()
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert re.search(r"typedef\s+enum\s+p3d_update_mode\s*\{\s*P3D_UPDATE_REFIT\s*=\s*0\s*,\s*P3D_UPDATE_REBUILD\s*=\s*1\s*\}\s*p3d_update_mode\s*;", code)
    assert re.search(r"p3d_scene_update_prims\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*const\s+uint32_t\s*\*\s*\w+,\s*const\s+p3d_prim\s*\*\s*\w+,"
                     r"\s*uint32_t\s+\w+,\s*float\s*\*\s*\w+\)", code)
    assert re.search(r"p3d_scene_export_bvh\s*\(\s*p3d_scene\s*\*\s*\w+,\s*p3d_bvh_node\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+,"
                     r"\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+\)", code)
    assert re.search(r"p3d_host_scene_set_geometry\s*\(\s*p3d_host_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*const\s+uint32_t\s*\*\s*\w+,\s*const\s+float\s*\*\s*\w+\s*\)", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4
    assert (p3d.UPDATE_REFIT, p3d.UPDATE_REBUILD) == (0, 1)
    assert hasattr(p3d.HostScene, "set_geometry")
    for name in ("update_prims", "export_bvh"):
        assert hasattr(p3d.DeviceScene, name), name


@pytest.mark.parametrize("scene", ["balls_low.p3f", "tri_low.p3f", "box.p3f"])
def test_set_geometry_with_the_objects_own_numbers_changes_no_byte(scene):
    hs = p3d.HostScene(scene_path(scene), legacy_f11=scene in LEGACY)
    before = hs.arrays(bvh=True)
    objs = np.nonzero(before["prim_type"] != PLANE)[0].astype(np.uint32)
    assert len(objs)
    hs.set_geometry(objs, before["prim_v"][objs])
    after = hs.arrays(bvh=True)
    _same_bytes(before, after, PRIM_KEYS + BVH_KEYS, scene)
    assert before["bvh_max_depth"] == after["bvh_max_depth"]


@pytest.mark.parametrize("scene", ["balls_low.p3f", "tri_low.p3f", "box.p3f"])
def test_set_geometry_equals_the_loader(scene, tmp_path):
    """Every non-plane object moved by offsets that are exact in binary: the setter's objects, boxes and normals, and the host
    BVH built AFTER it, are those of the scene file with the same numbers (so the tree of the old positions was dropped)."""
    src = scene_path(scene)
    hs = p3d.HostScene(src, legacy_f11=scene in LEGACY)
    before = hs.arrays(bvh=True)  # builds the host BVH of the old positions
    objs = np.nonzero(before["prim_type"] != PLANE)[0].astype(np.uint32)
    offsets = np.array([(0.25, -1.5, 0.5), (-1.5, 0.25, 2.0), (0.125, 0.75, -0.25)], np.float32)[np.arange(len(objs)) % 3]
    new_v = translated(before["prim_type"], before["prim_v"], objs, offsets)
    hs.set_geometry(objs, new_v)
    moved = hs.arrays(bvh=True)
    loaded = p3d.HostScene(write_moved_p3f(src, str(tmp_path / scene), before["prim_type"], objs, new_v),
                           legacy_f11=scene in LEGACY).arrays(bvh=True)
    assert moved["prim_v"].tobytes() != before["prim_v"].tobytes()
    assert moved["prim_v"][objs].tobytes() == new_v.tobytes()
    _same_bytes(moved, loaded, PRIM_KEYS + BVH_KEYS, scene)
    assert moved["bvh_max_depth"] == loaded["bvh_max_depth"]
    # the rest of the descriptor is untouched
    _same_bytes(moved, before, ("materials", "lights", "background"), scene)


def test_host_refusals_change_nothing():
    hs = p3d.HostScene(os.path.join(ROOT, "scenes", "planes.p3f"))
    before = hs.arrays(bvh=True)
    planes = np.nonzero(before["prim_type"] == PLANE)[0]
    others = np.nonzero(before["prim_type"] != PLANE)[0]
    assert len(planes) and len(others)
    lib = p3d.lib()
    v = np.zeros((2, 9), np.float32)
    v[:] = np.arange(9) + 1
    obj = np.array([others[0], planes[0]], np.uint32)
    cases = [("a plane", (hs._h, 2, obj.ctypes.data, v.ctypes.data)),
             ("an index out of range", (hs._h, 2, np.array([others[0], before["n_prims"]], np.uint32).ctypes.data, v.ctypes.data)),
             ("null objects", (hs._h, 1, None, v.ctypes.data)),
             ("null floats", (hs._h, 1, obj.ctypes.data, None)),
             ("null scene", (None, 1, obj.ctypes.data, v.ctypes.data))]
    for what, args in cases:
        assert lib.p3d_host_scene_set_geometry(*args) == -1, what  # P3D_ERR_INVALID
        assert p3d.lib().p3d_last_error()
        _same_bytes(before, hs.arrays(bvh=True), PRIM_KEYS + BVH_KEYS, what)
    with pytest.raises(p3d.P3DError) as e:
        hs.set_geometry(planes[:1], before["prim_v"][planes[:1]])
    assert e.value.code == -1
    assert lib.p3d_host_scene_set_geometry(hs._h, 0, None, None) == 0  # nothing to do is not an error


def test_device_entry_points_refuse_a_null_scene_without_a_device():
    lib = p3d.lib()
    ms = C.c_float(7.0)
    assert lib.p3d_scene_update_prims(None, 0, None, None, p3d.UPDATE_REBUILD, C.byref(ms)) == -1
    n, m, depth = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.p3d_scene_export_bvh(None, None, C.byref(n), None, C.byref(m), C.byref(depth)) == -1
    assert b"null" in lib.p3d_last_error()
