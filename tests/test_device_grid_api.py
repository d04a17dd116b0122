"""The device-built uniform grid (p3d_scene_build_grid / p3d_scene_export_grid, include/p3d.h) without a GPU: the entry
points are declared, exported and wrapped, the ABI version is untouched, null arguments are refused with a message, and
DeviceScene refuses grid="device" on a scene kind that cannot have one before it touches a device."""
import ctypes as C
import os
import re

import pytest

from api_checks import header_code
from conftest import ROOT, scene_path
import p3d_amd as p3d

SYMBOLS = ["p3d_scene_build_grid", "p3d_scene_export_grid"]


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    code = header_code()
    assert re.search(r"\bint\s+p3d_scene_build_grid\s*\(\s*p3d_scene\s*\*\s*\w+,\s*float\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+p3d_scene_export_grid\s*\(\s*p3d_scene\s*\*\s*\w+,\s*p3d_grid_desc\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+,"
                     r"\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)
    # the stated limit is in the header's text
    assert "2^28" in open(os.path.join(ROOT, "include", "p3d.h")).read()


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4
    for name in ("build_grid", "export_grid"):
        assert hasattr(p3d.DeviceScene, name), name


def test_null_arguments_are_refused_with_a_message():
    lib = p3d.lib()
    ms = C.c_float(7.0)
    assert lib.p3d_scene_build_grid(None, C.byref(ms)) == -1
    assert b"p3d_scene_build_grid" in lib.p3d_last_error() and b"null" in lib.p3d_last_error()
    assert lib.p3d_scene_build_grid(None, None) == -1
    info = p3d.GridDesc()
    n, m = C.c_uint32(0), C.c_uint32(0)
    assert lib.p3d_scene_export_grid(None, C.byref(info), None, C.byref(n), None, C.byref(m)) == -1
    assert b"p3d_scene_export_grid" in lib.p3d_last_error() and b"null" in lib.p3d_last_error()
    assert ms.value == 7.0 and (n.value, m.value) == (0, 0)


@pytest.mark.parametrize("bvh", [True, False])
def test_grid_device_needs_bvh_device(bvh):
    """Refused by the wrapper itself, before any device call: p3d_scene_create fails with -2 where there is no device"""
    hs = p3d.HostScene(scene_path("balls_low.p3f"))
    with pytest.raises(p3d.P3DError) as e:
        p3d.DeviceScene(hs, bvh=bvh, grid="device")
    assert e.value.code == -1 and 'bvh="device"' in str(e.value)
