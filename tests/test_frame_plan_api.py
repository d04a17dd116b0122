"""The read-only view of a launch's plan (p3d_debug_frame_plan, csrc/p3d_debug.h) without a GPU: the entry point is
declared in the private header and not in include/p3d.h, exported and wrapped, null arguments are refused with a message,
and p3d_debug_plan has the same size and fields in C and in ctypes."""
import ctypes as C
import os
import re

from api_checks import header_code
from conftest import ROOT
import p3d_amd as p3d

FIELDS = ["pt", "literal", "lds_scene", "lds_spill", "sub4", "per_level", "repair_tiles", "stack_mode", "spill_entries", "bound", "cap",
          "zero_weight_reflections"]


def _debug_header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "p3d-raytracer_amd", "csrc", "p3d_debug.h")).read(), flags=re.S)


def test_private_header_declares_it_and_the_public_one_does_not():
    code = _debug_header()
    assert re.search(r"\bint\s+p3d_debug_frame_plan\s*\(\s*p3d_scene\s*\*\s*\w+,\s*const\s+p3d_config\s*\*\s*\w+,\s*const\s+p3d_tile\s*\*\s*\w+,"
                     r"\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*p3d_debug_plan\s*\*\s*\w+\s*\)\s*;", code)
    assert re.search(r"\buint32_t\s+p3d_debug_frame_plan_size\s*\(\s*void\s*\)\s*;", code)
    assert "p3d_debug" not in header_code()
    assert "p3d_debug_frame_plan" not in p3d.EXPORTS  # EXPORTS is include/p3d.h


def test_library_exports_it_and_python_wraps_it():
    lib = p3d.lib()
    assert hasattr(lib, "p3d_debug_frame_plan") and hasattr(lib, "p3d_debug_frame_plan_size")
    assert hasattr(p3d.DeviceScene, "frame_plan")
    assert p3d.FramePlan._fields == tuple(FIELDS)
    assert set(p3d.PLAN_MODES) == {"frame", "adaptive", "features"}
    for name, value in re.findall(r"#define\s+P3D_DEBUG_PLAN_(\w+)\s+(\d+)u", _debug_header()):
        assert p3d.PLAN_MODES[name.lower()] == int(value)


def test_struct_size_and_fields_agree_between_c_and_ctypes():
    assert p3d.lib().p3d_debug_frame_plan_size() == C.sizeof(p3d.DebugPlan) == 4 * len(FIELDS)
    body = re.search(r"typedef\s+struct\s+p3d_debug_plan\s*\{(.*?)\}\s*p3d_debug_plan\s*;", _debug_header(), flags=re.S).group(1)
    declared = [n for line in re.findall(r"uint32_t\s+([^;]+);", body) for n in re.split(r"\s*,\s*", line.strip())]
    assert declared == FIELDS == [k for k, _ in p3d.DebugPlan._fields_]
    assert all(t is C.c_uint32 for _, t in p3d.DebugPlan._fields_)


def test_null_arguments_are_refused_with_a_message():
    lib = p3d.lib()
    cfg, tile, out = p3d.whitted_config(), p3d.Tile(0, 0, 8, 8, 0, 1), p3d.DebugPlan()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    for args in ((None, C.byref(cfg), C.byref(tile), 0, 1, 0, C.byref(out)), (None, None, None, 0, 1, 0, None)):
        assert lib.p3d_debug_frame_plan(*args) == -1
        assert b"p3d_debug_frame_plan" in lib.p3d_last_error() and b"null" in lib.p3d_last_error()
    assert bytes(out) == b"\xab" * C.sizeof(out)  # nothing written on a refusal
