"""The shading updates (include/p3d_shading.h) without a GPU: the header and the library's symbols, the rules of the Python
surface the seven entry points keep, the host setters on HostScene.arrays(), and the refusals that need no device."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import p3d_amd as p3d
from api_checks import header_code, scene_without_a_library
from conftest import scene_path
from frame_checks import CORNELL
from shading_update_checks import COL, KD, POS, host, light_rows, seeded, tables

NAMES = ("p3d_scene_set_materials", "p3d_scene_set_lights", "p3d_scene_materials", "p3d_scene_lights", "p3d_scene_set_shading_device",
         "p3d_host_scene_set_materials", "p3d_host_scene_set_lights")
FUNCTIONS = ("set_materials", "set_lights", "scene_materials", "scene_lights", "set_shading_device", "host_set_materials", "host_set_lights")
BALLS = scene_path("balls_low.p3f")


def same_arrays(a, b, but=()):
    """The keys of two HostScene.arrays() that differ in some byte, `but` aside"""
    assert a.keys() == b.keys()
    flat = lambda v: b"".join(np.asarray(x).tobytes() for x in v.values()) if isinstance(v, dict) else np.asarray(v).tobytes()
    return [k for k in a if k not in but and flat(a[k]) != flat(b[k])]


def test_the_header_declares_them():
    code, main = header_code("p3d_shading.h"), header_code()
    assert re.search(r'#include\s+"p3d_shading.h"', main) and re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)
    u32 = r"\s*uint32_t\s+\w+\s*,"
    for name, scene, record, const in (("p3d_scene_set_materials", "p3d_scene", "p3d_material", True), ("p3d_scene_set_lights", "p3d_scene", "p3d_light", True),
                                       ("p3d_scene_materials", "p3d_scene", "p3d_material", False), ("p3d_scene_lights", "p3d_scene", "p3d_light", False),
                                       ("p3d_host_scene_set_materials", "p3d_host_scene", "p3d_material", True),
                                       ("p3d_host_scene_set_lights", "p3d_host_scene", "p3d_light", True)):
        array = (r"\s*const\s+" if const else r"\s*") + record + r"\s*\*\s*\w+\s*\)"
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*(struct\s+)?" + scene + r"\s*\*\s*\w+," + u32 + u32 + array, code), name
    cv = r"\s*const\s+void\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_scene_set_shading_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 + u32 + cv + u32 + u32 + cv + r"\s*void\s*\*\s*\w+\)", code)


def test_the_surface_rules():
    lib = p3d.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    assert [len(p3d.PROTOTYPES[name][1]) for name in NAMES] == [4, 4, 4, 4, 8, 4, 4]
    assert lib.p3d_abi_version() == 4
    assert C.sizeof(p3d.Material) == 4 * p3d.MATERIAL_FLOATS == 64 and C.sizeof(p3d.Light) == 4 * p3d.LIGHT_FLOATS == 32
    record = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "python_api_surface.json")))
    classes = [k for k, v in record["names"].items() if v["kind"] in ("class", "structure")]
    assert "DeviceScene" in classes and "HostScene" in classes
    for fn in FUNCTIONS:
        assert callable(getattr(p3d, fn)), fn
        for cls in classes:
            assert not hasattr(getattr(p3d, cls), fn), "%s is a member of the recorded class %s" % (fn, cls)


@pytest.mark.parametrize("path", [BALLS, CORNELL])
def test_the_scenes_own_numbers_change_no_byte(path):
    hs = host(path)
    before = hs.arrays(bvh=True, grid=True)
    p3d.host_set_materials(hs, 0, before["materials"])  # arrays()["materials"] passed back unchanged
    p3d.host_set_lights(hs, 0, before["lights"])        # (n, 6): position then colour
    p3d.host_set_lights(hs, 0, light_rows(before["lights"]))
    assert same_arrays(before, hs.arrays(bvh=True, grid=True)) == []


def test_new_numbers_change_exactly_the_named_rows():
    hs = host(BALLS)
    before = hs.arrays(bvh=True, grid=True)
    mats, lights = tables(hs)
    new_m, new_l = seeded(mats, lights, 5)
    new_m[:, 9:16] = [0.25, 1.5, 0.125, 0.5, 0.75, 1.0, 9.0]  # every field arrives where it belongs; reserved is not kept
    p3d.host_set_materials(hs, 1, new_m[1:2])
    p3d.host_set_lights(hs, 1, new_l[1:3])
    after = hs.arrays(bvh=True, grid=True)  # the tree and the grid built before the change stand
    assert same_arrays(before, after, but=("materials", "lights")) == []
    want_m = mats.copy()
    want_m[1] = new_m[1]
    want_m[1, 15] = 0
    assert after["materials"].tobytes() == want_m.tobytes()
    want_l = before["lights"].copy()
    want_l[1:3, 0:3], want_l[1:3, 3:6] = new_l[1:3, POS], new_l[1:3, COL]
    assert after["lights"].tobytes() == want_l.tobytes() and not np.array_equal(want_l[1:3], before["lights"][1:3])
    assert after["lights"][0].tobytes() == before["lights"][0].tobytes()


def test_after_replicate_lights_the_indices_are_the_replicated_ones():
    hs = host(BALLS)
    n = hs.arrays()["n_lights"]
    hs.replicate_lights(2, 0.5)
    before = hs.arrays()
    assert before["n_lights"] == 4 * n
    row = np.array([[9, 8, 7, 0.1, 0.2, 0.3]], np.float32)
    p3d.host_set_lights(hs, 4 * n - 1, row)
    after = hs.arrays()
    assert after["lights"][-1].tobytes() == row[0].tobytes() and after["lights"][:-1].tobytes() == before["lights"][:-1].tobytes()
    assert same_arrays(before, after, but=("lights",)) == []
    with pytest.raises(p3d.P3DError):
        p3d.host_set_lights(hs, 4 * n, row)


def test_refusals_that_need_no_device():
    hs = host(BALLS)
    before = hs.arrays(bvh=True, grid=True)
    mats, lights = tables(hs)
    L = p3d.lib()
    for what, word, call in [
        ("materials past the end", "ends behind", lambda: p3d.host_set_materials(hs, 1, mats)),
        ("lights past the end", "ends behind", lambda: p3d.host_set_lights(hs, len(lights), lights[:1])),
        ("a first that does not fit", "first must be", lambda: p3d.host_set_lights(hs, -1, lights[:1])),
        ("materials of 15 columns", "needed: (n, 16)", lambda: p3d.host_set_materials(hs, 0, mats[:, :15])),
        ("a flat material", "needed: (n, 16)", lambda: p3d.host_set_materials(hs, 0, mats[0])),
        ("lights of 7 columns", "needed: (n, 8) or (n, 6)", lambda: p3d.host_set_lights(hs, 0, lights[:, :7])),
    ]:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
    # a null array with n > 0, a null scene: the raw library
    assert L.p3d_host_scene_set_materials(hs._h, 0, 1, None) == -1 and b"null array" in L.p3d_last_error()
    assert L.p3d_host_scene_set_lights(hs._h, 0, 1, None) == -1 and b"null array" in L.p3d_last_error()
    assert L.p3d_host_scene_set_materials(None, 0, 1, mats.ctypes.data) == -1 and L.p3d_host_scene_set_lights(None, 0, 1, lights.ctypes.data) == -1
    assert L.p3d_host_scene_set_materials(hs._h, len(mats), 0, None) == 0 and L.p3d_host_scene_set_lights(hs._h, 0, 0, None) == 0  # n = 0
    assert same_arrays(before, hs.arrays(bvh=True, grid=True)) == []
    # the device entry points refuse a null scene before anything else
    for name in NAMES[:4]:
        assert getattr(L, name)(None, 0, 1, mats.ctypes.data) == -1 and name.encode() in L.p3d_last_error() and b"null scene" in L.p3d_last_error()
    assert L.p3d_scene_set_shading_device(None, 0, 0, None, 0, 0, None, None) == -1 and b"null scene" in L.p3d_last_error()


def test_wrappers_refuse_bad_arguments_before_the_library():
    import torch
    dev = scene_without_a_library()
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    for what, word, call in [
        ("materials of 15 columns", "needed: (n, 16)", lambda: p3d.set_materials(dev, 0, np.zeros((2, 15), np.float32))),
        ("lights of 5 columns", "needed: (n, 8) or (n, 6)", lambda: p3d.set_lights(dev, 0, np.zeros((2, 5), np.float32))),
        ("a negative count", "n must not be negative", lambda: p3d.scene_materials(dev, 0, -1)),
        ("numpy materials", "materials: a CUDA/HIP torch.Tensor", lambda: p3d.set_shading_device(dev, materials=np.zeros((2, 16), np.float32))),
        ("CPU materials", "materials: the tensor is in host memory", lambda: p3d.set_shading_device(dev, materials=f32(2, 16))),
        ("float64 lights", "lights: dtype", lambda: p3d.set_shading_device(dev, lights=f32(2, 8).double())),
        ("lights of 6 columns on the device", "lights: shape", lambda: p3d.set_shading_device(dev, lights=f32(2, 6))),
        ("materials of 3 dimensions", "materials: shape", lambda: p3d.set_shading_device(dev, materials=f32(1, 2, 16))),
    ]:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
