"""The pose of a rigged live scene from device matrices on the caller's stream (p3d_scene_set_rig, p3d_scene_rig,
p3d_scene_pose_device, include/p3d.h) without a GPU: the entry points are declared, exported and wrapped, and the tensor
wrapper refuses what it cannot pass on before the library is called, with the checks of the other device-buffer wrappers
(test_device_geometry_api.py, test_stream_refit_api.py)."""
import inspect
import os
import re

import numpy as np
import pytest

from api_checks import scene_without_a_library
from conftest import ROOT
import p3d_amd as p3d

NAMES = ("p3d_scene_set_rig", "p3d_scene_rig", "p3d_scene_pose_device")


def test_header_declares_the_entry_points():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p3d.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+p3d_scene_set_rig\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*const\s+p3d_xform_range\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s+\w+\)", code)
    assert re.search(r"\bint\s+p3d_scene_rig\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+,\s*uint32_t\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_scene_pose_device\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*const\s+void\s*\*\s*\w+,"
                     r"\s*const\s+void\s*\*\s*\w+,\s*void\s*\*\s*\w+\)", code)
    # detected by their symbols: the version and the modes stay
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)
    assert re.search(r"P3D_UPDATE_REFIT\s*=\s*0\s*,\s*P3D_UPDATE_REBUILD\s*=\s*1\s*\}", code)


def test_library_exports_them():
    lib = p3d.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4
    assert lib.p3d_scene_pose_device(None, 0, None, None, None) == -1  # P3D_ERR_INVALID
    assert lib.p3d_last_error().startswith(b"p3d_scene_pose_device: null scene")
    assert lib.p3d_scene_set_rig(None, 0, None, 0) == -1
    assert lib.p3d_last_error().startswith(b"p3d_scene_set_rig: null scene")
    assert lib.p3d_scene_rig(None, None, None, None) == -1
    assert lib.p3d_last_error().startswith(b"p3d_scene_rig")


def test_python_wraps_them():
    for name, args in (("set_rig", ["self", "ranges", "n_xforms"]), ("rig", ["self"]),
                       ("pose_device", ["self", "xforms", "sphere_scale", "stream"])):
        f = getattr(p3d.DeviceScene, name)
        assert callable(f), name
        assert list(inspect.signature(f).parameters) == args, name
    sig = inspect.signature(p3d.DeviceScene.pose_device)
    assert sig.parameters["stream"].default == 0
    assert sig.parameters["sphere_scale"].default is None


def test_the_wrapper_refuses_bad_tensors_before_the_library():
    import torch
    dev = scene_without_a_library()
    good = (0x1000, 4)  # a raw pair is taken at its word: the fault is in the other argument
    cases = [
        ("a CPU tensor", "host memory", lambda: dev.pose_device(torch.zeros((4, 3, 4), dtype=torch.float32))),
        ("a CPU [K, 12] tensor", "host memory", lambda: dev.pose_device(torch.zeros((4, 12), dtype=torch.float32), stream=0)),
        ("a float64 tensor", "dtype", lambda: dev.pose_device(torch.zeros((4, 3, 4), dtype=torch.float64))),
        ("a float16 [K, 12] tensor", "dtype", lambda: dev.pose_device(torch.zeros((4, 12), dtype=torch.float16))),
        ("a non-contiguous [K, 12] tensor", "contiguous", lambda: dev.pose_device(torch.zeros((12, 4), dtype=torch.float32).t())),
        ("a non-contiguous [K, 3, 4] tensor", "contiguous", lambda: dev.pose_device(torch.zeros((4, 4, 3), dtype=torch.float32).transpose(1, 2))),
        ("a [K, 3, 3] shape", "shape", lambda: dev.pose_device(torch.zeros((4, 3, 3), dtype=torch.float32))),
        ("a [K, 9] shape", "shape", lambda: dev.pose_device(torch.zeros((4, 9), dtype=torch.float32))),
        ("a flat shape", "shape", lambda: dev.pose_device(torch.zeros(48, dtype=torch.float32))),
        ("no transforms", "shape", lambda: dev.pose_device(torch.zeros((0, 3, 4), dtype=torch.float32))),
        ("a numpy array", "torch.Tensor", lambda: dev.pose_device(np.zeros((4, 3, 4), np.float32))),
        ("a null raw address", "raw pair", lambda: dev.pose_device((0, 4))),
        ("a raw pair without rows", "raw pair", lambda: dev.pose_device((0x1000, 0))),
        ("CPU scales", "sphere_scale: the tensor is in host memory", lambda: dev.pose_device(good, torch.ones(4, dtype=torch.float32))),
        ("float64 scales", "sphere_scale: dtype", lambda: dev.pose_device(good, torch.ones(4, dtype=torch.float64))),
        ("[K, 1] scales", "sphere_scale: shape", lambda: dev.pose_device(good, torch.ones((4, 1), dtype=torch.float32))),
        ("strided scales", "sphere_scale: the tensor is not contiguous", lambda: dev.pose_device(good, torch.ones(8, dtype=torch.float32)[::2])),
        ("numpy scales", "torch.Tensor", lambda: dev.pose_device(good, np.ones(4, np.float32))),
        ("a null raw address for the scales", "raw pair", lambda: dev.pose_device(good, (0, 4))),
        ("scales of another length", "sphere_scale: 5 values for 4 transforms", lambda: dev.pose_device(good, (0x2000, 5), stream=0)),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
