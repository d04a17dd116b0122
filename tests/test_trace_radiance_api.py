"""Radiance along rays in device memory and a camera's rays (p3d_trace_radiance_device, p3d_camera_rays_device,
include/p3d_radiance.h, which include/p3d.h includes) without a GPU: the entry points are declared, exported and in the prototype table, a null scene is refused
with a message, and the tensor wrappers refuse what they cannot pass on before the library is called."""
import os
import re

import numpy as np
import pytest

from api_checks import scene_without_a_library
from conftest import ROOT
import p3d_amd as p3d


def test_header_declares_the_two_prototypes():
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    main, code = strip("p3d.h"), strip("p3d_radiance.h")
    assert re.search(r'#include\s+"p3d_radiance.h"', main)  # p3d.h brings the declarations along
    assert re.search(r"\bint\s+p3d_trace_radiance_device\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,"
                     r"\s*const\s+float\s*\*\s*\w+,\s*const\s+float\s*\*\s*\w+,\s*int32_t\s+\w+,\s*uint32_t\s+\w+,"
                     r"\s*float\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_camera_rays_device\s*\(\s*p3d_scene\s*\*\s*\w+,\s*const\s+p3d_camera\s*\*\s*\w+\s*,"
                     r"\s*const\s+p3d_tile\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+,\s*float\s*\*\s*\w+,\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_RADIANCE_MAX_DEPTH\s+16u?\b", code)
    assert re.search(r"#define\s+P3D_RADIANCE_SKYBOX\s+1u?\b", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)  # detected by the symbols


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in ("p3d_trace_radiance_device", "p3d_camera_rays_device"):
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES, name
    assert len(p3d.PROTOTYPES["p3d_trace_radiance_device"][1]) == 10 and len(p3d.PROTOTYPES["p3d_camera_rays_device"][1]) == 6
    assert lib.p3d_abi_version() == 4
    for name in ("trace_radiance_device", "camera_rays_device"):
        assert callable(getattr(p3d, name)), name
    assert p3d.RADIANCE_MAX_DEPTH == 16 and p3d.RADIANCE_SKYBOX == 1
    assert lib.p3d_trace_radiance_device(None, p3d.ACCEL_BVH, 4, None, None, 4, 0, None, None, None) == -1  # P3D_ERR_INVALID
    assert b"p3d_trace_radiance_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_trace_radiance_device(None, p3d.ACCEL_NONE, 0, None, None, 0, 0, None, None, None) == -1  # before n = 0 is looked at
    assert lib.p3d_camera_rays_device(None, None, None, None, None, None) == -1
    assert b"p3d_camera_rays_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def test_wrappers_refuse_bad_arguments_before_the_library():
    import torch
    dev = scene_without_a_library()
    dev.res = (8, 6)
    raw = (0x1000, 6)  # a raw (address, rows) pair is taken at its word
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    q = lambda *a, **kw: p3d.trace_radiance_device(dev, *a, **kw)
    cases = [
        ("a numpy origin", "origin: a CUDA/HIP torch.Tensor", lambda: q(p3d.ACCEL_BVH, np.zeros((6, 3), np.float32), raw, 4)),
        ("a numpy direction", "direction: a CUDA/HIP torch.Tensor", lambda: q(p3d.ACCEL_BVH, raw, np.zeros((6, 3), np.float32), 4)),
        ("a float64 origin", "origin: dtype", lambda: q(p3d.ACCEL_BVH, f32(6, 3).double(), raw, 4)),
        ("a float16 direction", "direction: dtype", lambda: q(p3d.ACCEL_BVH, raw, f32(6, 3).half(), 4)),
        ("an (n, 4) origin", "origin: shape", lambda: q(p3d.ACCEL_BVH, f32(6, 4), raw, 4)),
        ("a flat direction", "direction: shape", lambda: q(p3d.ACCEL_BVH, raw, f32(18), 4)),
        ("a non-contiguous origin", "origin: the tensor is not contiguous", lambda: q(p3d.ACCEL_BVH, f32(3, 6).t(), raw, 4)),
        ("a CPU origin", "origin: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, f32(6, 3), raw, 4)),
        ("a CPU direction", "direction: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, f32(6, 3), 4)),
        ("fewer directions", "6 origins, 5 directions", lambda: q(p3d.ACCEL_BVH, raw, (0x2000, 5), 4)),
        ("a null raw address", "raw pair", lambda: q(p3d.ACCEL_BVH, (0, 6), raw, 4)),
        ("max_depth -1", "max_depth must be 0 .. 16, got -1", lambda: q(p3d.ACCEL_BVH, raw, raw, -1)),
        ("max_depth 17", "max_depth must be 0 .. 16, got 17", lambda: q(p3d.ACCEL_BVH, raw, raw, 17)),
        ("an unknown flag bit", "unknown flag", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, flags=p3d.RADIANCE_SKYBOX | 2)),
        ("a CPU rgb", "out['rgb']: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, want=(), out={"rgb": f32(6, 3)})),
        ("an int rgb", "out['rgb']: dtype", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, want=(), out={"rgb": torch.zeros((6, 3), dtype=torch.int32)})),
        ("a float hit_id", "out['hit_id']: dtype", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, out={"rgb": (0x4000, 6), "hit_id": f32(6)})),
        ("a missing output", "out has no 'hit_id'", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, out={"rgb": (0x4000, 6)})),
        ("a short output", "5 rows for 6 rays", lambda: q(p3d.ACCEL_NONE, raw, raw, 4, want=(), out={"rgb": (0x4000, 5)})),
        ("an unknown output", "unknown output 't'", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, want=("t",))),
    ]
    c = lambda **kw: p3d.camera_rays_device(dev, **kw)
    cases += [
        ("CPU camera rays", "out['origin']: the tensor is in host memory", lambda: c(out={"origin": f32(48, 3), "direction": (0x5000, 48)})),
        ("float64 camera rays", "out['direction']: dtype", lambda: c(out={"origin": (0x5000, 48), "direction": f32(48, 3).double()})),
        ("(n, 4) camera rays", "out['origin']: shape", lambda: c(out={"origin": f32(48, 4), "direction": (0x5000, 48)})),
        ("a missing direction", "out has no 'direction'", lambda: c(out={"origin": (0x5000, 48)})),
        ("rows of another tile", "48 rows for 12 pixels", lambda: c(tile=p3d.Tile(1, 1, 4, 3, 0, 1), out={"origin": (0x5000, 48), "direction": (0x6000, 48)})),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
