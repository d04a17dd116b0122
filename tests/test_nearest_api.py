"""Nearest-surface queries (p3d_host_scene_nearest, p3d_nearest_device, include/p3d.h) without a GPU: the entry points are
declared, exported and wrapped, a null scene is refused by name, and the tensor wrapper refuses what it cannot pass on before
the library is called."""
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
import p3d_amd as p3d


def test_header_declares_the_prototypes():
    code = header_code()
    cf, f, i32 = r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_nearest_device\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s+\w+," + cf + cf + i32 + f + f + f
                     + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_host_scene_nearest\s*\(\s*p3d_host_scene\s*\*\s*\w+,\s*uint32_t\s+\w+," + cf + cf + i32 + f
                     + r"\s*float\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in ("p3d_host_scene_nearest", "p3d_nearest_device"):
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4
    assert callable(p3d.DeviceScene.nearest_device) and callable(p3d.HostScene.nearest)
    assert lib.p3d_nearest_device(None, p3d.ACCEL_BVH, 4, None, None, None, None, None, None, None) == -1  # P3D_ERR_INVALID
    assert b"p3d_nearest_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_nearest_device(None, p3d.ACCEL_NONE, 0, None, None, None, None, None, None, None) == -1
    assert lib.p3d_host_scene_nearest(None, 0, None, None, None, None, None) == -1
    assert b"p3d_host_scene_nearest" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def test_the_wrapper_refuses_bad_arguments_before_the_library():
    import torch
    dev = scene_without_a_library()
    q = dev.nearest_device
    raw = (0x1000, 6)  # a raw (address, rows) pair is taken at its word
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    cases = [
        ("numpy points", "points: a CUDA/HIP torch.Tensor", lambda: q(p3d.ACCEL_BVH, np.zeros((6, 3), np.float32))),
        ("a numpy limit", "max_dist: a CUDA/HIP torch.Tensor", lambda: q(p3d.ACCEL_BVH, raw, max_dist=np.zeros(6, np.float32))),
        ("float64 points", "points: dtype", lambda: q(p3d.ACCEL_BVH, f32(6, 3).double())),
        ("a float64 limit", "max_dist: dtype", lambda: q(p3d.ACCEL_BVH, raw, max_dist=f32(6).double())),
        ("(n, 4) points", "points: shape", lambda: q(p3d.ACCEL_BVH, f32(6, 4))),
        ("flat points", "points: shape", lambda: q(p3d.ACCEL_BVH, f32(18))),
        ("an (n, 1) limit", "max_dist: shape", lambda: q(p3d.ACCEL_BVH, raw, max_dist=f32(6, 1))),
        ("non-contiguous points", "points: the tensor is not contiguous", lambda: q(p3d.ACCEL_BVH, f32(3, 6).t())),
        ("a strided limit", "max_dist: the tensor is not contiguous", lambda: q(p3d.ACCEL_BVH, raw, max_dist=f32(12)[::2])),
        ("CPU points", "points: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, f32(6, 3))),
        ("a CPU limit", "max_dist: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, max_dist=f32(6))),
        ("more limits", "6 points, 7 limits", lambda: q(p3d.ACCEL_BVH, raw, max_dist=(0x3000, 7))),
        ("a null raw address", "raw pair", lambda: q(p3d.ACCEL_BVH, (0, 6))),
        ("a raw pair without rows", "raw pair", lambda: q(p3d.ACCEL_BVH, (0x1000, 0))),
        # outputs the caller supplies are checked like the inputs
        ("a CPU object", "out['object']: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, want=(), out={"object": torch.zeros(6, dtype=torch.int32)})),
        ("a float object", "out['object']: dtype", lambda: q(p3d.ACCEL_BVH, raw, want=(), out={"object": f32(6)})),
        ("a missing output", "out has no 'dist'", lambda: q(p3d.ACCEL_BVH, raw, out={"object": (0x4000, 6)})),
        ("a short output", "5 rows for 6 points", lambda: q(p3d.ACCEL_NONE, raw, want=(), out={"object": (0x4000, 5)})),
        ("a flat closest", "out['closest']: shape", lambda: q(p3d.ACCEL_NONE, raw, want=("closest",), out={"object": (0x4000, 6), "closest": f32(18)})),
        ("an unknown output", "unknown output 'hit_point'", lambda: q(p3d.ACCEL_BVH, raw, want=("hit_point",))),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
