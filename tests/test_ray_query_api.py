"""Ray queries over device buffers (p3d_trace_closest_device, p3d_trace_any_device, include/p3d.h) without a GPU: the entry
points are declared, exported and wrapped, a null scene is refused with a message, and the tensor wrappers refuse what they
cannot pass on before the library is called."""
import ctypes as C
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
import p3d_amd as p3d


def test_header_declares_the_two_prototypes():
    code = header_code()
    rays = r"p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*uint32_t\s+\w+,\s*const\s+float\s*\*\s*\w+,\s*const\s+float\s*\*\s*\w+,\s*const\s+float\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_trace_closest_device\s*\(\s*" + rays + r"\s*int32_t\s*\*\s*\w+,\s*float\s*\*\s*\w+,\s*float\s*\*\s*\w+,"
                     r"\s*float\s*\*\s*\w+,\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_trace_any_device\s*\(\s*" + rays + r"\s*uint8_t\s*\*\s*\w+,\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in ("p3d_trace_closest_device", "p3d_trace_any_device"):
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4
    for name in ("trace_closest_device", "trace_any_device"):
        assert callable(getattr(p3d.DeviceScene, name)), name
    assert lib.p3d_trace_any_device(None, p3d.ACCEL_NONE, 0, None, None, None, None, None) == -1  # P3D_ERR_INVALID
    assert b"p3d_trace_any_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_trace_closest_device(None, p3d.ACCEL_BVH, 4, None, None, None, None, None, None, None, None) == -1
    assert b"p3d_trace_closest_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def test_wrappers_refuse_bad_rays_before_the_library():
    import torch
    dev = scene_without_a_library()
    raw = (0x1000, 6)  # a raw (address, rows) pair is taken at its word
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    queries = {"closest": dev.trace_closest_device, "any": dev.trace_any_device}
    for kind, q in queries.items():
        cases = [
            ("a numpy origin", "origin: a CUDA/HIP torch.Tensor", lambda: q(p3d.ACCEL_BVH, np.zeros((6, 3), np.float32), raw)),
            ("a numpy direction", "direction: a CUDA/HIP torch.Tensor", lambda: q(p3d.ACCEL_BVH, raw, np.zeros((6, 3), np.float32))),
            ("a float64 origin", "origin: dtype", lambda: q(p3d.ACCEL_BVH, f32(6, 3).double(), raw)),
            ("a float64 t_max", "t_max: dtype", lambda: q(p3d.ACCEL_BVH, raw, raw, t_max=f32(6).double())),
            ("an (n, 4) origin", "origin: shape", lambda: q(p3d.ACCEL_BVH, f32(6, 4), raw)),
            ("an (n, 4) direction", "direction: shape", lambda: q(p3d.ACCEL_BVH, raw, f32(6, 4))),
            ("an (n, 1) t_max", "t_max: shape", lambda: q(p3d.ACCEL_BVH, raw, raw, t_max=f32(6, 1))),
            ("a non-contiguous origin", "origin: the tensor is not contiguous", lambda: q(p3d.ACCEL_BVH, f32(3, 6).t(), raw)),
            ("a strided t_max", "t_max: the tensor is not contiguous", lambda: q(p3d.ACCEL_BVH, raw, raw, t_max=f32(12)[::2])),
            ("a CPU origin", "origin: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, f32(6, 3), raw)),
            ("a CPU direction", "direction: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, f32(6, 3))),
            ("a CPU t_max", "t_max: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, raw, t_max=f32(6))),
            ("fewer directions", "6 origins, 5 directions", lambda: q(p3d.ACCEL_BVH, raw, (0x2000, 5))),
            ("fewer limits", "6 origins, 6 directions, 7 limits", lambda: q(p3d.ACCEL_BVH, raw, raw, t_max=(0x3000, 7))),
            ("a null raw address", "raw pair", lambda: q(p3d.ACCEL_BVH, (0, 6), raw)),
        ]
        for what, word, call in cases:
            with pytest.raises(p3d.P3DError) as e:
                call()
            assert e.value.code == -1 and word in str(e.value), "%s, %s: %s" % (kind, what, e.value)
    # outputs the caller supplies are checked like the inputs
    out_cases = [
        ("a CPU hit_id", "out['hit_id']: the tensor is in host memory",
         lambda: dev.trace_closest_device(p3d.ACCEL_BVH, raw, raw, want=(), out={"hit_id": torch.zeros(6, dtype=torch.int32)})),
        ("a float hit_id", "out['hit_id']: dtype",
         lambda: dev.trace_closest_device(p3d.ACCEL_BVH, raw, raw, want=(), out={"hit_id": f32(6)})),
        ("a missing output", "out has no 't'", lambda: dev.trace_closest_device(p3d.ACCEL_BVH, raw, raw, out={"hit_id": (0x4000, 6)})),
        ("a short output", "5 rows for 6 rays", lambda: dev.trace_any_device(p3d.ACCEL_NONE, raw, raw, out={"occluded": (0x4000, 5)})),
        ("an unknown output", "unknown output 'colour'", lambda: dev.trace_closest_device(p3d.ACCEL_BVH, raw, raw, want=("colour",))),
    ]
    for what, word, call in out_cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
