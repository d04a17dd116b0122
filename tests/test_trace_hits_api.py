"""The hits in order along a ray (p3d_trace_hits_device, include/p3d.h) without a GPU: the entry point and its constant are
declared, exported and wrapped, a null scene is refused by name, and the tensor wrapper refuses what it
cannot pass on before the library is called."""
import os
import re

import numpy as np
import pytest

from api_checks import scene_without_a_library
from conftest import ROOT
import p3d_amd as p3d

NO_ARGS = (None,) * 10  # the ten pointers behind (scene, accel, n, k)


def test_header_declares_the_prototype():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p3d.h")).read(), flags=re.S)
    u32, cf, f, i32 = r"\s*uint32_t\s+\w+\s*,", r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_trace_hits_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 + u32 + u32 + cf + cf + cf + i32 + i32 + i32 + f + f + f
                     + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_TRACE_HITS_K_MAX\s+16u\b", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)
    # the caveat is stated where the call is declared: total counts objects, not crossings
    text = open(os.path.join(ROOT, "include", "p3d.h")).read()
    start = text.index("The HITS IN ORDER along a ray")
    assert "total counts OBJECTS, not crossings" in text[start:text.index("#define P3D_TRACE_HITS_K_MAX")]


def test_library_exports_it_and_python_wraps_it():
    lib = p3d.lib()
    assert hasattr(lib, "p3d_trace_hits_device") and "p3d_trace_hits_device" in p3d.EXPORTS
    assert lib.p3d_abi_version() == 4 and p3d.TRACE_HITS_K_MAX == 16
    assert callable(p3d.DeviceScene.trace_hits_device)
    assert lib.p3d_trace_hits_device(None, p3d.ACCEL_BVH, 4, 2, *NO_ARGS) == -1  # P3D_ERR_INVALID
    assert b"p3d_trace_hits_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_trace_hits_device(None, p3d.ACCEL_NONE, 0, 0, *NO_ARGS) == -1


def test_the_wrapper_refuses_bad_arguments_before_the_library():
    import torch
    dev = scene_without_a_library()
    q = dev.trace_hits_device
    B, N = p3d.ACCEL_BVH, p3d.ACCEL_NONE
    raw = (0x1000, 6)  # a raw (address, rows) pair is taken at its word
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    both = {"count": (0x4000, 6), "object": (0x5000, 6)}
    cases = [
        ("a numpy origin", "origin: a CUDA/HIP torch.Tensor", lambda: q(B, np.zeros((6, 3), np.float32), raw, 4)),
        ("a numpy direction", "direction: a CUDA/HIP torch.Tensor", lambda: q(B, raw, np.zeros((6, 3), np.float32), 4)),
        ("a numpy limit", "t_max: a CUDA/HIP torch.Tensor", lambda: q(B, raw, raw, 4, t_max=np.zeros(6, np.float32))),
        ("a float64 origin", "origin: dtype", lambda: q(B, f32(6, 3).double(), raw, 4)),
        ("a float64 limit", "t_max: dtype", lambda: q(B, raw, raw, 4, t_max=f32(6).double())),
        ("an (n, 4) direction", "direction: shape", lambda: q(B, raw, f32(6, 4), 4)),
        ("a flat origin", "origin: shape", lambda: q(B, f32(18), raw, 4)),
        ("an (n, 1) limit", "t_max: shape", lambda: q(B, raw, raw, 4, t_max=f32(6, 1))),
        ("a non-contiguous origin", "origin: the tensor is not contiguous", lambda: q(B, f32(3, 6).t(), raw, 4)),
        ("a strided limit", "t_max: the tensor is not contiguous", lambda: q(B, raw, raw, 4, t_max=f32(12)[::2])),
        ("a CPU origin", "origin: the tensor is in host memory", lambda: q(B, f32(6, 3), raw, 4)),
        ("a CPU limit", "t_max: the tensor is in host memory", lambda: q(B, raw, raw, 4, t_max=f32(6))),
        ("fewer directions", "6 origins, 5 directions", lambda: q(B, raw, (0x2000, 5), 4)),
        ("more limits", "6 origins, 6 directions, 7 limits", lambda: q(B, raw, raw, 4, t_max=(0x3000, 7))),
        ("a null raw address", "raw pair", lambda: q(B, (0, 6), raw, 4)),
        ("k = 17 with outputs to allocate", "k must be 0 .. 16", lambda: q(B, raw, raw, 17)),
        ("k = -1", "k must be 0 .. 16", lambda: q(B, raw, raw, -1, out=both)),
        ("k = 0 without total", "want must hold 'total'", lambda: q(B, raw, raw, 0)),
        ("k = 0 without total, with outputs", "want must hold 'total'", lambda: q(N, raw, raw, 0, want=("count", "object"), out=both)),
        # outputs the caller supplies are checked like the inputs, with the shapes of this k
        ("a CPU count", "out['count']: the tensor is in host memory", lambda: q(B, raw, raw, 4, want=(), out={"count": i32(6), "object": (0x5000, 6)})),
        ("a float count", "out['count']: dtype", lambda: q(B, raw, raw, 4, want=(), out={"count": f32(6), "object": (0x5000, 6)})),
        ("an (n, k) count", "out['count']: shape", lambda: q(B, raw, raw, 4, want=(), out={"count": i32(6, 4), "object": (0x5000, 6)})),
        ("a float object", "out['object']: dtype", lambda: q(B, raw, raw, 4, want=(), out={"count": (0x4000, 6), "object": f32(6, 4)})),
        ("an object of another k", "out['object']: shape", lambda: q(B, raw, raw, 4, want=(), out={"count": (0x4000, 6), "object": i32(6, 5)})),
        ("a missing count", "out has no 'count'", lambda: q(B, raw, raw, 4, want=(), out={"object": (0x5000, 6)})),
        ("a missing output", "out has no 't'", lambda: q(B, raw, raw, 4, out=both)),
        ("a missing total", "out has no 'total'", lambda: q(B, raw, raw, 4, want=("total",), out=both)),
        ("a missing total, k = 0", "out has no 'total'", lambda: q(B, raw, raw, 0, want=("total",), out=both)),
        ("a float total", "out['total']: dtype", lambda: q(N, raw, raw, 0, want=("total",), out={"total": f32(6)})),
        ("an (n, k) total", "out['total']: shape", lambda: q(N, raw, raw, 4, want=("total",), out=dict(both, total=i32(6, 4)))),
        ("a short total", "5 rows for 6 rays", lambda: q(N, raw, raw, 0, want=("total",), out={"total": (0x4000, 5)})),
        ("a short object", "5 rows for 6 rays", lambda: q(N, raw, raw, 4, want=(), out=dict(both, object=(0x5000, 5)))),
        ("a t of another k", "out['t']: shape", lambda: q(N, raw, raw, 4, want=("t",), out=dict(both, t=f32(6, 3)))),
        ("an (n, 3) hit_point", "out['hit_point']: shape", lambda: q(N, raw, raw, 4, want=("hit_point",), out=dict(both, hit_point=f32(6, 3)))),
        ("a transposed normal", "out['normal']: the tensor is not contiguous",
         lambda: q(N, raw, raw, 3, want=("normal",), out=dict(both, normal=f32(6, 3, 3).transpose(1, 2)))),
        ("a CPU hit_point", "out['hit_point']: the tensor is in host memory", lambda: q(N, raw, raw, 4, want=("hit_point",), out=dict(both, hit_point=f32(6, 4, 3)))),
        ("an unknown output", "unknown output 'closest'", lambda: q(B, raw, raw, 4, want=("closest",))),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
