"""The k-nearest queries (p3d_host_scene_nearest_k, p3d_nearest_k_device, include/p3d.h) without a GPU: the entry points are
declared, exported and wrapped, a null scene and a bad k are refused by name, and the tensor wrapper refuses what it cannot
pass on before the library is called."""
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
import p3d_amd as p3d


def test_header_declares_the_prototypes():
    code = header_code()
    u32, cf, f, i32 = r"\s*uint32_t\s+\w+\s*,", r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_nearest_k_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 + u32 + u32 + cf + cf + i32 + i32 + f + f + f
                     + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_host_scene_nearest_k\s*\(\s*p3d_host_scene\s*\*\s*\w+," + u32 + u32 + cf + cf + i32 + i32 + f
                     + r"\s*float\s*\*\s*\w+\s*\)", code)
    assert re.search(r"#define\s+P3D_NEAREST_K_MAX\s+16u\b", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in ("p3d_host_scene_nearest_k", "p3d_nearest_k_device"):
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS, name
    assert lib.p3d_abi_version() == 4 and p3d.NEAREST_K_MAX == 16
    assert callable(p3d.DeviceScene.nearest_k_device) and callable(p3d.HostScene.nearest_k)
    assert lib.p3d_nearest_k_device(None, p3d.ACCEL_BVH, 4, 2, None, None, None, None, None, None, None, None) == -1  # P3D_ERR_INVALID
    assert b"p3d_nearest_k_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_nearest_k_device(None, p3d.ACCEL_NONE, 0, 2, None, None, None, None, None, None, None, None) == -1
    assert lib.p3d_host_scene_nearest_k(None, 0, 2, None, None, None, None, None, None) == -1
    assert b"p3d_host_scene_nearest_k" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def test_the_wrapper_refuses_bad_arguments_before_the_library():
    import torch
    dev = scene_without_a_library()
    q = dev.nearest_k_device
    B, N = p3d.ACCEL_BVH, p3d.ACCEL_NONE
    raw = (0x1000, 6)  # a raw (address, rows) pair is taken at its word
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    both = {"count": (0x4000, 6), "object": (0x5000, 6)}
    cases = [
        ("numpy points", "points: a CUDA/HIP torch.Tensor", lambda: q(B, np.zeros((6, 3), np.float32), 4)),
        ("a numpy limit", "max_dist: a CUDA/HIP torch.Tensor", lambda: q(B, raw, 4, max_dist=np.zeros(6, np.float32))),
        ("float64 points", "points: dtype", lambda: q(B, f32(6, 3).double(), 4)),
        ("a float64 limit", "max_dist: dtype", lambda: q(B, raw, 4, max_dist=f32(6).double())),
        ("(n, 4) points", "points: shape", lambda: q(B, f32(6, 4), 4)),
        ("flat points", "points: shape", lambda: q(B, f32(18), 4)),
        ("an (n, 1) limit", "max_dist: shape", lambda: q(B, raw, 4, max_dist=f32(6, 1))),
        ("non-contiguous points", "points: the tensor is not contiguous", lambda: q(B, f32(3, 6).t(), 4)),
        ("a strided limit", "max_dist: the tensor is not contiguous", lambda: q(B, raw, 4, max_dist=f32(12)[::2])),
        ("CPU points", "points: the tensor is in host memory", lambda: q(B, f32(6, 3), 4)),
        ("a CPU limit", "max_dist: the tensor is in host memory", lambda: q(B, raw, 4, max_dist=f32(6))),
        ("more limits", "6 points, 7 limits", lambda: q(B, raw, 4, max_dist=(0x3000, 7))),
        ("a null raw address", "raw pair", lambda: q(B, (0, 6), 4)),
        ("a raw pair without rows", "raw pair", lambda: q(B, (0x1000, 0), 4)),
        ("k = 0 with outputs to allocate", "k must be 1 .. 16", lambda: q(B, raw, 0)),
        ("k = 17 with outputs to allocate", "k must be 1 .. 16", lambda: q(B, raw, 17)),
        # outputs the caller supplies are checked like the inputs, with the shapes of this k
        ("a CPU count", "out['count']: the tensor is in host memory", lambda: q(B, raw, 4, want=(), out={"count": i32(6), "object": (0x5000, 6)})),
        ("a float count", "out['count']: dtype", lambda: q(B, raw, 4, want=(), out={"count": f32(6), "object": (0x5000, 6)})),
        ("an (n, k) count", "out['count']: shape", lambda: q(B, raw, 4, want=(), out={"count": i32(6, 4), "object": (0x5000, 6)})),
        ("a CPU object", "out['object']: the tensor is in host memory", lambda: q(B, raw, 4, want=(), out={"count": (0x4000, 6), "object": i32(6, 4)})),
        ("a float object", "out['object']: dtype", lambda: q(B, raw, 4, want=(), out={"count": (0x4000, 6), "object": f32(6, 4)})),
        ("an object of another k", "out['object']: shape", lambda: q(B, raw, 4, want=(), out={"count": (0x4000, 6), "object": i32(6, 5)})),
        ("a flat object", "out['object']: shape", lambda: q(B, raw, 4, want=(), out={"count": (0x4000, 6), "object": i32(24)})),
        ("a missing count", "out has no 'count'", lambda: q(B, raw, 4, want=(), out={"object": (0x5000, 6)})),
        ("a missing output", "out has no 'dist'", lambda: q(B, raw, 4, out=both)),
        ("a short count", "5 rows for 6 points", lambda: q(N, raw, 4, want=(), out=dict(both, count=(0x4000, 5)))),
        ("a short object", "5 rows for 6 points", lambda: q(N, raw, 4, want=(), out=dict(both, object=(0x5000, 5)))),
        ("an (n, k) dist of another k", "out['dist']: shape", lambda: q(N, raw, 4, want=("dist",), out=dict(both, dist=f32(6, 3)))),
        ("an (n, 3) closest", "out['closest']: shape", lambda: q(N, raw, 4, want=("closest",), out=dict(both, closest=f32(6, 3)))),
        ("an (n, 3, k) closest", "out['closest']: shape", lambda: q(N, raw, 4, want=("closest",), out=dict(both, closest=f32(6, 3, 4)))),
        ("a transposed normal", "out['normal']: the tensor is not contiguous",
         lambda: q(N, raw, 3, want=("normal",), out=dict(both, normal=f32(6, 3, 3).transpose(1, 2)))),
        ("a CPU closest", "out['closest']: the tensor is in host memory", lambda: q(N, raw, 4, want=("closest",), out=dict(both, closest=f32(6, 4, 3)))),
        ("an unknown output", "unknown output 'hit_point'", lambda: q(B, raw, 4, want=("hit_point",))),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
