"""Path-traced radiance along rays in device memory and a camera's sample rays (p3d_trace_path_device,
p3d_camera_sample_rays_device, include/p3d_radiance.h) without a GPU: the entry points are declared, exported and in the
prototype table, a null scene is refused with a message, the tensor wrappers refuse what they cannot pass on before the
library is called, and the RNG state arithmetic tests/test_gpu_trace_path.py builds its states with is the oracle's."""
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
from oracle import binding as ob
import p3d_amd as p3d
from rng_reference import M64, next31, seed_stream


def test_header_declares_the_two_prototypes():
    code = header_code("p3d_radiance.h")
    main = header_code()
    f, u32, u64 = r"\s*float\s*\*\s*\w+\s*,", r"\s*uint32_t\s+\w+\s*,", r"\s*uint64_t\s*\*\s*\w+\s*,"
    cf = r"\s*const\s+float\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_trace_path_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 + u32 + cf + cf + r"\s*int32_t\s+\w+," + u32 + u32 +
                     r"\s*uint64_t\s+\w+," + u64 + u32 + f + r"\s*int32_t\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_camera_sample_rays_device\s*\(\s*p3d_scene\s*\*\s*\w+,\s*const\s+p3d_camera\s*\*\s*\w+\s*,"
                     r"\s*const\s+p3d_tile\s*\*\s*\w+\s*,\s*const\s+p3d_config\s*\*\s*\w+\s*," + u32 + f + f + u64 + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_PATH_ACCUMULATE\s+2u?\b", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)  # detected by the symbols


def test_library_exports_them_and_python_wraps_them():
    lib = p3d.lib()
    for name in ("p3d_trace_path_device", "p3d_camera_sample_rays_device"):
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    assert len(p3d.PROTOTYPES["p3d_trace_path_device"][1]) == 14 and len(p3d.PROTOTYPES["p3d_camera_sample_rays_device"][1]) == 9
    assert lib.p3d_abi_version() == 4
    for name in ("trace_path_device", "camera_sample_rays_device"):
        assert callable(getattr(p3d, name)), name
    assert p3d.PATH_ACCUMULATE == 2 and not p3d.PATH_ACCUMULATE & p3d.RADIANCE_SKYBOX
    assert lib.p3d_trace_path_device(None, p3d.ACCEL_BVH, 4, None, None, 4, 0, 1, 0, None, 0, None, None, None) == -1  # P3D_ERR_INVALID
    assert b"p3d_trace_path_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_trace_path_device(None, p3d.ACCEL_NONE, 0, None, None, 0, 0, 1, 0, None, 0, None, None, None) == -1  # before n = 0 is looked at
    assert lib.p3d_camera_sample_rays_device(None, None, None, None, 0, None, None, None, None) == -1
    assert b"p3d_camera_sample_rays_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def test_wrappers_refuse_bad_arguments_before_the_library():
    import torch
    dev = scene_without_a_library()
    dev.res = (8, 6)
    raw = (0x1000, 6)  # a raw (address, rows) pair is taken at its word
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    i64 = lambda *shape: torch.zeros(shape, dtype=torch.int64)
    q = lambda *a, **kw: p3d.trace_path_device(dev, *a, **kw)
    acc = p3d.PATH_ACCUMULATE
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
        ("max_depth -1", "max_depth must be 0 .. 1024, got -1", lambda: q(p3d.ACCEL_BVH, raw, raw, -1)),
        ("max_depth 1025", "max_depth must be 0 .. 1024, got 1025", lambda: q(p3d.ACCEL_BVH, raw, raw, 1025)),
        ("samples = 0", "samples must be at least 1", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, samples=0)),
        ("samples past 2^32", "sample_begin + samples", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, samples=2, sample_begin=0xffffffff)),
        ("an unknown flag bit", "unknown flag", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, flags=p3d.RADIANCE_SKYBOX | 4)),
        ("an (n, 3) rng", "rng: shape", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, rng=i64(6, 3))),
        ("a float rng", "rng: dtype", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, rng=f32(6, 2))),
        ("a float64 rng", "rng: dtype", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, rng=f32(6, 2).double())),
        ("a CPU rng", "rng: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, rng=i64(6, 2))),
        ("a non-contiguous rng", "rng: the tensor is not contiguous", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, rng=i64(2, 6).t())),
        ("fewer states", "6 rays, 5 rng states", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, rng=(0x3000, 5))),
        ("accumulate without out", "PATH_ACCUMULATE adds to out['rgb']", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, flags=acc)),
        ("accumulate without out['rgb']", "PATH_ACCUMULATE adds to out['rgb']", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, flags=acc, out={"hit_id": (0x4000, 6)})),
        ("a CPU rgb", "out['rgb']: the tensor is in host memory", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, want=(), out={"rgb": f32(6, 3)})),
        ("a float hit_id", "out['hit_id']: dtype", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, out={"rgb": (0x4000, 6), "hit_id": f32(6)})),
        ("a missing output", "out has no 'hit_id'", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, out={"rgb": (0x4000, 6)})),
        ("a short output", "5 rows for 6 rays", lambda: q(p3d.ACCEL_NONE, raw, raw, 4, want=(), out={"rgb": (0x4000, 5)})),
        ("an unknown output", "unknown output 't'", lambda: q(p3d.ACCEL_BVH, raw, raw, 4, want=("t",))),
    ]
    cfg = p3d.pathtrace_config(spp_sqrt=2)
    c = lambda **kw: p3d.camera_sample_rays_device(dev, cfg, 0, **kw)
    pair = (0x5000, 48)
    cases += [
        ("CPU sample rays", "out['origin']: the tensor is in host memory", lambda: c(out={"origin": f32(48, 3), "direction": pair, "rng": pair})),
        ("float64 sample rays", "out['direction']: dtype", lambda: c(out={"origin": pair, "direction": f32(48, 3).double(), "rng": pair})),
        ("an int32 rng", "out['rng']: dtype", lambda: c(out={"origin": pair, "direction": pair, "rng": torch.zeros((48, 2), dtype=torch.int32)})),
        ("an (n, 3) rng", "out['rng']: shape", lambda: c(out={"origin": pair, "direction": pair, "rng": i64(48, 3)})),
        ("a missing rng", "out has no 'rng'", lambda: c(out={"origin": pair, "direction": pair})),
        ("rows of another tile", "48 rows for 12 pixels", lambda: c(tile=p3d.Tile(1, 1, 4, 3, 0, 1), want=(), out={"origin": pair, "direction": pair})),
        ("an unknown output", "unknown output 'hit_id'", lambda: c(want=("hit_id",))),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)


def test_the_python_rng_is_the_oracles():
    """mix64, seed_stream and next31 above against oracle.binding.rng_stream: the states the GPU tests hand to the library"""
    for seed, pixel, sample in [(0, 0, 0), (0x5EED, 1919, 15), (M64, 0xffffffff, 0xffffffff), (0x0123456789ABCDEF, 40 * 48 + 7, 3), (7, 1, 0), (7, 0, 1)]:
        state, inc = seed_stream(seed, pixel, sample)
        assert inc & 1 and 0 <= state <= M64
        draws = []
        for _ in range(64):
            state, v = next31(state, inc)
            draws.append(v)
        assert draws == ob.rng_stream(seed, pixel, sample, 64).tolist(), (seed, pixel, sample)
        assert max(draws) < 1 << 31
    assert seed_stream(7, 1, 0) != seed_stream(7, 0, 1)
