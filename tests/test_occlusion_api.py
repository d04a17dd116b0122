"""Hemisphere occlusion (include/p3d_occlusion.h) without a GPU: the host writer of the rays, p3d_occlusion_rays, against the
float64 statement of tests/occlusion_reference.py; its split batches and split samples; the refusals that need no device; and
the rules of the Python surface the three entry points keep.

The bounds (64 points, 70 samples; every quantity is <= 1 in magnitude):
  direction   2^-19 per component: about a dozen float32 roundings precede the normalisation and three lie in it, 2^-24 each;
              that sum doubled, rounded up to a power of two
  origin      point + normal * bias in float32, bit for bit
  |direction| within 2^-22 of 1; direction . normal >= -2^-19
  mean cosine |mean(direction . normal) - 2/3| <= 0.02 over 4096 samples: five standard deviations of a cosine-weighted
              cosine (variance 1/18)"""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
from frame_checks import assert_bits
import intersect_reference as ref
import occlusion_reference as occ
import p3d_amd as p3d

SAMPLES, BEGIN, OFFSET, SEED = 70, 3, 7, 0xA0


def the_points():
    """64 points with unit normals (normalised in float32): the six axis normals, normals with |w.x| either side of 0.1 and at
    float32(0.1) itself, random ones"""
    rng = np.random.default_rng(11)
    axis = np.concatenate([np.eye(3), -np.eye(3)])
    near = np.array([[x, s * np.sqrt(1 - x * x) * 0.6, np.sqrt(1 - x * x) * 0.8] for x in (0.0999, 0.1001, -0.0999, -0.1001, 0.1, -0.1) for s in (1, -1)])
    rest = rng.standard_normal((64 - len(axis) - len(near), 3))
    normals = ref.normalize32(np.concatenate([axis, near, rest]).astype(np.float32))
    normals[len(axis) + 8, 0], normals[len(axis) + 10, 0] = np.float32(0.1), np.float32(-0.1)  # (the threshold itself; still unit to 1e-8)
    return rng.uniform(-2, 2, (64, 3)).astype(np.float32), normals


@pytest.fixture(scope="module")
def written():
    p, w = the_points()
    o, d = p3d.occlusion_rays(p, w, SAMPLES, sample_begin=BEGIN, seed=SEED, point_offset=OFFSET)
    return p, w, o, d


def test_the_host_writer_is_the_float64_rule(written):
    p, w, o, d = written
    assert o.shape == d.shape == (64 * SAMPLES, 3) and o.dtype == d.dtype == np.float32
    assert (np.abs(w[:, 0]) >= np.float32(0.1)).sum() > 8 and (np.abs(w[:, 0]) < np.float32(0.1)).sum() > 8
    want_o, want_d = occ.rays(p, w, SAMPLES, sample_begin=BEGIN, seed=SEED, point_offset=OFFSET)
    err = np.abs(d.astype(np.float64) - want_d).max()
    length = np.abs(np.sqrt((d.astype(np.float64) ** 2).sum(1)) - 1).max()
    cosine = (d.astype(np.float64) * np.repeat(w.astype(np.float64), SAMPLES, 0)).sum(1)
    print("direction: max |error| %.3g (2^-19 = %.3g); | |d| - 1 | %.3g (2^-22 = %.3g); min d.n %.3g" % (err, 2.0 ** -19, length, 2.0 ** -22, cosine.min()))
    assert err <= 2.0 ** -19
    assert_bits(o, want_o, "origin")
    assert length <= 2.0 ** -22
    assert cosine.min() >= -2.0 ** -19


def test_the_sampling_is_cosine_weighted():
    w = ref.normalize32(np.array([[0.3, -0.5, 0.8]], np.float32))
    _, d = p3d.occlusion_rays(np.zeros((1, 3), np.float32), w, 4096, seed=3)
    mean = float((d.astype(np.float64) @ w[0].astype(np.float64)).mean())
    print("mean cosine over 4096 samples: %.5f" % mean)
    assert abs(mean - 2.0 / 3.0) <= 0.02


def test_a_split_batch_and_split_samples_give_the_same_rows(written):
    p, w, o, d = written
    for a, b in ((0, 1), (1, 33), (33, 64)):
        po, pd = p3d.occlusion_rays(p[a:b], w[a:b], SAMPLES, sample_begin=BEGIN, seed=SEED, point_offset=OFFSET + a)
        assert_bits(po, o[a * SAMPLES:b * SAMPLES], "origin of points %d..%d" % (a, b))
        assert_bits(pd, d[a * SAMPLES:b * SAMPLES], "direction of points %d..%d" % (a, b))
    rows = d.reshape(64, SAMPLES, 3)
    for first, count in ((0, 32), (32, 38), (69, 1)):
        _, sd = p3d.occlusion_rays(p, w, count, sample_begin=BEGIN + first, seed=SEED, point_offset=OFFSET)
        assert_bits(sd.reshape(64, count, 3), rows[:, first:first + count], "samples %d..%d" % (first, first + count))
    _, other = p3d.occlusion_rays(p, w, SAMPLES, sample_begin=BEGIN, seed=SEED + 1, point_offset=OFFSET)
    assert (other != d).any(1).all(), "the seed changes nothing"


def test_a_degenerate_normal_gives_nan_rays():
    _, d = p3d.occlusion_rays(np.zeros((2, 3), np.float32), np.array([[0, 0, 0], [np.inf, 0, 0]], np.float32), 3)
    assert np.isnan(d).all()


def params(**kw):
    base = dict(seed=1, samples=4, sample_begin=0, point_offset=0, flags=0, bias=1e-4, team=0)
    base.update(kw)
    return p3d.OcclusionParams(**base)


def test_refusals_that_need_no_device():
    L = p3d.lib()
    p = np.zeros((2, 3), np.float32)
    out = np.full((8, 3), 7, np.float32)
    raw = lambda q, point=p.ctypes.data, origin=out.ctypes.data: L.p3d_occlusion_rays(2, point, p.ctypes.data, C.byref(q) if q else None, origin, out.ctypes.data)
    for what, word, q in [("samples = 0", "samples must be at least 1", params(samples=0)), ("team = 3", "team", params(team=3)),
                          ("team = 128", "team", params(team=128)), ("an unknown flag", "unknown flag", params(flags=2)),
                          ("a NaN bias", "bias", params(bias=float("nan"))), ("an infinite bias", "bias", params(bias=float("inf"))),
                          ("samples past 2^32", "2^32", params(sample_begin=0xffffffff, samples=2)), ("null params", "null params", None)]:
        assert raw(q) == -1, what
        assert b"p3d_occlusion_rays" in L.p3d_last_error() and word.encode() in L.p3d_last_error(), "%s: %s" % (what, L.p3d_last_error())
    assert raw(params(), point=None) == -1 and b"null argument" in L.p3d_last_error()
    assert raw(params(), origin=None) == -1 and b"null argument" in L.p3d_last_error()
    assert L.p3d_occlusion_rays(0x10000, p.ctypes.data, p.ctypes.data, C.byref(params(samples=0x10000)), out.ctypes.data, out.ctypes.data) == -4  # P3D_ERR_CAPACITY
    assert (out == 7).all(), "a refused call wrote"
    assert L.p3d_occlusion_rays(0, None, None, C.byref(params()), None, None) == 0  # n = 0
    assert raw(params(team=64, flags=p3d.OCCLUSION_ACCUMULATE)) == 0 and not (out == 7).any()
    # the device entry points refuse a null scene before anything else
    assert L.p3d_occlusion_device(None, p3d.ACCEL_BVH, 2, None, None, None, C.byref(params()), None, None, None) == -1
    assert b"p3d_occlusion_device" in L.p3d_last_error() and b"null scene" in L.p3d_last_error()
    assert L.p3d_occlusion_rays_device(None, 2, None, None, C.byref(params()), None, None, None) == -1
    assert b"p3d_occlusion_rays_device" in L.p3d_last_error() and b"null scene" in L.p3d_last_error()


def test_wrappers_refuse_bad_arguments_before_the_library():
    import torch
    dev = scene_without_a_library()
    raw = (0x1000, 6)
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    q = lambda *a, **kw: p3d.occlusion_device(dev, p3d.ACCEL_BVH, *a, **kw)
    r = lambda *a, **kw: p3d.occlusion_rays_device(dev, *a, **kw)
    acc = p3d.OCCLUSION_ACCUMULATE
    for what, word, call in [
        ("numpy points", "points: a CUDA/HIP torch.Tensor", lambda: q(np.zeros((6, 3), np.float32), raw, 4)),
        ("CPU normals", "normals: the tensor is in host memory", lambda: q(raw, f32(6, 3), 4)),
        ("float64 points", "points: dtype", lambda: q(f32(6, 3).double(), raw, 4)),
        ("fewer normals", "6 points, 5 normals", lambda: q(raw, (0x2000, 5), 4)),
        ("fewer limits", "6 points, 5 limits", lambda: q(raw, raw, 4, max_dist=(0x2000, 5))),
        ("a 2-d limit", "max_dist: shape", lambda: q(raw, raw, 4, max_dist=f32(6, 1))),
        ("samples = 0", "samples must be at least 1", lambda: q(raw, raw, 0)),
        ("samples past 2^32", "sample_begin + samples", lambda: q(raw, raw, 2, sample_begin=0xffffffff)),
        ("team = 3", "team must be 0", lambda: q(raw, raw, 4, team=3)),
        ("team = 128", "team must be 0", lambda: q(raw, raw, 4, team=128)),
        ("an unknown flag", "unknown flag", lambda: q(raw, raw, 4, flags=2)),
        ("a NaN bias", "bias must be finite", lambda: q(raw, raw, 4, bias=float("nan"))),
        ("a negative point_offset", "point_offset", lambda: q(raw, raw, 4, point_offset=-1)),
        ("accumulate without out", "OCCLUSION_ACCUMULATE adds", lambda: q(raw, raw, 4, flags=acc)),
        ("accumulate without out['bent']", "OCCLUSION_ACCUMULATE adds", lambda: q(raw, raw, 4, flags=acc, want=("bent",), out={"unoccluded": raw})),
        ("an unknown output", "unknown output 't'", lambda: q(raw, raw, 4, want=("t",))),
        ("a float count", "out['unoccluded']: dtype", lambda: q(raw, raw, 4, out={"unoccluded": f32(6)})),
        ("a short output", "5 rows for 6 points", lambda: q(raw, raw, 4, out={"unoccluded": (0x3000, 5)})),
        ("a missing output", "out has no 'bent'", lambda: q(raw, raw, 4, want=("bent",), out={"unoccluded": raw})),
        ("rays: samples = 0", "samples must be at least 1", lambda: r(raw, raw, 0)),
        ("rays: short rows", "6 rows for 24 rays", lambda: r(raw, raw, 4, out={"origin": raw, "direction": raw})),
        ("rays: CPU rows", "out['origin']: the tensor is in host memory", lambda: r(raw, raw, 4, out={"origin": f32(24, 3), "direction": (0x4000, 24)})),
        ("host rays: shapes", "needed: (n, 3) both", lambda: p3d.occlusion_rays(np.zeros((4, 3)), np.zeros((5, 3)), 2)),
        ("host rays: samples = 0", "samples must be at least 1", lambda: p3d.occlusion_rays(np.zeros((4, 3)), np.zeros((4, 3)), 0)),
    ]:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)


def test_the_surface_rules():
    names = ("p3d_occlusion_device", "p3d_occlusion_rays_device", "p3d_occlusion_rays")
    lib = p3d.lib()
    for name in names:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    assert [len(p3d.PROTOTYPES[name][1]) for name in names] == [10, 8, 6]
    assert lib.p3d_abi_version() == 4
    assert C.sizeof(p3d.OcclusionParams) == 32 and p3d.OCCLUSION_ACCUMULATE == 1
    record = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "python_api_surface.json")))
    classes = [k for k, v in record["names"].items() if v["kind"] in ("class", "structure")]
    assert "DeviceScene" in classes and "HostScene" in classes
    for fn in ("occlusion_device", "occlusion_rays_device", "occlusion_rays"):
        assert callable(getattr(p3d, fn)), fn
        for cls in classes:
            assert not hasattr(getattr(p3d, cls), fn), "%s is a member of the recorded class %s" % (fn, cls)


def test_the_header_declares_them():
    code, main = header_code("p3d_occlusion.h"), header_code()
    assert re.search(r'#include\s+"p3d_occlusion.h"', main) and re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)
    assert re.search(r"#define\s+P3D_OCCLUSION_ACCUMULATE\s+1u?\b", code)
    fields = re.search(r"typedef\s+struct\s+p3d_occlusion_params\s*\{(.*?)\}\s*p3d_occlusion_params\s*;", code, re.S).group(1)
    assert re.findall(r"(\w+)\s+(\w+)\s*;", fields) == [("uint64_t", "seed"), ("uint32_t", "samples"), ("uint32_t", "sample_begin"), ("uint32_t", "point_offset"),
                                                        ("uint32_t", "flags"), ("float", "bias"), ("uint32_t", "team")]
    cf, f, par = r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*const\s+p3d_occlusion_params\s*\*\s*\w+\s*,"
    u32 = r"\s*uint32_t\s+\w+\s*,"
    assert re.search(r"\bint\s+p3d_occlusion_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 + u32 + cf + cf + cf + par + r"\s*uint32_t\s*\*\s*\w+\s*," + f + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_occlusion_rays_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 + cf + cf + par + f + f + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_occlusion_rays\s*\(" + u32 + cf + cf + par + f + r"\s*float\s*\*\s*\w+\s*\)", code)
