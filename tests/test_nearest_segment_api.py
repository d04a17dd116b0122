"""Nearest surfaces to a segment (include/p3d_segment.h) without a GPU: the entry points are declared, exported and wrapped as
functions; what the wrappers and the host form refuse; and the bound the tree is culled with, p3d_debug_segment_box_d2, against
the rule: never above the rule's d2 for anything in the box, once the cull's slack is allowed for."""
import re

import numpy as np
import pytest
import torch

from api_checks import header_code, scene_without_a_library
from device_query_contract import INVALID, UNSUPPORTED
import intersect_reference as ref
import p3d_amd as p3d

SLACK = 1.0 + 2.0 ** -10  # kNearestSlack


def test_the_header_declares_them():
    code, main = header_code("p3d_segment.h"), header_code()
    assert re.search(r'#include\s+"p3d_segment.h"', main) and re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)
    cf, f, i32, u32 = r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,", r"\s*uint32_t\s+\w+\s*,"
    filt = r"\s*const\s+int32_t\s*\*\s*\w+\s*," + u32 + r"\s*const\s+int32_t\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_nearest_segment_k_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 * 3 + cf * 3 + filt + i32 * 2 + f * 5 + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_host_scene_nearest_segment_k\s*\(\s*p3d_host_scene\s*\*\s*\w+," + u32 * 2 + cf * 3 + filt + i32 * 2 + f * 3 + r"\s*float\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+p3d_debug_segment_box_d2\s*\(" + u32 + cf * 4 + r"\s*float\s*\*\s*\w+\s*\)", code)
    assert "box" in open(p3d.HERE + "/../include/p3d_segment.h").read()  # (the header says that a box is left for later)


def test_the_library_exports_them_and_python_wraps_them_as_functions():
    names = ("p3d_nearest_segment_k_device", "p3d_host_scene_nearest_segment_k")
    lib = p3d.lib()
    for name in names:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    assert hasattr(lib, "p3d_debug_segment_box_d2") and "p3d_debug_segment_box_d2" not in p3d.EXPORTS + p3d.EXPORTS_ADDED
    assert [len(p3d.PROTOTYPES[name][1]) for name in names] == [18, 15]
    assert lib.p3d_abi_version() == 4
    for fn in ("nearest_segment_k_device", "host_nearest_segment_k"):
        assert callable(getattr(p3d, fn)), fn
        assert not hasattr(p3d.DeviceScene, fn) and not hasattr(p3d.HostScene, fn), fn
    assert lib.p3d_nearest_segment_k_device(None, p3d.ACCEL_BVH, 4, 2, None, None, None, None, 0, None, *([None] * 8)) == INVALID
    assert b"p3d_nearest_segment_k_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_host_scene_nearest_segment_k(None, 0, 2, None, None, None, None, 0, None, *([None] * 6)) == INVALID
    assert b"p3d_host_scene_nearest_segment_k" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def _refused(code, word, call):
    with pytest.raises(p3d.P3DError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_the_device_wrapper_refuses_without_a_library():
    """shapes, dtypes, where the tensors live, k and the grid: the library is not called (scene_without_a_library fails on any use)"""
    dev = scene_without_a_library()
    good = (0x1000, 5)  # a raw (address, rows) pair is taken at its word
    ask = lambda a=good, b=good, k=2, accel=p3d.ACCEL_BVH, **kw: p3d.nearest_segment_k_device(dev, accel, a, b, k, **kw)
    _refused(INVALID, "a: shape", lambda: ask(a=torch.zeros(5, 4)))
    _refused(INVALID, "b: shape", lambda: ask(b=torch.zeros(5)))
    _refused(INVALID, "a: dtype", lambda: ask(a=torch.zeros(5, 3, dtype=torch.float64)))
    _refused(INVALID, "host memory", lambda: ask(a=torch.zeros(5, 3)))
    _refused(INVALID, "not contiguous", lambda: ask(b=torch.zeros(3, 5).t()))
    _refused(INVALID, "a CUDA/HIP torch.Tensor", lambda: ask(a=np.zeros((5, 3), np.float32)))
    _refused(INVALID, "5 a rows, 6 b rows", lambda: ask(b=(0x2000, 6)))
    _refused(INVALID, "limits", lambda: ask(max_dist=(0x3000, 4)))
    _refused(INVALID, "max_dist: shape", lambda: ask(max_dist=torch.zeros(5, 1)))
    _refused(INVALID, "skip: shape", lambda: ask(skip=torch.zeros(5, dtype=torch.int32)))
    _refused(INVALID, "skip: dtype", lambda: ask(skip=torch.zeros(5, 2, dtype=torch.int64)))
    _refused(INVALID, "needs n_skip", lambda: ask(skip=(0x4000, 5)))
    _refused(INVALID, "skip ranges", lambda: ask(skip_range=(0x5000, 4)))
    _refused(INVALID, "unknown output", lambda: ask(want=("t",)))
    for k in (0, 17, -1):
        _refused(INVALID, "k must be 1 .. 16", lambda: ask(k=k))
    _refused(UNSUPPORTED, "grid", lambda: ask(accel=p3d.ACCEL_GRID))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("segment_api")
    plain, boxed = tmp / "plain.p3f", tmp / "boxed.p3f"
    plain.write_text(ref.HEAD + "s 4 0 0 1\np 3\n0 0 0\n2 0 0\n0 2 0\n")
    boxed.write_text(ref.HEAD + "s 4 0 0 1\nbox -1 3 -1 1 7 2\n")
    return p3d.HostScene(str(plain)), p3d.HostScene(str(boxed))


def test_the_host_form_refuses(scenes):
    hs, boxed = scenes
    a, b = np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32)
    for k in (0, 17):
        _refused(INVALID, "k must be 1 .. P3D_NEAREST_K_MAX", lambda: p3d.host_nearest_segment_k(hs, a, b, k))
    _refused(INVALID, "n_skip must be", lambda: p3d.host_nearest_segment_k(hs, a, b, 1, skip=np.zeros((3, 9), np.int32)))
    _refused(INVALID, "n_skip must be", lambda: p3d.host_nearest_segment_k(hs, a[:0], b[:0], 1, skip=np.zeros((0, 9), np.int32)))
    _refused(INVALID, "needed: (n, 3) both", lambda: p3d.host_nearest_segment_k(hs, a, b[:2], 1))
    _refused(INVALID, "limits", lambda: p3d.host_nearest_segment_k(hs, a, b, 1, max_dist=np.ones(2, np.float32)))
    _refused(INVALID, "skip_range", lambda: p3d.host_nearest_segment_k(hs, a, b, 1, skip_range=np.zeros((3, 3), np.int32)))
    for n in (3, 0):
        _refused(UNSUPPORTED, "is a box", lambda: p3d.host_nearest_segment_k(boxed, a[:n], b[:n], 1))
    # the device wrapper refuses the box and a plane under the tree by the host scene it came from, before any call
    dev = scene_without_a_library()
    dev.host = boxed
    _refused(UNSUPPORTED, "holds a box", lambda: p3d.nearest_segment_k_device(dev, p3d.ACCEL_NONE, (0x1000, 3), (0x2000, 3), 1))


def test_an_empty_batch(scenes):
    hs, _ = scenes
    none = np.zeros((0, 3), np.float32)
    count, obj, dist, param, on_segment, closest = p3d.host_nearest_segment_k(hs, none, none, 4)
    assert count.shape == (0,) and obj.shape == (0, 4) and dist.shape == (0, 4) and param.shape == (0, 4)
    assert on_segment.shape == (0, 4, 3) and closest.shape == (0, 4, 3)
    assert p3d.segment_box_d2(none, none, none, none).shape == (0,)
    lib = p3d.lib()
    assert lib.p3d_host_scene_nearest_segment_k(hs._h, 0, 17, None, None, None, None, 0, None, *([None] * 6)) == INVALID  # k, whatever n
    assert lib.p3d_host_scene_nearest_segment_k(hs._h, 2, 1, None, None, None, None, 0, None, *([None] * 6)) == INVALID
    assert b"null array" in lib.p3d_last_error()
    assert lib.p3d_debug_segment_box_d2(2, None, None, None, None, None) == INVALID


# ---- the bound ------------------------------------------------------------------------------------------------------------------

PAIRS, PER_SCENE = 20000, 9  # a scene of nine triangles: the eight on a segment's skip list leave ONE, whichever it is


def test_the_bound_never_exceeds_the_rule(tmp_path):
    """20 000 seeded pairs of a segment and a triangle, the box being the triangle's own: bound <= dist^2 * kNearestSlack, dist
    from the host form with every other triangle of the scene filtered out.  Evaluated in float64; dist is the float32 square
    root of the float32 d2 the cull compares: two roundings of 2^-24 each, which its square carries twice: (1 + 2^-24)^4.  No
    violation is allowed and no pair is left out"""
    rng = np.random.default_rng(977)
    n_scenes = 12
    per = -(-PAIRS // n_scenes)
    worst, pairs, touching, crossing, apart = 0.0, 0, 0, 0, 0
    for scene in range(n_scenes):
        centre = rng.uniform(-50, 50, (PER_SCENE, 1, 3))
        size = np.exp(rng.uniform(np.log(0.01), np.log(20.0), (PER_SCENE, 1, 1)))
        tri = centre + size * rng.uniform(-1, 1, (PER_SCENE, 3, 3))
        path = tmp_path / ("bound_%d.p3f" % scene)
        path.write_text(ref.HEAD + "".join("p 3\n" + "".join("%.9g %.9g %.9g\n" % tuple(v) for v in t) for t in tri))
        hs = p3d.HostScene(str(path))
        v = hs.arrays()["prim_v"][:, :9].reshape(PER_SCENE, 3, 3).astype(np.float32)  # the float32 vertices the rule sees
        lo, hi = v.min(1), v.max(1)
        j = rng.integers(0, PER_SCENE, per)
        extent = np.linalg.norm(hi - lo, axis=1)[j].astype(np.float64)
        # half long, half short against the box; starts from inside the box to three extents away; every eighth runs through
        # the box's centre, every eighth starts on a face
        length = extent * np.where(np.arange(per) % 2 == 0, np.exp(rng.uniform(np.log(0.5), np.log(5.0), per)), np.exp(rng.uniform(np.log(1e-3), np.log(0.1), per)))
        mid = ((lo + hi) / 2)[j].astype(np.float64)
        a = mid + (extent * np.exp(rng.uniform(np.log(1e-2), np.log(3.0), per)))[:, None] * ref._unit(rng, per)
        on_face = np.arange(per) % 8 == 3
        a[on_face, 0] = hi[j][on_face, 0]
        d = ref._unit(rng, per)
        through = np.arange(per) % 8 == 5
        d[through] = (mid - a)[through] / np.maximum(np.linalg.norm(mid - a, axis=1), 1e-30)[through, None]
        b = a + d * length[:, None]
        a, b = a.astype(np.float32), b.astype(np.float32)
        skip = np.array([[i for i in range(PER_SCENE) if i != t][:8] for t in j], np.int32)
        count, obj, dist, _, _, _ = p3d.host_nearest_segment_k(hs, a, b, 1, skip=skip)
        assert (count == 1).all() and (obj[:, 0] == j).all()
        bound = p3d.segment_box_d2(a, b, lo[j], hi[j]).astype(np.float64)
        allowed = dist[:, 0].astype(np.float64) ** 2 * SLACK * (1.0 + 2.0 ** -24) ** 4
        bad = np.nonzero(~(bound <= allowed))[0]
        assert len(bad) == 0, "scene %d: %d violations, first: pair %d, bound %.9g against dist %.9g" % (scene, len(bad), bad[0], bound[bad[0]], dist[bad[0], 0])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(allowed > 0, bound / allowed, 0.0))))
        pairs += per
        touching += int((bound == 0).sum())
        crossing += int((dist[:, 0] == 0).sum())
        apart += int((bound > 0).sum())
    print("%d pairs: %d with a bound of 0 (the extents overlap), %d at distance 0, %d apart; the largest bound / allowed is %.6f" % (pairs, touching, crossing, apart, worst))
    assert pairs >= PAIRS and touching > pairs // 20 and apart > pairs // 4 and crossing > 50
