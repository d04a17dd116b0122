"""Overlap queries (include/p3d_overlap.h) without a GPU: the entry points are declared, exported and wrapped as functions, and
what the wrappers and the host form refuse."""
import re

import numpy as np
import pytest
import torch

from api_checks import header_code, scene_without_a_library
from device_query_contract import INVALID, UNSUPPORTED
import intersect_reference as ref
import p3d_amd as p3d

NAMES = ("p3d_overlap_box_device", "p3d_host_scene_overlap_box")


def test_the_header_declares_them():
    code, main = header_code("p3d_overlap.h"), header_code()
    assert re.search(r'#include\s+"p3d_segment.h"\s*#include\s+"p3d_overlap.h"', main), "p3d.h includes it below p3d_segment.h"
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)
    assert re.search(r"#define\s+P3D_OVERLAP_SOLID\s+1u?\b", code)
    cf, i32, u32 = r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,", r"\s*uint32_t\s+\w+\s*,"
    filt = r"\s*const\s+int32_t\s*\*\s*\w+\s*," + u32 + r"\s*const\s+int32_t\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_overlap_box_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 * 3 + cf * 2 + filt + u32 + i32 * 2 + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_host_scene_overlap_box\s*\(\s*p3d_host_scene\s*\*\s*\w+," + u32 * 2 + cf * 2 + filt + u32 + i32 + r"\s*int32_t\s*\*\s*\w+\s*\)", code)


def test_the_library_exports_them_and_python_wraps_them_as_functions():
    lib = p3d.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    assert [len(p3d.PROTOTYPES[name][1]) for name in NAMES] == [13, 11]
    assert lib.p3d_abi_version() == 4
    for fn in ("overlap_box_device", "host_overlap_box", "_overlap_outputs"):
        assert callable(getattr(p3d, fn)), fn
        assert not hasattr(p3d.DeviceScene, fn) and not hasattr(p3d.HostScene, fn), fn
    assert p3d._overlap_outputs(0) == {"total": ("int32", None)} and p3d._overlap_outputs(3) == {"total": ("int32", None), "object": ("int32", 3)}
    assert lib.p3d_overlap_box_device(None, p3d.ACCEL_BVH, 4, 2, None, None, None, 0, None, 0, None, None, None) == INVALID
    assert b"p3d_overlap_box_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_host_scene_overlap_box(None, 0, 2, None, None, None, 0, None, 0, None, None) == INVALID
    assert b"p3d_host_scene_overlap_box" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


def _refused(code, word, call):
    with pytest.raises(p3d.P3DError) as e:
        call()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_the_device_wrapper_refuses_without_a_library():
    """shapes, dtypes, where the tensors live, k and the grid: the library is not called (scene_without_a_library fails on any use)"""
    dev = scene_without_a_library()
    good = (0x1000, 5)  # a raw (address, rows) pair is taken at its word
    ask = lambda lo=good, hi=good, k=2, accel=p3d.ACCEL_BVH, **kw: p3d.overlap_box_device(dev, accel, lo, hi, k, **kw)
    _refused(INVALID, "lo: shape", lambda: ask(lo=torch.zeros(5, 4)))
    _refused(INVALID, "hi: shape", lambda: ask(hi=torch.zeros(5)))
    _refused(INVALID, "lo: dtype", lambda: ask(lo=torch.zeros(5, 3, dtype=torch.float64)))
    _refused(INVALID, "host memory", lambda: ask(lo=torch.zeros(5, 3)))
    _refused(INVALID, "not contiguous", lambda: ask(hi=torch.zeros(3, 5).t()))
    _refused(INVALID, "a CUDA/HIP torch.Tensor", lambda: ask(lo=np.zeros((5, 3), np.float32)))
    _refused(INVALID, "5 lo rows, 6 hi rows", lambda: ask(hi=(0x2000, 6)))
    _refused(INVALID, "skip: shape", lambda: ask(skip=torch.zeros(5, dtype=torch.int32)))
    _refused(INVALID, "skip: dtype", lambda: ask(skip=torch.zeros(5, 2, dtype=torch.int64)))
    _refused(INVALID, "needs n_skip", lambda: ask(skip=(0x4000, 5)))
    _refused(INVALID, "skip ranges", lambda: ask(skip_range=(0x5000, 4)))
    for k in (17, -1):
        _refused(INVALID, "k must be 0 .. 16", lambda: ask(k=k))
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        _refused(INVALID, "out has no 'total'", lambda: ask(k=0, accel=accel, out={}))  # k = 0 passes the wrapper's own checks
    _refused(UNSUPPORTED, "grid", lambda: ask(accel=p3d.ACCEL_GRID))


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("overlap_api")
    plain, planed = tmp / "plain.p3f", tmp / "planed.p3f"
    plain.write_text(ref.HEAD + "s 4 0 0 1\np 3\n0 0 0\n2 0 0\n0 2 0\nbox -1 3 -1 1 7 2\n")
    planed.write_text(ref.HEAD + "s 4 0 0 1\npl 0 0 0\n1 0 0\n0 1 0\n")
    return p3d.HostScene(str(plain)), p3d.HostScene(str(planed))


def test_the_host_form_refuses(scenes):
    hs, planed = scenes
    lo, hi = np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32)
    for k in (17, -1):
        _refused(INVALID, "k must be 0 .. P3D_NEAREST_K_MAX", lambda: p3d.host_overlap_box(hs, lo, hi, k))
    _refused(INVALID, "n_skip must be", lambda: p3d.host_overlap_box(hs, lo, hi, 1, skip=np.zeros((3, 9), np.int32)))
    _refused(INVALID, "n_skip must be", lambda: p3d.host_overlap_box(hs, lo[:0], hi[:0], 1, skip=np.zeros((0, 9), np.int32)))
    _refused(INVALID, "needed: (n, 3) both", lambda: p3d.host_overlap_box(hs, lo, hi[:2], 1))
    _refused(INVALID, "needed: (n, 3) both", lambda: p3d.host_overlap_box(hs, lo[:, :2], hi[:, :2], 1))
    _refused(INVALID, "skip_range", lambda: p3d.host_overlap_box(hs, lo, hi, 1, skip_range=np.zeros((3, 3), np.int32)))
    _refused(INVALID, "skip", lambda: p3d.host_overlap_box(hs, lo, hi, 1, skip=np.zeros((2, 1), np.int32)))
    lib = p3d.lib()
    total, obj = np.full(3, 77, np.int32), np.full((3, 1), 77, np.int32)
    raw = lambda n, k, flags, t=total, o=obj, scene=hs: lib.p3d_host_scene_overlap_box(
        scene._h, n, k, lo.ctypes.data, hi.ctypes.data, None, 0, None, flags, t.ctypes.data if t is not None else None, o.ctypes.data if o is not None else None)
    for flags in (2, 3, 0x80000000):  # an unknown bit, alone or next to the known one, whatever n
        for n in (3, 0):
            assert raw(n, 1, flags) == INVALID and b"unknown flag" in lib.p3d_last_error()
    assert raw(0, 17, 0) == INVALID and b"k must be" in lib.p3d_last_error()  # k, whatever n
    assert raw(3, 1, 0, t=None) == INVALID and b"null array" in lib.p3d_last_error()
    assert raw(3, 1, 0, o=None) == INVALID and b"null array" in lib.p3d_last_error()
    assert (total == 77).all() and (obj == 77).all(), "a refused call wrote"
    assert raw(3, 0, 1, o=None) == 0 and (obj == 77).all(), "k = 0 needs no object array and writes none"
    assert list(total) == [1, 1, 1]  # the unit box at the origin holds the triangle's corner; the sphere and the box lie apart
    # the device wrapper refuses a plane under the tree by the host scene it came from, before any call; the brute force takes it
    dev = scene_without_a_library()
    dev.host = planed
    _refused(UNSUPPORTED, "plane", lambda: p3d.overlap_box_device(dev, p3d.ACCEL_BVH, (0x1000, 3), (0x2000, 3), 1))
    with pytest.raises(AssertionError, match="the library was called"):
        p3d.overlap_box_device(dev, p3d.ACCEL_NONE, (0x1000, 3), (0x2000, 3), 0, out={"total": (0x3000, 3)})
    total, obj = p3d.host_overlap_box(planed, lo, hi, 2)
    assert list(total) == [1, 1, 1] and (obj == [1, -1]).all()  # the plane z = 0 touches the unit box's bottom face


def test_an_empty_batch_and_the_count_alone(scenes):
    hs, _ = scenes
    none = np.zeros((0, 3), np.float32)
    total, obj = p3d.host_overlap_box(hs, none, none, 4)
    assert total.shape == (0,) and obj.shape == (0, 4) and total.dtype == obj.dtype == np.int32
    lo, hi = np.array([[-5, -5, -5], [3.5, -0.25, -0.25]], np.float32), np.array([[9, 9, 9], [4.5, 0.25, 0.25]], np.float32)
    total, obj = p3d.host_overlap_box(hs, lo, hi, 0)
    assert obj.shape == (2, 0) and list(total) == [3, 0]  # everything; and a box wholly inside the sphere's shell
    total, obj = p3d.host_overlap_box(hs, lo, hi, 2, solid=True)
    assert list(total) == [3, 1] and obj.tolist() == [[0, 1], [0, -1]]
    total, obj = p3d.host_overlap_box(hs, lo, hi, 2, skip_range=np.array([[0, 1], [0, 0]], np.int32), skip=np.array([[2], [-1]], np.int32))
    assert list(total) == [1, 0] and obj.tolist() == [[1, -1], [-1, -1]]  # the body skips itself and one more
