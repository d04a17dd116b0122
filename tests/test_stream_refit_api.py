"""The refit of a live scene from device buffers on the caller's stream (p3d_scene_refit_device, include/p3d.h) without a
GPU: the entry point is declared, exported and wrapped, and the tensor wrappers refuse what they cannot pass on before the
library is called, with the checks of the waiting wrappers (test_device_geometry_api.py)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from api_checks import scene_without_a_library
from conftest import ROOT
import p3d_amd as p3d
from scene_update_helpers import SPHERE, TRIANGLE


def test_header_declares_the_entry_point():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "p3d.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+p3d_scene_refit_device\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*const\s+p3d_geom_source\s*\*\s*\w+,"
                     r"\s*void\s*\*\s*\w+\)", code)
    # detected by its symbol: the version and the modes stay
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)
    assert re.search(r"P3D_UPDATE_REFIT\s*=\s*0\s*,\s*P3D_UPDATE_REBUILD\s*=\s*1\s*\}", code)


def test_library_exports_it():
    lib = p3d.lib()
    assert hasattr(lib, "p3d_scene_refit_device")
    assert "p3d_scene_refit_device" in p3d.EXPORTS
    assert lib.p3d_abi_version() == 4
    assert lib.p3d_scene_refit_device(None, 0, None, None) == -1  # P3D_ERR_INVALID
    assert lib.p3d_last_error().startswith(b"p3d_scene_refit_device: null scene")


def test_python_wraps_it():
    for name, args in (("refit_triangles", ["self", "first", "positions", "indices", "stream"]),
                       ("refit_spheres", ["self", "first", "centre_radius", "stream"]),
                       ("refit_device", ["self", "sources", "stream"])):
        f = getattr(p3d.DeviceScene, name)
        assert callable(f), name
        sig = inspect.signature(f)
        assert list(sig.parameters) == args, name
        assert sig.parameters["stream"].default == 0, name


def test_wrappers_refuse_bad_tensors_before_the_library():
    import torch
    dev = scene_without_a_library()
    good_pos = torch.zeros((6, 3), dtype=torch.float32)
    good_idx = torch.zeros((2, 3), dtype=torch.int32)
    cases = [
        ("a CPU tensor", "host memory", lambda: dev.refit_triangles(0, good_pos)),
        ("CPU indices", "indices: the tensor is in host memory", lambda: dev.refit_triangles(0, (0x1000, 6), good_idx, stream=0)),
        ("a float64 tensor", "dtype", lambda: dev.refit_triangles(0, good_pos.double())),
        ("int64 indices", "indices: dtype", lambda: dev.refit_triangles(0, (0x1000, 6), good_idx.long())),
        ("a non-contiguous tensor", "contiguous", lambda: dev.refit_triangles(0, torch.zeros((3, 6), dtype=torch.float32).t())),
        ("a [V, 2] shape", "shape", lambda: dev.refit_triangles(0, torch.zeros((6, 2), dtype=torch.float32))),
        ("a soup of 4 positions", "3 positions per triangle", lambda: dev.refit_triangles(0, (0x1000, 4))),
        ("a numpy array", "torch.Tensor", lambda: dev.refit_triangles(0, np.zeros((6, 3), np.float32))),
        ("CPU spheres", "host memory", lambda: dev.refit_spheres(0, torch.zeros((5, 4), dtype=torch.float32))),
        ("float64 spheres", "dtype", lambda: dev.refit_spheres(0, torch.zeros((5, 4), dtype=torch.float64))),
        ("an index tensor for spheres", "dtype", lambda: dev.refit_spheres(0, torch.zeros((5, 4), dtype=torch.int32))),
        ("[N, 3] spheres", "shape", lambda: dev.refit_spheres(0, torch.zeros((5, 3), dtype=torch.float32))),
        ("non-contiguous spheres", "contiguous", lambda: dev.refit_spheres(0, torch.zeros((4, 5), dtype=torch.float32).t())),
        ("one bad mesh in a list", "dtype", lambda: dev.refit_triangles([(0, (0x1000, 6)), (2, good_pos.half())], stream=0)),
        ("one bad set in a list", "shape", lambda: dev.refit_spheres([(0, (0x1000, 2)), (2, torch.zeros((5, 3), dtype=torch.float32))])),
        ("a null raw address", "raw pair", lambda: dev.refit_spheres(0, (0, 5))),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
    # spheres take no index tensor: a set of three is not a sphere set
    with pytest.raises(TypeError):
        dev.refit_spheres([(0, (0x1000, 5), good_idx)])
    # the sources the waiting wrappers make are the sources these pass on
    sph = dev.sphere_source(3, (0x3000, 5))
    assert (sph.first, sph.count, sph.kind, sph.n_elems, sph.d_data, sph.d_index) == (3, 5, SPHERE, 5, 0x3000, None)
    tri = dev.triangle_source(7, (0x1000, 30), (0x2000, 11))
    assert (tri.first, tri.count, tri.kind, tri.n_elems, tri.d_data, tri.d_index) == (7, 11, TRIANGLE, 30, 0x1000, 0x2000)
