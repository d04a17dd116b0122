"""Geometry from device memory (p3d_scene_update_geometry_device, include/p3d.h) without a GPU: the entry point and its
structure are declared, exported and wrapped; p3d.deformed / p3d.deformed_spheres - the host route of the GPU tests - are plain
gathers that return the input bits, in soup and indexed form alike, and produce rows HostScene.set_geometry accepts with the
result a scene file holding those numbers gives; and the tensor wrappers refuse what they cannot pass on before the library
is called."""
import ctypes as C
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
from conftest import scene_path
from device_geometry_helpers import deformed_mesh, indexed, moved_spheres
import p3d_amd as p3d
from scene_update_helpers import SPHERE, TRIANGLE, write_moved_p3f

DESC_KEYS = ("prim_v", "prim_type", "prim_material", "prim_n", "prim_bmin", "prim_bmax")


def test_header_declares_the_structure_and_the_entry_point():
    code = header_code()
    assert re.search(r"typedef\s+struct\s+p3d_geom_source\s*\{\s*uint32_t\s+first\s*,\s*count\s*;\s*uint32_t\s+kind\s*;\s*uint32_t\s+n_elems\s*;"
                     r"\s*const\s+void\s*\*\s*d_data\s*;\s*const\s+uint32_t\s*\*\s*d_index\s*;\s*uint64_t\s+reserved\[2\]\s*;\s*\}\s*p3d_geom_source\s*;", code)
    assert re.search(r"\bint\s+p3d_scene_update_geometry_device\s*\(\s*p3d_scene\s*\*\s*\w+,\s*uint32_t\s+\w+,\s*const\s+p3d_geom_source\s*\*\s*\w+,"
                     r"\s*uint32_t\s+\w+,\s*float\s*\*\s*\w+\)", code)
    assert re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", code)
    assert re.search(r"P3D_UPDATE_REFIT\s*=\s*0\s*,\s*P3D_UPDATE_REBUILD\s*=\s*1\s*\}", code)
    assert C.sizeof(p3d.GeomSource) == 48
    assert [(n, getattr(p3d.GeomSource, n).offset) for n, _ in p3d.GeomSource._fields_] == [
        ("first", 0), ("count", 4), ("kind", 8), ("n_elems", 12), ("d_data", 16), ("d_index", 24), ("reserved", 32)]


def test_library_exports_it_and_python_wraps_it():
    lib = p3d.lib()
    assert hasattr(lib, "p3d_scene_update_geometry_device")
    assert "p3d_scene_update_geometry_device" in p3d.EXPORTS
    assert lib.p3d_abi_version() == 4
    for name in ("update_geometry_device", "update_triangles", "update_spheres", "triangle_source", "sphere_source"):
        assert callable(getattr(p3d.DeviceScene, name)), name
    assert callable(p3d.deformed) and callable(p3d.deformed_spheres)
    ms = C.c_float(7.0)
    assert lib.p3d_scene_update_geometry_device(None, 0, None, p3d.UPDATE_REBUILD, C.byref(ms)) == -1  # P3D_ERR_INVALID
    assert b"null scene" in lib.p3d_last_error()


def _same_desc(a, b, what):
    for k in DESC_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs" % (what, k)


def test_deformed_is_a_gather_soup_and_indexed(tri5k_path, tmp_path):
    hs = p3d.HostScene(tri5k_path)
    a = hs.arrays()
    n = a["n_prims"]
    assert (a["prim_type"] == TRIANGLE).all()
    # the scene's own vertices, as a soup: the input rows
    objs, rows = p3d.deformed(a["prim_v"], 0, a["prim_v"].reshape(-1, 3))
    assert np.array_equal(objs, np.arange(n)) and objs.dtype == np.uint32
    assert rows.dtype == np.float32 and rows.shape == (n, 9) and rows.tobytes() == a["prim_v"].tobytes()
    # the indexed form, positions deduplicated, with every index dtype the device route takes
    pos, idx = indexed(a["prim_v"])
    assert len(pos) <= 3 * n and idx.shape == (n, 3)
    for dtype in (np.int32, np.uint32, np.int64):
        objs_i, rows_i = p3d.deformed(a["prim_v"], 0, pos, idx.astype(dtype))
        assert np.array_equal(objs_i, objs) and rows_i.tobytes() == rows.tobytes(), dtype
    # a part of the mesh, from the middle
    objs_p, rows_p = p3d.deformed(a["prim_v"], 100, pos, idx[100:357])
    assert np.array_equal(objs_p, np.arange(100, 357)) and rows_p.tobytes() == a["prim_v"][100:357].tobytes()
    # a deformation: set_geometry takes the rows, and the descriptor is that of a scene file with these numbers
    pos_d, idx_d, soup = deformed_mesh(a, seed=3)
    objs, rows = p3d.deformed(a["prim_v"], 0, soup)
    assert rows.tobytes() == p3d.deformed(a["prim_v"], 0, pos_d, idx_d)[1].tobytes()
    assert rows.tobytes() != a["prim_v"].tobytes()
    assert np.abs(rows.astype(np.float64) - a["prim_v"]).max() > 0
    hs.set_geometry(objs, rows)
    moved = hs.arrays()
    assert moved["prim_v"].tobytes() == rows.tobytes()
    assert np.isfinite(moved["prim_n"]).all() and (moved["prim_bmin"] <= moved["prim_bmax"]).all()
    loaded = p3d.HostScene(write_moved_p3f(tri5k_path, str(tmp_path / "moved.p3f"), a["prim_type"], objs, rows)).arrays()
    _same_desc(moved, loaded, "tri5k, deformed")
    for bad in (dict(positions=pos, indices=idx[:, :2]), dict(positions=pos[:, :2], indices=idx), dict(positions=pos[:4]),
                dict(positions=pos, indices=idx + len(pos)), dict(positions=pos, indices=idx.astype(np.float32))):
        with pytest.raises(ValueError):
            p3d.deformed(a["prim_v"], 0, **bad)
    with pytest.raises(ValueError):
        p3d.deformed(a["prim_v"], n - 1, pos, idx[:2])  # past the last object


def test_deformed_spheres_likewise(tmp_path):
    path = scene_path("balls_low.p3f")
    hs = p3d.HostScene(path)
    a = hs.arrays()
    spheres = np.nonzero(a["prim_type"] == SPHERE)[0]
    first, count = int(spheres[0]), len(spheres)
    assert np.array_equal(spheres, np.arange(first, first + count))
    objs, rows = p3d.deformed_spheres(a["prim_v"], first, a["prim_v"][spheres, :4])
    assert np.array_equal(objs, spheres) and rows.tobytes() == a["prim_v"][spheres].tobytes()
    cr = moved_spheres(a, first, count, seed=4)
    objs, rows = p3d.deformed_spheres(a["prim_v"], first, cr)
    assert rows[:, :4].tobytes() == cr.tobytes() and not rows[:, 4:].any()
    hs.set_geometry(objs, rows)
    moved = hs.arrays()
    assert moved["prim_v"][spheres].tobytes() == rows.tobytes()
    loaded = p3d.HostScene(write_moved_p3f(path, str(tmp_path / "moved.p3f"), a["prim_type"], objs, rows)).arrays()
    _same_desc(moved, loaded, "balls_low, moved spheres")
    with pytest.raises(ValueError):
        p3d.deformed_spheres(a["prim_v"], first, cr[:, :3])
    with pytest.raises(ValueError):
        p3d.deformed_spheres(a["prim_v"], first + 1, cr)


def test_wrappers_refuse_bad_tensors_before_the_library():
    import torch
    dev = scene_without_a_library()
    good_pos = torch.zeros((6, 3), dtype=torch.float32)
    good_idx = torch.zeros((2, 3), dtype=torch.int32)
    cases = [
        ("a CPU tensor", "host memory", lambda: dev.update_triangles(0, good_pos)),
        ("CPU indices", "indices: the tensor is in host memory", lambda: dev.update_triangles(0, (0x1000, 6), good_idx)),
        ("a float64 tensor", "dtype", lambda: dev.update_triangles(0, good_pos.double())),
        ("int64 indices", "indices: dtype", lambda: dev.update_triangles(0, (0x1000, 6), good_idx.long())),
        ("a non-contiguous tensor", "contiguous", lambda: dev.update_triangles(0, torch.zeros((3, 6), dtype=torch.float32).t())),
        ("a [V, 2] shape", "shape", lambda: dev.update_triangles(0, torch.zeros((6, 2), dtype=torch.float32))),
        ("a flat tensor", "shape", lambda: dev.update_triangles(0, torch.zeros(18, dtype=torch.float32))),
        ("a soup of 4 positions", "3 positions per triangle", lambda: dev.update_triangles(0, (0x1000, 4))),
        ("a numpy array", "torch.Tensor", lambda: dev.update_triangles(0, np.zeros((6, 3), np.float32))),
        ("CPU spheres", "host memory", lambda: dev.update_spheres(0, torch.zeros((5, 4), dtype=torch.float32))),
        ("float64 spheres", "dtype", lambda: dev.update_spheres(0, torch.zeros((5, 4), dtype=torch.float64))),
        ("[N, 3] spheres", "shape", lambda: dev.update_spheres(0, torch.zeros((5, 3), dtype=torch.float32))),
        ("non-contiguous spheres", "contiguous", lambda: dev.update_spheres(0, torch.zeros((4, 5), dtype=torch.float32).t())),
        ("one bad mesh in a list", "dtype", lambda: dev.update_triangles([(0, (0x1000, 6)), (2, good_pos.half())])),
        ("a null raw address", "raw pair", lambda: dev.update_spheres(0, (0, 5))),
    ]
    for what, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1 and word in str(e.value), "%s: %s" % (what, e.value)
    # raw (address, rows) pairs are taken at their word: the sources they make
    tri = dev.triangle_source(7, (0x1000, 30), (0x2000, 11))
    assert (tri.first, tri.count, tri.kind, tri.n_elems, tri.d_data, tri.d_index) == (7, 11, TRIANGLE, 30, 0x1000, 0x2000)
    soup = dev.triangle_source(0, (0x1000, 30))
    assert (soup.count, soup.n_elems, soup.d_index) == (10, 30, None) and not any(soup.reserved)
    sph = dev.sphere_source(3, (0x3000, 5))
    assert (sph.first, sph.count, sph.kind, sph.n_elems, sph.d_data, sph.d_index) == (3, 5, SPHERE, 5, 0x3000, None)
