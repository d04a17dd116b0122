"""HostScene: the loader and the host builders of libp3d.so."""
import ctypes as C
import os

import numpy as np

from ._abi import LOAD_LEGACY_F11, SceneDesc, _check, _Handle, lib
from ._device_args import _NEAREST_OUTPUTS
from ._host_args import _host_nearest_k, _host_query, _per_row, _points


class HostScene(_Handle):
    """Scene::load_p3f + BVH::build / Grid::Build on the host (C++ inside libp3d.so)."""
    _destroy = "p3d_host_scene_destroy"

    def __init__(self, path, legacy_f11=False):
        self._L = lib()
        h = C.c_void_p()
        _check(self._L.p3d_host_scene_load(os.fsencode(path), LOAD_LEGACY_F11 if legacy_f11 else 0, C.byref(h)))
        self._h = h
        self.path = path

    def set_resolution(self, rx, ry):
        _check(self._L.p3d_host_scene_set_resolution(self._h, int(rx), int(ry)))

    def set_lens(self, aperture_ratio, focal_ratio):
        _check(self._L.p3d_host_scene_set_lens(self._h, float(aperture_ratio), float(focal_ratio)))

    def replicate_lights(self, spp_sqrt, light_side):
        _check(self._L.p3d_host_scene_replicate_lights(self._h, int(spp_sqrt), float(light_side)))

    def set_geometry(self, objects, v):
        """p3d_host_scene_set_geometry: the nine geometry floats `v[i]` (what prim_v holds for the object's kind) replace those of
        object `objects[i]`, through the loader's constructors.  Planes are refused.  Drops the host BVH and grid."""
        obj = np.ascontiguousarray(objects, np.uint32).reshape(-1)
        g = np.ascontiguousarray(v, np.float32).reshape(-1, 9)
        if len(g) != len(obj):
            raise ValueError("set_geometry: %d objects, %d rows of nine floats" % (len(obj), len(g)))
        _check(self._L.p3d_host_scene_set_geometry(self._h, len(obj), obj.ctypes.data, g.ctypes.data))

    def nearest(self, points, max_dist=None):
        """p3d_host_scene_nearest: for every point the object whose surface is nearest, by brute force on the CPU ->
        (object int32 (n,), dist float32 (n,), closest float32 (n, 3)); -1, FLT_MAX and zeros where nothing lies within
        max_dist (float32 (n,), or None: no limit)."""
        p = _points(points)
        m = _per_row("nearest", max_dist, len(p), "points", "limits", error=ValueError)
        return _host_query(self, "nearest", len(p), (p, m), _NEAREST_OUTPUTS, ("object", "dist", "closest"))

    def nearest_k(self, points, k, max_dist=None):
        """p3d_host_scene_nearest_k: for every point the (at most) k objects whose surfaces are nearest, nearer than max_dist
        (float32 (n,), or None: no limit), ordered by (distance, object index), by brute force on the CPU -> (count int32 (n,),
        object int32 (n, k), dist float32 (n, k), closest float32 (n, k, 3)); rows from count on hold -1, FLT_MAX and zeros.
        count == k: there may be more.  1 <= k <= NEAREST_K_MAX."""
        return _host_nearest_k(self, "nearest_k", points, k, max_dist, error=ValueError)

    def has_skybox(self):
        """A cubemap is loaded: the folder of the scene's `env` line was found, or load_skybox was called (p3d_host_scene_has_skybox)."""
        return bool(self._L.p3d_host_scene_has_skybox(self._h))

    def load_skybox(self, sky_dir):
        """Scene::LoadSkybox (scene.cpp:329-377): the six faces of `sky_dir` as .jpg (decoded by the library) or .ppm."""
        _check(self._L.p3d_host_scene_load_skybox(self._h, os.fsencode(sky_dir)))

    def skybox_face(self, face):
        """Scene::skybox_img[face] as the library decoded it: (res_y, res_x, 3) uint8, bottom row first."""
        img = C.POINTER(C.c_uint8)()
        w, h = C.c_uint32(), C.c_uint32()
        _check(self._L.p3d_host_scene_skybox_face(self._h, int(face), C.byref(img), C.byref(w), C.byref(h)))
        return np.ctypeslib.as_array(img, shape=(h.value, w.value, 3)).copy()

    def view(self):
        """p3d_host_scene_view: the `v` block -> dict(from_, at, up, angle, aperture_ratio, focal_ratio), the arguments of
        look_at that rebuild the scene's camera (float32 values as the loader read them)."""
        f, a, u = (C.c_float * 3)(), (C.c_float * 3)(), (C.c_float * 3)()
        ang, ap, fr = C.c_float(), C.c_float(), C.c_float()
        _check(self._L.p3d_host_scene_view(self._h, f, a, u, C.byref(ang), C.byref(ap), C.byref(fr)))
        return dict(from_=tuple(f), at=tuple(a), up=tuple(u), angle=ang.value, aperture_ratio=ap.value, focal_ratio=fr.value)

    def desc(self, bvh=False, grid=False):
        p = C.POINTER(SceneDesc)()
        _check(self._L.p3d_host_scene_desc(self._h, int(bvh), int(grid), C.byref(p)))
        return p.contents

    # numpy views of the flattened arrays (copies), for host-logic tests
    def arrays(self, bvh=False, grid=False):
        d = self.desc(bvh, grid)
        out = dict(n_prims=d.n_prims, n_materials=d.n_materials, n_lights=d.n_lights,
                   res=(d.camera.res_x, d.camera.res_y), background=np.array(d.background[:], np.float32))
        prims = [d.prims[i] for i in range(d.n_prims)] if d.n_prims else []
        out["prim_v"] = np.array([list(p.v) for p in prims], np.float32).reshape(-1, 9)
        out["prim_type"] = np.array([p.type for p in prims], np.uint32)
        out["prim_material"] = np.array([p.material for p in prims], np.uint32)
        out["prim_n"] = np.array([list(p.n) for p in prims], np.float32).reshape(-1, 3)
        out["prim_bmin"] = np.array([list(p.bmin) for p in prims], np.float32).reshape(-1, 3)
        out["prim_bmax"] = np.array([list(p.bmax) for p in prims], np.float32).reshape(-1, 3)
        mats = [d.materials[i] for i in range(d.n_materials)]
        out["materials"] = np.array([[*m.diff_color, m.diffuse, *m.spec_color, m.specular, m.shine, m.transmittance,
                                      m.refr_index, m.reflection, *m.emission, 0.0] for m in mats],
                                    np.float32).reshape(-1, 16)
        out["lights"] = np.array([[*d.lights[i].position, *d.lights[i].color] for i in range(d.n_lights)],
                                 np.float32).reshape(-1, 6)
        c = d.camera
        out["camera"] = dict(eye=np.array(c.eye[:], np.float32), u=np.array(c.u[:], np.float32),
                             v=np.array(c.v[:], np.float32), n=np.array(c.n[:], np.float32), w=c.w, h=c.h,
                             plane_dist=c.plane_dist, focal_ratio=c.focal_ratio, aperture=c.aperture)
        if bvh:
            n = d.n_bvh_nodes
            buf = np.ctypeslib.as_array(C.cast(d.bvh_nodes, C.POINTER(C.c_uint32)), shape=(n, 8)).copy()
            out["bvh_bmin"] = buf[:, 0:3].view(np.float32)
            out["bvh_index"] = buf[:, 3].copy()
            out["bvh_bmax"] = buf[:, 4:7].view(np.float32)
            out["bvh_count_leaf"] = buf[:, 7].copy()
            out["bvh_order"] = (np.ctypeslib.as_array(d.bvh_prim_index, shape=(d.n_bvh_prim_index,)).copy()
                                if d.n_bvh_prim_index else np.zeros(0, np.uint32))
            out["bvh_max_depth"] = d.bvh_max_depth
        if grid:
            g = d.grid
            out["grid_n"] = (g.nx, g.ny, g.nz)
            out["grid_bmin"] = np.array(g.bmin[:], np.float32)
            out["grid_bmax"] = np.array(g.bmax[:], np.float32)
            out["grid_cell_start"] = np.ctypeslib.as_array(g.cell_start, shape=(g.n_cells + 1,)).copy()
            out["grid_cell_items"] = (np.ctypeslib.as_array(g.cell_items, shape=(g.n_items,)).copy()
                                      if g.n_items else np.zeros(0, np.uint32))
        return out
