"""DeviceScene: a scene resident on one GPU - frames, live updates and queries."""
import ctypes as C
import os

import numpy as np

from ._abi import (PLAN_MODES, UPDATE_REFIT, BvhCost, BvhNode, Camera, DebugPlan, FramePlan, GeomSource, GridDesc, P3DError, Prim,
                   SceneDesc, SkyboxDesc, Tile, Xform, XformRange, _check, _Handle, _ptr, _stream, lib)
from ._device_args import (NEAREST_K_MAX, TRACE_HITS_K_MAX, _NEAREST_OUTPUTS, _TRACE_OUTPUTS, _device_rows, _device_vector,
                           _nearest_k_outputs, _trace_hits_outputs)
from .device_queries import _device_points, _device_query, _device_rays
from .geometry import _xform_arrays
from .passes import Accumulator, AdaptiveAccumulator, _frame_outputs


def _xform_ranges(who, r):
    """The XformRange array of the (n, 3) integer ranges `r` as a call's argument (null without ranges); `who` refuses
    values that do not fit uint32"""
    if len(r) and (r.min() < 0 or r.max() > 0xffffffff):
        raise P3DError(-1, "%s: a range does not fit uint32" % who)
    rg = (XformRange * max(len(r), 1))()
    for i, (first, count, x) in enumerate(r):
        rg[i] = XformRange(int(first), int(count), int(x), 0)
    return C.cast(rg, C.c_void_p) if len(r) else None


def _geom_sources(sources):
    """(n, the GeomSource array as a call's argument - null without sources) of an iterable of GeomSources"""
    src = list(sources)
    arr = (GeomSource * max(len(src), 1))(*src)
    return len(src), C.cast(arr, C.c_void_p) if src else None


class DeviceScene(_Handle):
    """p3d_scene_create: the flattened scene resident in HBM of one MI355X."""
    _destroy = "p3d_scene_destroy"

    def __init__(self, host_scene, bvh=True, grid=False, device=0):
        """bvh: True = the reference-exact tree built on the host (BVH::build), "device" = a linear BVH built
        on the GPU (p3d_scene_create_device_bvh: correct closest hits, not the reference's tree), False = none,
        a dict with the bvh_* keys of HostScene.arrays(bvh=True) (e.g. from export_bvh) = that tree over the
        host scene's current objects.
        grid: True = the host's grid (Grid::Build) uploaded with the scene, "device" = the same grid built on the GPU after
        create (p3d_scene_build_grid; needs bvh="device"): it follows update_prims, an uploaded one refuses them."""
        self._L = lib()
        self.host = host_scene
        self.device_bvh_ms = None
        self.device_grid_ms = None
        device_grid = isinstance(grid, str) and grid == "device"
        if device_grid and not (isinstance(bvh, str) and bvh == "device"):
            raise P3DError(-1, 'DeviceScene: grid="device" needs bvh="device" (only those scenes keep their boxes on the GPU)')
        if isinstance(grid, str) and not device_grid:
            raise P3DError(-1, 'DeviceScene: grid is True, False or "device"')
        if device_grid:
            grid = False
        h = C.c_void_p()
        if isinstance(bvh, dict):
            src = host_scene.desc(False, grid)
            d = SceneDesc.from_buffer_copy(src)  # the host scene's descriptor with the tree swapped in
            n = len(bvh["bvh_index"])
            nodes = np.zeros((n, 8), np.uint32)
            nodes[:, 0:3] = np.ascontiguousarray(bvh["bvh_bmin"], np.float32).reshape(n, 3).view(np.uint32)
            nodes[:, 3] = bvh["bvh_index"]
            nodes[:, 4:7] = np.ascontiguousarray(bvh["bvh_bmax"], np.float32).reshape(n, 3).view(np.uint32)
            nodes[:, 7] = bvh["bvh_count_leaf"]
            order = np.ascontiguousarray(bvh["bvh_order"], np.uint32)
            d.n_bvh_nodes, d.n_bvh_prim_index, d.bvh_max_depth = n, len(order), int(bvh["bvh_max_depth"])
            d.bvh_nodes = C.cast(nodes.ctypes.data, C.POINTER(BvhNode))
            d.bvh_prim_index = C.cast(order.ctypes.data, C.POINTER(C.c_uint32))
            _check(self._L.p3d_scene_create(C.byref(d), int(device), C.byref(h)))
        elif isinstance(bvh, str) and bvh == "device":
            d = host_scene.desc(False, grid)
            if device_grid:  # a host scene that has built its grid once keeps it in its descriptor: this scene builds its own
                d = SceneDesc.from_buffer_copy(d)
                d.has_grid = 0
            ms = C.c_float(0)
            _check(self._L.p3d_scene_create_device_bvh(C.byref(d), int(device), C.byref(h), C.byref(ms)))
            self.device_bvh_ms = ms.value
        else:
            d = host_scene.desc(bool(bvh), grid)
            _check(self._L.p3d_scene_create(C.byref(d), int(device), C.byref(h)))
        self.res = (d.camera.res_x, d.camera.res_y)
        self._h = h
        self.device = device
        if device_grid:
            self.device_grid_ms = self.build_grid()

    def set_skybox(self, faces):
        """faces: 6 uint8 arrays (h, w, 3|4), row 0 = BOTTOM row, order RIGHT LEFT TOP BOTTOM FRONT BACK
        (what Scene::LoadSkybox keeps, scene.cpp:329-377).  See load_skybox_dir for JPEG folders."""
        keep = [np.ascontiguousarray(f, np.uint8) for f in faces]
        d = SkyboxDesc()
        for i, f in enumerate(keep):
            d.face[i].img = f.ctypes.data
            d.face[i].res_x, d.face[i].res_y, d.face[i].bpp = f.shape[1], f.shape[0], f.shape[2]
        _check(self._L.p3d_scene_set_skybox(self._h, C.byref(d)))

    def bind_host(self):
        """p3d_host_scene_bind_device: the host classes' query forwards answer from this device scene, and the cubemap the
        loader read for an `env` line is uploaded."""
        _check(self._L.p3d_host_scene_bind_device(self.host._h, self._h))

    def full_tile(self):
        return Tile(0, 0, self.res[0], self.res[1], 0, 1)

    @property
    def camera(self):
        """p3d_scene_camera: the scene's current Camera."""
        cam = Camera()
        _check(self._L.p3d_scene_camera(self._h, C.byref(cam)))
        return cam

    def set_camera(self, cam):
        """p3d_scene_set_camera: frames rendered after it see `cam` (a Camera of the scene's resolution, e.g. from look_at).
        Waits for the device.  Accumulators of this scene refuse passes until they are reset."""
        _check(self._L.p3d_scene_set_camera(self._h, C.byref(cam)))

    def update_prims(self, objects, mode=UPDATE_REFIT):
        """p3d_scene_update_prims: the records of `objects` are taken from the bound host scene's current descriptor (after
        HostScene.set_geometry) and the device BVH is refitted or rebuilt.  Waits for the device; returns update_ms.
        Accumulators of this scene refuse passes until they are reset."""
        obj = np.ascontiguousarray(objects, np.uint32).reshape(-1)
        d = self.host.desc(False, False)
        if len(obj) and int(obj.max()) >= d.n_prims:
            raise P3DError(-1, "update_prims: object index out of range")
        recs = (Prim * max(len(obj), 1))()
        for i, o in enumerate(obj):
            recs[i] = d.prims[int(o)]
        ms = C.c_float(0)
        _check(self._L.p3d_scene_update_prims(self._h, len(obj), obj.ctypes.data if len(obj) else None,
                                              C.cast(recs, C.c_void_p) if len(obj) else None, int(mode), C.byref(ms)))
        return ms.value

    def transform_prims(self, ranges, xforms, mode=UPDATE_REFIT, sphere_scale=None):
        """p3d_scene_transform_prims: the objects of every (first, count, xform) in `ranges` are set, on the device, to
        xforms[xform] of their REST geometry (what they were created with or last given by update_prims), and the device BVH
        is refitted or rebuilt.  `xforms`: (n, 3, 4) or (n, 12) float32; `sphere_scale`: n radius factors, default 1.  Waits
        for the device; returns update_ms.  The bound host scene is not touched: HostScene.set_geometry(*transformed(...)) of
        the rest prim_v brings it along.  Accumulators of this scene refuse passes until they are reset."""
        r, m, sc = _xform_arrays(ranges, xforms, sphere_scale)
        rg = _xform_ranges("transform_prims", r)
        xf = (Xform * max(len(m), 1))()
        for i in range(len(m)):
            xf[i].m[:] = m[i].tolist()
            xf[i].sphere_scale = float(sc[i])
        ms = C.c_float(0)
        _check(self._L.p3d_scene_transform_prims(self._h, len(r), rg, len(m),
                                                 C.cast(xf, C.c_void_p) if len(m) else None, int(mode), C.byref(ms)))
        return ms.value

    def triangle_source(self, first, positions, indices=None):
        """A GeomSource for update_geometry_device: triangles first, first + 1, ... from `positions` (float32 (V, 3)) and
        `indices` (int32 or uint32 (F, 3); None = a soup of V / 3 triangles), each a contiguous CUDA/HIP torch.Tensor on the
        scene's device or a raw (address, rows) pair.  Keep the tensors alive until the update has returned."""
        d_pos, n_pos = _device_rows(positions, "positions", 3, ("float32",), self.device)
        if indices is None:
            if n_pos % 3:
                raise P3DError(-1, "positions: a soup needs 3 positions per triangle, got %d" % n_pos)
            return GeomSource(int(first), n_pos // 3, 1, n_pos, d_pos, None)
        d_idx, n_tri = _device_rows(indices, "indices", 3, ("int32", "uint32"), self.device)
        return GeomSource(int(first), n_tri, 1, n_pos, d_pos, d_idx)

    def sphere_source(self, first, centre_radius):
        """A GeomSource for update_geometry_device: spheres first, first + 1, ... from a float32 (N, 4) tensor of centres and
        radii (or a raw (address, rows) pair)."""
        d_cr, n = _device_rows(centre_radius, "centre_radius", 4, ("float32",), self.device)
        return GeomSource(int(first), n, 0, n, d_cr, None)

    def update_geometry_device(self, sources, mode=UPDATE_REFIT):
        """p3d_scene_update_geometry_device: the objects of every GeomSource in `sources` (raw device addresses; see
        triangle_source / sphere_source) take their nine geometry floats from device memory, normals and boxes are computed on
        the device as the host's constructors compute them, and the device BVH is refitted or rebuilt.  Waits for the device -
        work that any stream had enqueued to fill the buffers has finished before they are read; returns update_ms.  The bound
        host scene is not touched: HostScene.set_geometry(*deformed(...)) brings it along.  Accumulators of this scene refuse
        passes until they are reset."""
        ms = C.c_float(0)
        _check(self._L.p3d_scene_update_geometry_device(self._h, *_geom_sources(sources), int(mode), C.byref(ms)))
        return ms.value

    def update_triangles(self, first, positions=None, indices=None, mode=UPDATE_REFIT):
        """Triangles first, first + 1, ... from a float32 (V, 3) position tensor and an int32 / uint32 (F, 3) index tensor on
        the scene's device (F objects), or from positions alone (V / 3 objects); raw (address, rows) pairs are taken too.
        Several meshes in one call: update_triangles([(first, positions), (first, positions, indices), ...], mode=...).
        A tensor on the host, of another dtype or shape, or not contiguous raises P3DError before the library is called."""
        meshes = first if isinstance(first, list) else [(first, positions, indices)]
        return self.update_geometry_device([self.triangle_source(*m) for m in meshes], mode)

    def update_spheres(self, first, centre_radius=None, mode=UPDATE_REFIT):
        """Spheres first, first + 1, ... from a float32 (N, 4) tensor of centres and radii on the scene's device; or a list
        of (first, centre_radius) for several sets in one call."""
        sets = first if isinstance(first, list) else [(first, centre_radius)]
        return self.update_geometry_device([self.sphere_source(*m) for m in sets], mode)

    def refit_device(self, sources, stream=0):
        """p3d_scene_refit_device: the REFIT of update_geometry_device enqueued on `stream` (a torch.cuda.Stream or a raw
        hipStream_t; 0 = the default stream) without a wait: what the stream had enqueued to fill the buffers runs first,
        frames and queries enqueued on it afterwards see the new geometry.  At most 16 GeomSources.  Only the first call on a
        scene may wait.  Keep the tensors alive until the stream has passed the call.  Objects the kernel skips (a bad
        index, an unusable box) show in status(), not here.  Accumulators of this scene refuse passes until they are reset."""
        _check(self._L.p3d_scene_refit_device(self._h, *_geom_sources(sources), _stream(stream)))

    def refit_triangles(self, first, positions=None, indices=None, stream=0):
        """update_triangles(..., UPDATE_REFIT) on `stream` without a wait (refit_device): the same arguments, tensors or raw
        (address, rows) pairs, or a list of meshes; refused before the library is called like there."""
        meshes = first if isinstance(first, list) else [(first, positions, indices)]
        self.refit_device([self.triangle_source(*m) for m in meshes], stream)

    def refit_spheres(self, first, centre_radius=None, stream=0):
        """update_spheres(..., UPDATE_REFIT) on `stream` without a wait (refit_device)."""
        sets = first if isinstance(first, list) else [(first, centre_radius)]
        self.refit_device([self.sphere_source(*m) for m in sets], stream)

    def set_rig(self, ranges, n_xforms):
        """p3d_scene_set_rig: the objects of every (first, count, xform) in `ranges` (as for transform_prims) follow slot
        `xform` of the `n_xforms` matrices every later pose_device brings.  A setup call: it waits for the device and makes
        the rest copy, the builder's state and the rig's table.  No ranges remove the rig."""
        r = np.asarray(list(ranges), np.int64).reshape(-1, 3)
        _check(self._L.p3d_scene_set_rig(self._h, len(r), _xform_ranges("set_rig", r), int(n_xforms)))

    def rig(self):
        """p3d_scene_rig: {"n_ranges", "n_xforms", "n_posed_objects"} of the current rig, three zeros without one"""
        n = [C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)]
        _check(self._L.p3d_scene_rig(self._h, C.byref(n[0]), C.byref(n[1]), C.byref(n[2])))
        return dict(n_ranges=n[0].value, n_xforms=n[1].value, n_posed_objects=n[2].value)

    def pose_device(self, xforms, sphere_scale=None, stream=0):
        """p3d_scene_pose_device: transform_prims(the rig's ranges, xforms, UPDATE_REFIT, sphere_scale) enqueued on `stream`
        (a torch.cuda.Stream or a raw hipStream_t; 0 = the default stream) without a wait.  `xforms`: a contiguous float32
        CUDA/HIP torch.Tensor of shape [K, 3, 4] or [K, 12] on the scene's device, K the rig's n_xforms, or a raw
        (address, K) pair; `sphere_scale`: a [K] tensor, a raw pair, or None = 1.  What the stream had enqueued to fill them
        runs first; keep them alive until the stream has passed the call.  Objects the kernel skips (an unusable transform
        or box) show in status(), not here.  Accumulators of this scene refuse passes until they are reset."""
        if hasattr(xforms, "data_ptr") and hasattr(xforms, "dim") and xforms.dim() == 3:
            if tuple(xforms.shape[1:]) != (3, 4):
                raise P3DError(-1, "xforms: shape %r, needed: (n, 3, 4) or (n, 12) with n > 0" % (tuple(xforms.shape),))
            if not xforms.is_contiguous():
                raise P3DError(-1, "xforms: the tensor is not contiguous")
            xforms = xforms.view(xforms.shape[0], 12)
        d_x, k = _device_rows(xforms, "xforms", 12, ("float32",), self.device)
        d_s = None
        if sphere_scale is not None:
            d_s, n = _device_vector(sphere_scale, "sphere_scale", ("float32",), self.device)
            if n != k:
                raise P3DError(-1, "sphere_scale: %d values for %d transforms" % (n, k))
        _check(self._L.p3d_scene_pose_device(self._h, k, _ptr(d_x), _ptr(d_s), _stream(stream)))

    def export_bvh(self):
        """p3d_scene_export_bvh: the current device-built tree as numpy arrays, with the bvh_* keys of HostScene.arrays(bvh=True)
        (children adjacent and behind their parent): DeviceScene(hs, bvh=that dict) uploads it again."""
        n, m, depth = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(self._L.p3d_scene_export_bvh(self._h, None, C.byref(n), None, C.byref(m), C.byref(depth)))
        buf = np.zeros((n.value, 8), np.uint32)
        order = np.zeros(m.value, np.uint32)
        _check(self._L.p3d_scene_export_bvh(self._h, buf.ctypes.data, C.byref(n), order.ctypes.data, C.byref(m), C.byref(depth)))
        return dict(bvh_bmin=buf[:, 0:3].view(np.float32), bvh_index=buf[:, 3].copy(), bvh_bmax=buf[:, 4:7].view(np.float32),
                    bvh_count_leaf=buf[:, 7].copy(), bvh_order=order, bvh_max_depth=depth.value)

    def bvh_cost(self):
        """p3d_scene_bvh_cost: the SAH cost of the current device-built tree (tree_cost of export_bvh(), summed on the GPU)
        -> dict(sah, sah_baseline, n_inner, n_leaves, refits_since_build, last_update_rebuilt).  Waits for the device."""
        c = BvhCost()
        _check(self._L.p3d_scene_bvh_cost(self._h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in c._fields_}

    def set_auto_rebuild(self, ratio):
        """p3d_scene_set_auto_rebuild: 0 = off (the default); with a ratio >= 1 (inf: never) an UPDATE_REFIT whose refitted tree
        costs more than ratio x sah_baseline runs the builder in the same call, with the result of UPDATE_REBUILD."""
        _check(self._L.p3d_scene_set_auto_rebuild(self._h, float(ratio)))

    def auto_rebuild(self):
        """p3d_scene_auto_rebuild: the ratio, 0 = off."""
        r = C.c_float(0)
        _check(self._L.p3d_scene_auto_rebuild(self._h, C.byref(r)))
        return r.value

    def build_grid(self):
        """p3d_scene_build_grid: builds (or builds again) the uniform grid on the GPU from the scene's current object boxes - the
        grid Grid::Build gives, to the bit.  Only for bvh="device" scenes created without a grid.  Waits for the device; returns
        build_ms.  From then on update_prims rebuilds it."""
        ms = C.c_float(0)
        _check(self._L.p3d_scene_build_grid(self._h, C.byref(ms)))
        return ms.value

    def export_grid(self):
        """p3d_scene_export_grid: the device-built grid as numpy arrays, with the grid_* keys of HostScene.arrays(grid=True)."""
        g = GridDesc()
        n, m = C.c_uint32(0), C.c_uint32(0)
        _check(self._L.p3d_scene_export_grid(self._h, C.byref(g), None, C.byref(n), None, C.byref(m)))
        start = np.zeros(n.value, np.uint32)
        items = np.zeros(max(m.value, 1), np.uint32)
        _check(self._L.p3d_scene_export_grid(self._h, C.byref(g), start.ctypes.data, C.byref(n), items.ctypes.data, C.byref(m)))
        return dict(grid_n=(g.nx, g.ny, g.nz), grid_bmin=np.array(g.bmin[:], np.float32), grid_bmax=np.array(g.bmax[:], np.float32),
                    grid_cell_start=start, grid_cell_items=items[:m.value].copy())

    def render(self, cfg, tile=None, want_rgb8=False, stats=True):
        """Host-buffer form (p3d_render_tile): returns numpy arrays."""
        t = tile or self.full_tile()
        out, buffers = _frame_outputs(t, want_rgb8, stats)
        _check(self._L.p3d_render_tile(self._h, C.byref(cfg), C.byref(t), *buffers))
        return out

    def accumulator(self, cfg, tile=None):
        """p3d_accum_create: an Accumulator that renders this frame (cfg, tile) in passes over its samples; the pass that
        completes the SPP*SPP samples returns the same bits as render(cfg, tile).  Raises P3DError (P3D_ERR_UNSUPPORTED)
        for antialiasing = 0 and for Whitted over the BVH with P3D_STACK_LITERAL."""
        return Accumulator(self, cfg, tile or self.full_tile())

    def render_progressive(self, cfg, samples_per_pass, tile=None, want_rgb8=False, stats=True):
        """Renders the frame in passes of `samples_per_pass` samples (the last one takes what is left) and yields
        (samples_done, render tuple) after every pass; the last one is the frame render(cfg, tile) returns."""
        if samples_per_pass < 1:
            raise ValueError("samples_per_pass must be at least 1")
        acc = self.accumulator(cfg, tile)
        try:
            while acc.samples_done < acc.total:
                out = acc.render(min(samples_per_pass, acc.total - acc.samples_done), want_rgb8=want_rgb8, stats=stats)
                yield acc.samples_done, out
        finally:
            acc.close()

    def adaptive(self, cfg, rel_error, min_samples=16, tile=None, reserved=(0, 0)):
        """p3d_adaptive_create: an AdaptiveAccumulator - a progressive path-traced frame (cfg, tile) whose pixels stop
        taking samples once their relative error is below rel_error (and they have at least min_samples).  Raises
        P3DError: P3D_ERR_UNSUPPORTED for Whitted and antialiasing = 0, P3D_ERR_INVALID for bad parameters."""
        return AdaptiveAccumulator(self, cfg, tile or self.full_tile(), rel_error, min_samples, reserved)

    def render_adaptive(self, cfg, samples_per_pass, rel_error, min_samples=16, tile=None, want_rgb8=False, stats=True):
        """Renders the frame in adaptive passes of `samples_per_pass` samples (the last one takes what is left) and yields
        (samples_done, active_pixels, render tuple of AdaptiveAccumulator.render) after every pass, until no pixel is
        active or every sample is done."""
        if samples_per_pass < 1:
            raise ValueError("samples_per_pass must be at least 1")
        ad = self.adaptive(cfg, rel_error, min_samples, tile)
        try:
            while ad.samples_done < ad.total:
                out = ad.render(min(samples_per_pass, ad.total - ad.samples_done), want_rgb8=want_rgb8, stats=stats)
                active = ad.active_pixels
                yield ad.samples_done, active, out
                if active == 0:
                    break
        finally:
            ad.close()

    def status(self):
        """p3d_scene_status: waits for the device, returns P3D_OK (0) or the code of a device-detected error of the
        asynchronous render_device calls since the last check (message: last_error())."""
        return int(self._L.p3d_scene_status(self._h))

    def set_tail_stream(self, stream=None):
        """p3d_scene_set_tail_stream: the launches behind pass 1 of a literal frame (the hit_stack hand-off) go to `stream` (a
        torch.cuda.Stream, a raw hipStream_t or None = off); render_device calls without stats then return their outputs when
        that stream has passed them - see join()."""
        _check(self._L.p3d_scene_set_tail_stream(self._h, _stream(stream)))

    def join(self, stream=None, host_wait=False):
        """p3d_scene_join: make `stream` (or, with host_wait, the calling thread) wait for the scene's last frame, tail included."""
        _check(self._L.p3d_scene_join(self._h, _stream(stream), 1 if host_wait else 0))

    def debug_limits(self, trip_bound=0, max_rounds=0, halo_chain=0, leftover_pool=0):
        """Tests only (csrc/p3d_debug.h, not part of include/p3d.h): shrink limits of THIS scene so that the device-side
        error paths fire; all 0 = the real limits.  Refused unless the process was started with P3D_TEST_HOOKS=1."""
        lim = (C.c_uint32 * 4)(trip_bound, max_rounds, halo_chain, leftover_pool)
        _check(self._L.p3d_debug_scene_limits(self._h, C.cast(lim, C.c_void_p)))

    def staged_f4(self, cfg, tile=None):
        """csrc/p3d_debug.h, read-only: the float4s a frame of `cfg` over `tile` copies into LDS (0: the scene is not
        staged, the kernels traverse it from global memory)."""
        n = C.c_uint32(0)
        _check(self._L.p3d_debug_staged_f4(self._h, C.byref(cfg), C.byref(tile or self.full_tile()), C.byref(n)))
        return n.value

    def frame_plan(self, cfg, tile=None, samples=None, mode="frame"):
        """csrc/p3d_debug.h, read-only: the plan of one launch as the kernel choosers read it -> FramePlan (flags as bool).
        samples: None = the whole frame (features: what render_features(cfg) takes, min(16, SPP*SPP)), n = samples [0, n),
        (begin, end) = that range (a pass of an accumulator).  mode: "frame", "adaptive" (one pass) or "features"."""
        total = cfg.spp_sqrt * cfg.spp_sqrt if cfg.antialiasing else 1
        if samples is None:
            samples = min(16, total) if mode == "features" else total
        begin, end = samples if isinstance(samples, tuple) else (0, samples)
        out = DebugPlan()
        _check(self._L.p3d_debug_frame_plan(self._h, C.byref(cfg), C.byref(tile or self.full_tile()), begin, end, PLAN_MODES[mode], C.byref(out)))
        ints = ("stack_mode", "spill_entries", "bound", "cap")
        return FramePlan(**{k: getattr(out, k) if k in ints else bool(getattr(out, k)) for k, _ in DebugPlan._fields_})

    def render_features(self, cfg, samples=0, tile=None):
        """p3d_render_features: the feature buffers of the primary rays of samples [0, K) (0: min(16, SPP*SPP)) ->
        (normal_depth, albedo_cov), two (h, w, 4) float32 arrays: (n, t) and (diff_color, coverage), means over the samples
        that hit."""
        t = tile or self.full_tile()
        nd = np.zeros((t.h, t.w, 4), np.float32)
        ac = np.zeros((t.h, t.w, 4), np.float32)
        _check(self._L.p3d_render_features(self._h, C.byref(cfg), C.byref(t), int(samples), nd.ctypes.data, ac.ctypes.data))
        return nd, ac

    def render_features_device(self, cfg, d_normal_depth, d_albedo_cov, samples=0, tile=None, stream=0):
        """p3d_render_features_device: raw HBM addresses (16-byte aligned) and a hipStream_t (or a torch.cuda.Stream)."""
        _check(self._L.p3d_render_features_device(self._h, C.byref(cfg), C.byref(tile or self.full_tile()), int(samples),
                                                  _ptr(d_normal_depth), _ptr(d_albedo_cov), _stream(stream)))

    def render_device(self, cfg, tile, d_rgb=0, d_hit=0, d_rgb8=0, stream=0, stats=None):
        """Device-buffer form: raw HBM addresses (e.g. torch.Tensor.data_ptr()) and a hipStream_t."""
        _check(self._L.p3d_render_tile_device(self._h, C.byref(cfg), C.byref(tile), _ptr(d_rgb), _ptr(d_hit), _ptr(d_rgb8), _ptr(stream),
                                              C.byref(stats) if stats is not None else None))

    def trace_closest(self, accel, origin, direction, want_t=False):
        o = np.ascontiguousarray(origin, np.float32)
        d = np.ascontiguousarray(direction, np.float32)
        n = o.shape[0]
        hit = np.zeros(n, np.int32)
        hp = np.zeros((n, 3), np.float32)
        t = np.zeros(n, np.float32) if want_t else None
        _check(self._L.p3d_trace_closest(self._h, int(accel), n, o.ctypes.data, d.ctypes.data, hit.ctypes.data,
                                         t.ctypes.data if want_t else None, hp.ctypes.data))
        return (hit, hp, t) if want_t else (hit, hp)

    def object_intercepts(self, obj, origin, direction, t_init=None):
        """Object::intercepts for n rays: -> (hit, t, direction as the test left it).  t starts as t_init (a scalar or n values;
        default zeros) and keeps that value where the test fails."""
        o = np.ascontiguousarray(origin, np.float32)
        d = np.array(direction, np.float32, order="C")
        n = o.shape[0]
        hit = np.zeros(n, np.uint8)
        t = np.zeros(n, np.float32)
        if t_init is not None:
            t[:] = t_init
        _check(self._L.p3d_object_intercepts(self._h, int(obj), n, C.c_void_p(o.ctypes.data), C.c_void_p(d.ctypes.data),
                                             C.c_void_p(hit.ctypes.data), C.c_void_p(t.ctypes.data)))
        return hit.astype(bool), t, d

    def object_normal(self, obj, points):
        p = np.ascontiguousarray(points, np.float32)
        out = np.zeros_like(p)
        _check(self._L.p3d_object_normal(self._h, int(obj), p.shape[0], C.c_void_p(p.ctypes.data), C.c_void_p(out.ctypes.data)))
        return out

    def skybox_color(self, directions):
        d = np.ascontiguousarray(directions, np.float32)
        out = np.zeros_like(d)
        _check(self._L.p3d_skybox_color(self._h, d.shape[0], C.c_void_p(d.ctypes.data), C.c_void_p(out.ctypes.data)))
        return out

    def trace_any(self, accel, origin, direction):
        o = np.ascontiguousarray(origin, np.float32)
        d = np.ascontiguousarray(direction, np.float32)
        n = o.shape[0]
        occ = np.zeros(n, np.uint8)
        _check(self._L.p3d_trace_any(self._h, int(accel), n, o.ctypes.data, d.ctypes.data, occ.ctypes.data))
        return occ

    def trace_closest_device(self, accel, origin, direction, t_max=None, want=("hit_id", "t"), stream=0, out=None):
        """p3d_trace_closest_device: the closest hits of n rays held in device memory, enqueued on `stream` (a torch.cuda.Stream
        or a raw hipStream_t; 0 = the default stream) without a wait -> {name: tensor} for the names in `want` ("hit_id", always
        there, "t", "hit_point", "normal").  origin, direction: contiguous float32 (n, 3) CUDA/HIP tensors on the scene's device,
        or raw (address, rows) pairs; t_max: float32 (n,), a hit is kept only if t < t_max.  `out`: a dict of tensors (or raw
        pairs) to write into instead of new ones.  A tensor on the host, of another dtype or shape, not contiguous, or row
        counts that differ raise P3DError before the library is called.  Read the results once the stream has passed the call."""
        who = "trace_closest_device"
        names = ["hit_id"] + [w for w in ("t", "hit_point", "normal") if w in want]
        return _device_query(self, who, accel, lambda: _device_rays(self, who, origin, direction, t_max), _TRACE_OUTPUTS, names, want,
                                  ("hit_id", "t", "hit_point", "normal"), stream, out, origin)

    def trace_any_device(self, accel, origin, direction, t_max=None, stream=0, out=None):
        """p3d_trace_any_device -> {"occluded": uint8 (n,) tensor}.  Without t_max the reference's shadow feeler (trace_any: no
        distance limit); with t_max (float32 (n,)) the segment query: 1 iff some object is hit at t < t_max, for ACCEL_NONE and
        ACCEL_BVH (the grid is refused).  Arguments and stream as trace_closest_device."""
        who = "trace_any_device"
        return _device_query(self, who, accel, lambda: _device_rays(self, who, origin, direction, t_max), {"occluded": ("uint8", None)},
                                  ["occluded"], (), ("occluded",), stream, out, origin)

    def nearest_device(self, accel, points, max_dist=None, want=("object", "dist"), stream=0, out=None):
        """p3d_nearest_device: for n points held in device memory the object whose surface is nearest, enqueued on `stream`
        without a wait -> {name: tensor} for the names in `want` ("object", always there, "dist", "closest", "normal").  points:
        a contiguous float32 (n, 3) CUDA/HIP tensor on the scene's device, or a raw (address, rows) pair; max_dist: float32 (n,),
        an object counts only nearer than it.  ACCEL_NONE and ACCEL_BVH (not over a scene with planes); the answers are
        HostScene.nearest's, bit for bit.  `out`, `stream` and the refusals as trace_closest_device."""
        who = "nearest_device"
        names = ["object"] + [w for w in ("dist", "closest", "normal") if w in want]
        return _device_query(self, who, accel, lambda: _device_points(self, who, points, max_dist), _NEAREST_OUTPUTS, names, want,
                                  ("object", "dist", "closest", "normal"), stream, out, points, "points")

    def nearest_k_device(self, accel, points, k, max_dist=None, want=("count", "object", "dist"), stream=0, out=None):
        """p3d_nearest_k_device: for n points held in device memory the (at most) k objects whose surfaces are nearest, nearer
        than max_dist, ordered by (distance, object index), enqueued on `stream` without a wait -> {name: tensor} for the names
        in `want` ("count" (n,) and "object" (n, k), always there, "dist" (n, k), "closest" and "normal" (n, k, 3)); rows from
        count on hold -1, FLT_MAX and zeros, and count == k says that there may be more.  1 <= k <= NEAREST_K_MAX.  points,
        max_dist, `out`, `stream` and the refusals as nearest_device; the answers are HostScene.nearest_k's, bit for bit."""
        who = "nearest_k_device"
        k = int(k)
        names = ["count", "object"] + [w for w in ("dist", "closest", "normal") if w in want]
        refusal = None
        if out is None and not 1 <= k <= NEAREST_K_MAX:  # (with the caller's outputs the library says it)
            refusal = "k must be 1 .. %d, got %d" % (NEAREST_K_MAX, k)
        return _device_query(self, who, accel, lambda: _device_points(self, who, points, max_dist), _nearest_k_outputs(max(k, 0)), names, want,
                                  ("count", "object", "dist", "closest", "normal"), stream, out, points, "points", k=k, refusal=refusal)

    def trace_hits_device(self, accel, origin, direction, k, t_max=None, want=("count", "object", "t"), stream=0, out=None):
        """p3d_trace_hits_device: for n rays held in device memory the (at most) k objects hit in front of t_max, ordered by
        (t, object index), and the number of all of them, enqueued on `stream` without a wait -> {name: tensor} for the names in
        `want` ("count" (n,) and "object" (n, k), always there with k >= 1, "t" (n, k), "hit_point" and "normal" (n, k, 3), and
        "total" (n,): every object hit, whatever k is); rows from count on hold -1, FLT_MAX and zeros, and count == k without
        "total" says that there may be more.  0 <= k <= TRACE_HITS_K_MAX; k = 0 is the count alone: `want` must hold "total"
        and nothing else comes back.  total counts objects, not crossings (a sphere or a box: one; a closed triangle mesh: one
        per triangle crossed, so total & 1 is "the origin is inside").  ACCEL_NONE and ACCEL_BVH (the grid is refused); rays,
        t_max, `out`, `stream` and the refusals as trace_closest_device."""
        who = "trace_hits_device"
        k = int(k)
        names = (["count", "object"] + [w for w in ("t", "hit_point", "normal") if w in want] if k != 0 else []) + [w for w in ("total",) if w in want]
        refusal = None
        if k < 0 or (out is None and k > TRACE_HITS_K_MAX):  # (too large a k with the caller's outputs: the library says it)
            refusal = "k must be 0 .. %d, got %d" % (TRACE_HITS_K_MAX, k)
        elif not names:
            refusal = "k = 0 is the count alone: want must hold 'total'"
        return _device_query(self, who, accel, lambda: _device_rays(self, who, origin, direction, t_max), _trace_hits_outputs(max(k, 0)), names, want,
                                  ("count", "total", "object", "t", "hit_point", "normal"), stream, out, origin, k=k, known=_trace_hits_outputs(1),
                                  refusal=refusal)


SKYBOX_FACE_FILES = ("right", "left", "top", "bottom", "front", "back")  # scene.cpp:333


def load_skybox_dir(sky_dir, ext=".jpg"):
    """Decode <dir>/{right,left,top,bottom,front,back}.jpg the way Scene::LoadSkybox asks DevIL to
    (RGB bytes, lower-left origin).  Decoding is host-binding work (PIL here, DevIL in the reference);
    the texel values are whatever the decoder produces."""
    from PIL import Image
    faces = []
    for name in SKYBOX_FACE_FILES:
        img = Image.open(os.path.join(sky_dir, name + ext)).convert("RGB")
        faces.append(np.ascontiguousarray(np.asarray(img)[::-1]))
    return faces
