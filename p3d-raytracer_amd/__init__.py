"""p3d-raytracer_amd — Python face of libp3d.so (the C-ABI of include/p3d.h).

Thin ctypes plumbing only: the product is the shared library (host C++ loader / BVH /
grid builders + gfx950 HIP kernels).  Nothing here computes pixels, and nothing here
touches oracle/: if libp3d.so is missing, or there is no HIP device, calls fail loudly.

The directory name has a hyphen, so import it through the root-level shim:

    import p3d_amd as p3d        # repo root on sys.path
    hs = p3d.HostScene("scene.p3f")
    dev = p3d.DeviceScene(hs, bvh=True)
    rgb, hit, stats = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4))
"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("P3D_LIB") or os.path.join(HERE, "libp3d.so")  # P3D_LIB: kernel-variant experiments

ACCEL_NONE, ACCEL_GRID, ACCEL_BVH = 0, 1, 2
WHITTED, PATHTRACE = 0, 1
TILE_ORDER_COST, TILE_ORDER_FRAME = 0, 1
STACK_LITERAL, STACK_PER_PIXEL = 0, 1
CHAIN_AUTO, CHAIN_MEGAKERNEL, CHAIN_PER_LEVEL = 0, 1, 2
SAMPLE_JITTER, SAMPLE_TENT = 0, 1
LOAD_LEGACY_F11 = 1
DEBUG_NONE, DEBUG_TEST_INTERSECT, DEBUG_DEPTH_MAP = 0, 1, 2
HANDOFF_COMPACT, HANDOFF_DENSE = 0, 1
UPDATE_REFIT, UPDATE_REBUILD = 0, 1

EXPORTS = [
    "p3d_abi_version", "p3d_last_error", "p3d_device_count", "p3d_config_default",
    "p3d_scene_create", "p3d_scene_create_device_bvh", "p3d_scene_destroy", "p3d_scene_set_skybox", "p3d_render_tile", "p3d_render_tile_device",
    "p3d_scene_status", "p3d_scene_set_tail_stream", "p3d_scene_join", "p3d_object_intercepts", "p3d_object_normal", "p3d_skybox_color",
    "p3d_trace_closest", "p3d_trace_any", "p3d_host_scene_load", "p3d_host_scene_destroy",
    "p3d_host_scene_set_resolution", "p3d_host_scene_set_lens", "p3d_host_scene_replicate_lights",
    "p3d_host_scene_desc", "p3d_host_scene_bind_device", "p3d_host_scene_has_skybox", "p3d_host_scene_load_skybox", "p3d_host_scene_skybox_face",
    "p3d_accum_create", "p3d_accum_destroy", "p3d_accum_reset", "p3d_accum_samples_done", "p3d_accum_render", "p3d_accum_render_device",
    "p3d_adaptive_create", "p3d_adaptive_destroy", "p3d_adaptive_reset", "p3d_adaptive_samples_done", "p3d_adaptive_active_pixels",
    "p3d_adaptive_render", "p3d_adaptive_render_device", "p3d_adaptive_read_state",
    "p3d_render_features", "p3d_render_features_device", "p3d_denoise_params_default", "p3d_denoiser_create",
    "p3d_denoiser_destroy", "p3d_denoise", "p3d_denoise_device", "p3d_denoise_variance", "p3d_denoise_variance_device",
    "p3d_camera_look_at", "p3d_scene_set_camera", "p3d_scene_camera", "p3d_host_scene_view",
    "p3d_temporal_params_default", "p3d_temporal_create", "p3d_temporal_destroy", "p3d_temporal_reset", "p3d_temporal_frames",
    "p3d_temporal_accumulate", "p3d_temporal_accumulate_device",
    "p3d_scene_update_prims", "p3d_scene_export_bvh", "p3d_host_scene_set_geometry",
    "p3d_scene_build_grid", "p3d_scene_export_grid", "p3d_scene_transform_prims",
    "p3d_scene_bvh_cost", "p3d_scene_set_auto_rebuild", "p3d_scene_auto_rebuild",
    "p3d_scene_update_geometry_device",
    "p3d_trace_closest_device", "p3d_trace_any_device",
    "p3d_scene_refit_device",
    "p3d_scene_set_rig", "p3d_scene_rig", "p3d_scene_pose_device",
    "p3d_host_scene_nearest", "p3d_nearest_device",
    "p3d_host_scene_nearest_k", "p3d_nearest_k_device",
    "p3d_trace_hits_device",
]


class P3DError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("p3d error %d: %s" % (code, msg))
        self.code = code


class Prim(C.Structure):
    _fields_ = [("v", C.c_float * 9), ("type", C.c_uint32), ("material", C.c_uint32), ("reserved0", C.c_uint32),
                ("n", C.c_float * 3), ("reserved1", C.c_uint32), ("bmin", C.c_float * 3), ("reserved2", C.c_uint32),
                ("bmax", C.c_float * 3), ("reserved3", C.c_uint32)]


class Xform(C.Structure):
    _fields_ = [("m", C.c_float * 12), ("sphere_scale", C.c_float), ("reserved", C.c_uint32 * 3)]


class XformRange(C.Structure):
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("xform", C.c_uint32), ("reserved", C.c_uint32)]


class GeomSource(C.Structure):
    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32), ("kind", C.c_uint32), ("n_elems", C.c_uint32),
                ("d_data", C.c_void_p), ("d_index", C.c_void_p), ("reserved", C.c_uint64 * 2)]


class BvhCost(C.Structure):
    _fields_ = [("sah", C.c_double), ("sah_baseline", C.c_double), ("n_inner", C.c_uint32), ("n_leaves", C.c_uint32),
                ("refits_since_build", C.c_uint32), ("last_update_rebuilt", C.c_uint32)]


class Material(C.Structure):
    _fields_ = [("diff_color", C.c_float * 3), ("diffuse", C.c_float), ("spec_color", C.c_float * 3),
                ("specular", C.c_float), ("shine", C.c_float), ("transmittance", C.c_float),
                ("refr_index", C.c_float), ("reflection", C.c_float), ("emission", C.c_float * 3),
                ("reserved", C.c_float)]


class Light(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("reserved0", C.c_float), ("color", C.c_float * 3),
                ("reserved1", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("eye", C.c_float * 3), ("plane_dist", C.c_float), ("u", C.c_float * 3), ("w", C.c_float),
                ("v", C.c_float * 3), ("h", C.c_float), ("n", C.c_float * 3), ("focal_ratio", C.c_float),
                ("aperture", C.c_float), ("res_x", C.c_int32), ("res_y", C.c_int32), ("reserved", C.c_int32)]


class BvhNode(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("index", C.c_uint32), ("bmax", C.c_float * 3), ("count_leaf", C.c_uint32)]


class GridDesc(C.Structure):
    _fields_ = [("bmin", C.c_float * 3), ("nx", C.c_int32), ("bmax", C.c_float * 3), ("ny", C.c_int32),
                ("nz", C.c_int32), ("n_cells", C.c_uint32), ("n_items", C.c_uint32), ("reserved", C.c_uint32),
                ("cell_start", C.POINTER(C.c_uint32)), ("cell_items", C.POINTER(C.c_uint32))]


class SceneDesc(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_prims", C.c_uint32), ("n_materials", C.c_uint32),
                ("n_lights", C.c_uint32), ("prims", C.POINTER(Prim)), ("materials", C.POINTER(Material)),
                ("lights", C.POINTER(Light)), ("camera", Camera), ("background", C.c_float * 3),
                ("n_bvh_nodes", C.c_uint32), ("bvh_nodes", C.POINTER(BvhNode)),
                ("bvh_prim_index", C.POINTER(C.c_uint32)), ("n_bvh_prim_index", C.c_uint32),
                ("bvh_max_depth", C.c_uint32), ("has_grid", C.c_uint32), ("reserved", C.c_uint32),
                ("grid", GridDesc)]


class Config(C.Structure):
    _fields_ = [("integrator", C.c_uint32), ("accel", C.c_uint32), ("max_depth", C.c_int32),
                ("spp_sqrt", C.c_uint32), ("antialiasing", C.c_uint32), ("depth_of_field", C.c_uint32),
                ("sample_disk", C.c_uint32), ("soft_shadows", C.c_uint32), ("sample_mode", C.c_uint32),
                ("light_side", C.c_float), ("gamma", C.c_float), ("collect_stats", C.c_uint32),
                ("skybox", C.c_uint32), ("tile_order", C.c_uint32), ("seed", C.c_uint64),
                ("stack_mode", C.c_uint32), ("chain_launch", C.c_uint32), ("debug_view", C.c_uint32), ("handoff_records", C.c_uint32)]


class SkyboxFace(C.Structure):
    _fields_ = [("img", C.c_void_p), ("res_x", C.c_uint32), ("res_y", C.c_uint32), ("bpp", C.c_uint32),
                ("reserved", C.c_uint32)]


class SkyboxDesc(C.Structure):
    _fields_ = [("face", SkyboxFace * 6)]


class Tile(C.Structure):
    _fields_ = [("x0", C.c_int32), ("y0", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("stripe_h", C.c_int32), ("stripe_stride", C.c_int32)]


class AdaptiveParams(C.Structure):
    _fields_ = [("rel_error", C.c_float), ("min_samples", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class DenoiseParams(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_luma", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("sigma_albedo", C.c_float), ("gamma", C.c_float), ("reserved", C.c_uint32 * 2)]


class TemporalParams(C.Structure):
    _fields_ = [("alpha", C.c_float), ("alpha_moments", C.c_float), ("max_history", C.c_float), ("depth_tolerance", C.c_float),
                ("normal_tolerance", C.c_float), ("variance_min_history", C.c_uint32), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("reserved", C.c_uint32 * 2)]


class DebugPlan(C.Structure):
    """p3d_debug_plan (csrc/p3d_debug.h): what the kernel choosers read of the plan of one launch"""
    _fields_ = [(k, C.c_uint32) for k in ("pt", "literal", "lds_scene", "lds_spill", "sub4", "per_level", "repair_tiles", "stack_mode",
                                          "spill_entries", "bound", "cap", "zero_weight_reflections")]


FramePlan = collections.namedtuple("FramePlan", [k for k, _ in DebugPlan._fields_])
PLAN_MODES = {"frame": 0, "adaptive": 1, "features": 2}
STACK_LDS6, STACK_WINDOW, STACK_LDS8 = 0, 1, 2  # FramePlan.stack_mode (csrc/device_core.hpp "Stack")


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "rays_primary", "rays_shadow", "rays_reflect", "rays_refract", "rays_bounce", "rays_light",
        "node_tests", "sphere_tests", "tri_tests", "box_tests", "plane_tests", "shaded_hits", "pixels",
        "max_stack")] + [("kernel_ms", C.c_double)] + [(n, C.c_uint64) for n in (
        "handoff_checked", "handoff_redone", "handoff_rounds")] + [("pass1_ms", C.c_double), ("handoff_ms", C.c_double),
                                                                ("handoff_dense_retry", C.c_uint64)]

    @property
    def rays(self):
        return (self.rays_primary + self.rays_shadow + self.rays_reflect + self.rays_refract
                + self.rays_bounce + self.rays_light)

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def algorithmic_bytes(self):
        """DESIGN.md / SURVEY.md §8(d): bytes the algorithm has to look at."""
        return (32 * self.node_tests + 16 * self.sphere_tests + 48 * self.tri_tests + 24 * self.box_tests
                + 24 * self.plane_tests + 64 * self.shaded_hits + 16 * self.pixels)


def build(force=False):
    """Compile libp3d.so for gfx950 in-tree (hipcc cross-compiles without a GPU).  What is stale is the Makefile's
    decision (its prerequisites are every source under csrc/ and host/): `make` does nothing when the library is up to
    date, and without hipcc `make -q` only asks."""
    if os.environ.get("P3D_LIB"):  # a variant library (`make variant`) is not this Makefile target: it only has to exist
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("P3D_LIB names %s, which does not exist (build it with `make variant`)" % LIB_PATH)
        return LIB_PATH
    make = ["make", "-C", HERE, "libp3d.so"]
    if os.path.exists("/opt/rocm/bin/hipcc"):
        subprocess.check_call(make, stdout=subprocess.DEVNULL)
        return LIB_PATH
    stale = force or not os.path.exists(LIB_PATH)
    if not stale:
        try:
            stale = subprocess.call(make + ["-q"], stdout=subprocess.DEVNULL) != 0
        except OSError:  # no make either: nothing can say more than that the library is there
            pass
    if stale:
        raise RuntimeError("libp3d.so is missing/stale and hipcc is not available to build it")
    return LIB_PATH


_lib = None


def lib():
    """Load libp3d.so.  Raises if it is absent: there is no Python or CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C p3d-raytracer_amd`" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.p3d_last_error.restype = C.c_char_p
        L.p3d_abi_version.restype = C.c_uint32
        L.p3d_host_scene_load.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.p3d_host_scene_destroy.argtypes = [C.c_void_p]
        L.p3d_host_scene_set_resolution.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        L.p3d_host_scene_set_lens.argtypes = [C.c_void_p, C.c_float, C.c_float]
        L.p3d_host_scene_replicate_lights.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
        L.p3d_host_scene_desc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.POINTER(SceneDesc))]
        L.p3d_scene_create.argtypes = [C.POINTER(SceneDesc), C.c_int, C.POINTER(C.c_void_p)]
        L.p3d_host_scene_bind_device.argtypes = [C.c_void_p, C.c_void_p]
        L.p3d_host_scene_has_skybox.argtypes = [C.c_void_p]
        L.p3d_host_scene_load_skybox.argtypes = [C.c_void_p, C.c_char_p]
        L.p3d_host_scene_skybox_face.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.p3d_scene_destroy.argtypes = [C.c_void_p]
        L.p3d_scene_set_skybox.argtypes = [C.c_void_p, C.POINTER(SkyboxDesc)]
        L.p3d_render_tile.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(Tile), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(Stats)]
        L.p3d_render_tile_device.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(Tile), C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.p3d_trace_closest.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
        L.p3d_trace_any.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_object_intercepts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_object_normal.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
        L.p3d_skybox_color.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.p3d_scene_status.argtypes = [C.c_void_p]
        L.p3d_scene_set_tail_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.p3d_scene_join.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.p3d_debug_scene_limits.argtypes = [C.c_void_p, C.c_void_p]  # csrc/p3d_debug.h: not part of include/p3d.h
        L.p3d_debug_frame_plan.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(Tile), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(DebugPlan)]
        L.p3d_debug_frame_plan_size.restype = C.c_uint32
        L.p3d_accum_create.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(Tile), C.POINTER(C.c_void_p)]
        L.p3d_accum_destroy.argtypes = [C.c_void_p]
        L.p3d_accum_destroy.restype = None
        L.p3d_accum_reset.argtypes = [C.c_void_p]
        L.p3d_accum_samples_done.argtypes = [C.c_void_p]
        L.p3d_accum_samples_done.restype = C.c_uint32
        L.p3d_accum_render.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Stats)]
        L.p3d_accum_render_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.POINTER(Stats)]
        L.p3d_adaptive_create.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(Tile), C.POINTER(AdaptiveParams),
                                          C.POINTER(C.c_void_p)]
        L.p3d_adaptive_destroy.argtypes = [C.c_void_p]
        L.p3d_adaptive_destroy.restype = None
        L.p3d_adaptive_reset.argtypes = [C.c_void_p]
        L.p3d_adaptive_samples_done.argtypes = [C.c_void_p]
        L.p3d_adaptive_samples_done.restype = C.c_uint32
        L.p3d_adaptive_active_pixels.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        L.p3d_adaptive_render.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(Stats)]
        L.p3d_adaptive_render_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.POINTER(Stats)]
        L.p3d_adaptive_read_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_render_features.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(Tile), C.c_uint32, C.c_void_p, C.c_void_p]
        L.p3d_render_features_device.argtypes = [C.c_void_p, C.POINTER(Config), C.POINTER(Tile), C.c_uint32, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        L.p3d_denoise_params_default.argtypes = [C.POINTER(DenoiseParams)]
        L.p3d_denoise_params_default.restype = None
        L.p3d_denoiser_create.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.p3d_denoiser_destroy.argtypes = [C.c_void_p]
        L.p3d_denoiser_destroy.restype = None
        L.p3d_denoise.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]
        L.p3d_denoise_device.argtypes = [C.c_void_p, C.POINTER(DenoiseParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_denoise_variance.argtypes = [C.c_void_p, C.c_void_p]
        L.p3d_denoise_variance_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        F3 = C.c_float * 3
        L.p3d_camera_look_at.argtypes = [F3, F3, F3, C.c_float, C.c_int32, C.c_int32, C.c_float, C.c_float, C.POINTER(Camera)]
        L.p3d_scene_set_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
        L.p3d_scene_camera.argtypes = [C.c_void_p, C.POINTER(Camera)]
        L.p3d_host_scene_view.argtypes = [C.c_void_p, F3, F3, F3, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
        L.p3d_temporal_params_default.argtypes = [C.POINTER(TemporalParams)]
        L.p3d_temporal_params_default.restype = None
        L.p3d_temporal_create.argtypes = [C.c_int, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.p3d_temporal_destroy.argtypes = [C.c_void_p]
        L.p3d_temporal_destroy.restype = None
        L.p3d_temporal_reset.argtypes = [C.c_void_p]
        L.p3d_temporal_frames.argtypes = [C.c_void_p]
        L.p3d_temporal_frames.restype = C.c_uint32
        L.p3d_temporal_accumulate.argtypes = [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(Camera), C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_temporal_accumulate_device.argtypes = [C.c_void_p, C.POINTER(TemporalParams), C.POINTER(Camera), C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_scene_update_prims.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        L.p3d_scene_export_bvh.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_uint32)]
        L.p3d_host_scene_set_geometry.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.p3d_scene_build_grid.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.p3d_scene_export_grid.argtypes = [C.c_void_p, C.POINTER(GridDesc), C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p,
                                            C.POINTER(C.c_uint32)]
        L.p3d_scene_transform_prims.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                                C.POINTER(C.c_float)]
        L.p3d_scene_bvh_cost.argtypes = [C.c_void_p, C.POINTER(BvhCost)]
        L.p3d_scene_set_auto_rebuild.argtypes = [C.c_void_p, C.c_float]
        L.p3d_scene_auto_rebuild.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
        L.p3d_scene_update_geometry_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        L.p3d_trace_closest_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_trace_any_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_scene_refit_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
        L.p3d_scene_set_rig.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        L.p3d_scene_rig.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.p3d_scene_pose_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_host_scene_nearest.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_nearest_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]
        L.p3d_host_scene_nearest_k.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]
        L.p3d_nearest_k_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.p3d_trace_hits_device.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise P3DError(rc, lib().p3d_last_error().decode("utf-8", "replace"))


def device_count():
    n = lib().p3d_device_count()
    return max(n, 0)


def default_config(**kw):
    c = Config()
    lib().p3d_config_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise AttributeError(k)
        setattr(c, k, v)
    return c


def denoise_params(**kw):
    """p3d_denoise_params_default, then the fields given (iterations, sigma_color, sigma_luma, sigma_normal, sigma_depth,
    sigma_albedo, gamma, reserved)."""
    p = DenoiseParams()
    lib().p3d_denoise_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_uint32 * 2)(*v) if k == "reserved" else v)
    return p


def temporal_params(**kw):
    """p3d_temporal_params_default, then the fields given (alpha, alpha_moments, max_history, depth_tolerance,
    normal_tolerance, variance_min_history, sigma_normal, sigma_depth, reserved)."""
    p = TemporalParams()
    lib().p3d_temporal_params_default(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise AttributeError(k)
        setattr(p, k, (C.c_uint32 * 2)(*v) if k == "reserved" else v)
    return p


def _f3(v):
    v = [float(x) for x in v]
    if len(v) != 3:
        raise ValueError("a 3-vector is needed, got %r" % (v,))
    return (C.c_float * 3)(*v)


def look_at(from_, at, up, angle, res, aperture_ratio=0.0, focal_ratio=1.0):
    """p3d_camera_look_at: the Camera the .p3f loader builds for a `v` block with these values (camera.h:34-63);
    res = (res_x, res_y)."""
    cam = Camera()
    _check(lib().p3d_camera_look_at(_f3(from_), _f3(at), _f3(up), float(angle), int(res[0]), int(res[1]), float(aperture_ratio),
                                    float(focal_ratio), C.byref(cam)))
    return cam


def whitted_config(accel=ACCEL_BVH, max_depth=4, **kw):
    """SURVEY.md §8(d) Whitted configs: no AA / soft shadows / DOF, one ray per pixel."""
    base = dict(integrator=WHITTED, accel=accel, max_depth=max_depth, spp_sqrt=1, antialiasing=0,
                depth_of_field=0, soft_shadows=0)
    base.update(kw)
    return default_config(**base)


def pathtrace_config(accel=ACCEL_BVH, spp_sqrt=16, max_depth=20, dof=0, **kw):
    base = dict(integrator=PATHTRACE, accel=accel, max_depth=max_depth, spp_sqrt=spp_sqrt, antialiasing=1,
                depth_of_field=dof, sample_disk=1, soft_shadows=0)
    base.update(kw)
    return default_config(**base)


def _xform_arrays(ranges, xforms, sphere_scale):
    """(ranges as (n, 3) int64, xforms as (k, 12) float32, sphere_scale as (k,) float32) of the arguments of
    transformed / DeviceScene.transform_prims"""
    r = np.asarray(list(ranges), np.int64).reshape(-1, 3)
    m = np.ascontiguousarray(xforms, np.float32)
    if m.ndim == 3 and m.shape[1:] == (3, 4):
        m = m.reshape(-1, 12)
    if m.ndim != 2 or m.shape[1] != 12:
        raise ValueError("xforms: an (n, 3, 4) or (n, 12) array is needed, got shape %r" % (m.shape,))
    sc = np.ones(len(m), np.float32) if sphere_scale is None else np.ascontiguousarray(sphere_scale, np.float32).reshape(-1)
    if len(sc) != len(m):
        raise ValueError("sphere_scale: %d values for %d transforms" % (len(sc), len(m)))
    return r, m, sc


def transformed(prim_type, prim_v, ranges, xforms, sphere_scale=None):
    """What p3d_scene_transform_prims computes for the nine geometry floats, stated in numpy float32, one rounded operation
    at a time: -> (objects, new_v), the arguments of HostScene.set_geometry that bring a host scene along.  `ranges`: an
    iterable of (first, count, xform); `xforms`: (n, 3, 4) or (n, 12) float32, row-major; `sphere_scale`: n values, default
    1.  A point: x' = ((m0 x + m1 y) + m2 z) + m3; the vertices of a triangle, the centre of a sphere (radius' = radius *
    sphere_scale) and min / max of a box are points.  prim_v holds the REST geometry.  Planes are refused, and boxes unless
    the transform is a positive scale per axis and a translation."""
    r, m, sc = _xform_arrays(ranges, xforms, sphere_scale)
    prim_type = np.asarray(prim_type)
    v = np.ascontiguousarray(prim_v, np.float32).reshape(-1, 9)
    objects, rows = [], []
    for first, count, x in r:
        if count <= 0 or first < 0 or first + count > len(v) or not 0 <= x < len(m):
            raise ValueError("transformed: bad range (%d, %d, %d)" % (first, count, x))
        idx = np.arange(first, first + count)
        kind = prim_type[idx]
        if (kind == 3).any():
            raise ValueError("transformed: range (%d, %d) covers a plane" % (first, count))
        t = m[x].reshape(3, 4)
        if (kind == 2).any() and not ((np.diag(t[:, :3]) > 0).all() and (t[:, :3][~np.eye(3, dtype=bool)] == 0).all()):
            raise ValueError("transformed: range (%d, %d) covers a box, and transform %d is not positive-diagonal" % (first, count, x))
        out = v[idx].copy()
        for cols, k in (((0,), 0), ((0, 3, 6), 1), ((0, 3), 2)):
            sel = kind == k
            for c in cols:
                px, py, pz = v[idx, c][sel], v[idx, c + 1][sel], v[idx, c + 2][sel]
                for row in range(3):
                    out[sel, c + row] = ((t[row, 0] * px + t[row, 1] * py) + t[row, 2] * pz) + t[row, 3]
        sph = kind == 0
        out[sph, 3] = v[idx, 3][sph] * sc[x]
        objects.append(idx)
        rows.append(out)
    if not objects:
        return np.zeros(0, np.uint32), np.zeros((0, 9), np.float32)
    return np.concatenate(objects).astype(np.uint32), np.concatenate(rows).astype(np.float32)


def deformed(prim_v, first, positions, indices=None):
    """The host route of DeviceScene.update_triangles, a plain gather in numpy: triangle first + k takes the positions
    indices[k] of `positions` ((V, 3) float32), or 3k, 3k + 1, 3k + 2 without indices -> (objects, rows), the arguments of
    HostScene.set_geometry that bring a host scene along.  prim_v (the scene's (n, 9) geometry) bounds the range."""
    pos = np.ascontiguousarray(positions, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 3:
        raise ValueError("deformed: positions must be (V, 3), got shape %r" % (pos.shape,))
    if indices is None:
        if len(pos) % 3:
            raise ValueError("deformed: a soup needs 3 positions per triangle, got %d" % len(pos))
        idx = np.arange(len(pos), dtype=np.int64).reshape(-1, 3)
    else:
        idx = np.asarray(indices)
        if idx.ndim != 2 or idx.shape[1] != 3 or idx.dtype.kind not in "iu":
            raise ValueError("deformed: indices must be an integer (F, 3) array")
        idx = idx.astype(np.uint32).astype(np.int64) if idx.dtype.itemsize == 4 else idx.astype(np.int64)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(pos)):
            raise ValueError("deformed: an index is outside the %d positions" % len(pos))
    n = len(np.asarray(prim_v).reshape(-1, 9))
    if first < 0 or len(idx) == 0 or first + len(idx) > n:
        raise ValueError("deformed: objects [%d, %d) of %d" % (first, first + len(idx), n))
    return np.arange(first, first + len(idx), dtype=np.uint32), np.ascontiguousarray(pos[idx].reshape(-1, 9))


def deformed_spheres(prim_v, first, centre_radius):
    """The host route of DeviceScene.update_spheres: sphere first + k takes centre and radius centre_radius[k] ((N, 4)
    float32), the other five floats of its row stay -> (objects, rows) for HostScene.set_geometry."""
    cr = np.ascontiguousarray(centre_radius, np.float32)
    if cr.ndim != 2 or cr.shape[1] != 4:
        raise ValueError("deformed_spheres: centre_radius must be (N, 4), got shape %r" % (cr.shape,))
    v = np.ascontiguousarray(prim_v, np.float32).reshape(-1, 9)
    if first < 0 or len(cr) == 0 or first + len(cr) > len(v):
        raise ValueError("deformed_spheres: objects [%d, %d) of %d" % (first, first + len(cr), len(v)))
    rows = v[first:first + len(cr)].copy()
    rows[:, :4] = cr
    return np.arange(first, first + len(cr), dtype=np.uint32), rows


def _device_rows(x, what, cols, dtypes, device):
    """(address, rows) of a contiguous (rows, cols) CUDA/HIP torch.Tensor of one of `dtypes` on `device`, or of a raw
    (address, rows) pair, which is taken at its word.  Anything else: P3DError, and the library is not called."""
    if isinstance(x, tuple) and len(x) == 2 and not hasattr(x[0], "data_ptr"):
        ptr, rows = int(x[0]), int(x[1])
        if ptr <= 0 or rows <= 0:
            raise P3DError(-1, "%s: a raw pair needs an address and a row count > 0" % what)
        return ptr, rows
    if not (hasattr(x, "data_ptr") and hasattr(x, "is_cuda")):
        raise P3DError(-1, "%s: a CUDA/HIP torch.Tensor or an (address, rows) pair is needed, got %s" % (what, type(x).__name__))
    if str(x.dtype).replace("torch.", "") not in dtypes:
        raise P3DError(-1, "%s: dtype %s, needed: %s" % (what, x.dtype, " or ".join(dtypes)))
    if x.dim() != 2 or x.shape[1] != cols or x.shape[0] == 0:
        raise P3DError(-1, "%s: shape %r, needed: (n, %d) with n > 0" % (what, tuple(x.shape), cols))
    if not x.is_contiguous():
        raise P3DError(-1, "%s: the tensor is not contiguous" % what)
    if not x.is_cuda:
        raise P3DError(-1, "%s: the tensor is in host memory (device %s)" % (what, x.device))
    if x.device.index is not None and x.device.index != device:
        raise P3DError(-1, "%s: the tensor is on device %d, the scene on device %d" % (what, x.device.index, device))
    return int(x.data_ptr()), int(x.shape[0])


def _device_vector(x, what, dtypes, device):
    """_device_rows for one value per row: a contiguous (rows,) tensor, or a raw (address, rows) pair"""
    if hasattr(x, "data_ptr") and hasattr(x, "dim"):
        if x.dim() != 1:
            raise P3DError(-1, "%s: shape %r, needed: (n,) with n > 0" % (what, tuple(x.shape)))
        x = x.unsqueeze(1)  # (a strided vector stays non-contiguous)
    return _device_rows(x, what, 1, dtypes, device)


def _device_blocks(x, what, tail, dtypes, device):
    """_device_rows for a block of values per row: a contiguous (rows,) + tail tensor (tail: two sizes), or a raw (address, rows) pair"""
    if hasattr(x, "data_ptr") and hasattr(x, "dim"):
        if x.dim() != 3 or tuple(x.shape[1:]) != tuple(tail):
            raise P3DError(-1, "%s: shape %r, needed: (n, %d, %d) with n > 0" % (what, tuple(x.shape), tail[0], tail[1]))
        if x.is_contiguous():
            x = x.view(x.shape[0], tail[0] * tail[1])
        else:
            raise P3DError(-1, "%s: the tensor is not contiguous" % what)
    return _device_rows(x, what, tail[0] * tail[1], dtypes, device)


_TRACE_OUTPUTS = {"hit_id": ("int32", None), "t": ("float32", None), "hit_point": ("float32", 3), "normal": ("float32", 3)}
_NEAREST_OUTPUTS = {"object": ("int32", None), "dist": ("float32", None), "closest": ("float32", 3), "normal": ("float32", 3)}
NEAREST_K_MAX = 16  # P3D_NEAREST_K_MAX


def _nearest_k_outputs(k):
    """name -> (dtype, columns) of p3d_nearest_k_device's outputs for this k: k rows per point"""
    return {"count": ("int32", None), "object": ("int32", k), "dist": ("float32", k), "closest": ("float32", (k, 3)), "normal": ("float32", (k, 3))}


TRACE_HITS_K_MAX = 16  # P3D_TRACE_HITS_K_MAX


def _trace_hits_outputs(k):
    """name -> (dtype, columns) of p3d_trace_hits_device's outputs for this k: k rows per ray (k = 0: the count alone)"""
    rows = {"count": ("int32", None), "object": ("int32", k), "t": ("float32", k), "hit_point": ("float32", (k, 3)), "normal": ("float32", (k, 3))}
    return dict(rows if k else {}, total=("int32", None))


class HostScene:
    """Scene::load_p3f + BVH::build / Grid::Build on the host (C++ inside libp3d.so)."""

    def __init__(self, path, legacy_f11=False):
        self._L = lib()
        h = C.c_void_p()
        _check(self._L.p3d_host_scene_load(os.fsencode(path), LOAD_LEGACY_F11 if legacy_f11 else 0, C.byref(h)))
        self._h = h
        self.path = path

    def close(self):
        if getattr(self, "_h", None):
            self._L.p3d_host_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = len(p)
        m = None
        if max_dist is not None:
            m = np.ascontiguousarray(max_dist, np.float32).reshape(-1)
            if len(m) != n:
                raise ValueError("nearest: %d points, %d limits" % (n, len(m)))
        obj, dist, closest = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32)
        _check(self._L.p3d_host_scene_nearest(self._h, n, p.ctypes.data, m.ctypes.data if m is not None else None, obj.ctypes.data,
                                              dist.ctypes.data, closest.ctypes.data))
        return obj, dist, closest

    def nearest_k(self, points, k, max_dist=None):
        """p3d_host_scene_nearest_k: for every point the (at most) k objects whose surfaces are nearest, nearer than max_dist
        (float32 (n,), or None: no limit), ordered by (distance, object index), by brute force on the CPU -> (count int32 (n,),
        object int32 (n, k), dist float32 (n, k), closest float32 (n, k, 3)); rows from count on hold -1, FLT_MAX and zeros.
        count == k: there may be more.  1 <= k <= NEAREST_K_MAX."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n, k = len(p), int(k)
        m = None
        if max_dist is not None:
            m = np.ascontiguousarray(max_dist, np.float32).reshape(-1)
            if len(m) != n:
                raise ValueError("nearest_k: %d points, %d limits" % (n, len(m)))
        rows = max(k, 0)
        count, obj = np.zeros(n, np.int32), np.zeros((n, rows), np.int32)
        dist, closest = np.zeros((n, rows), np.float32), np.zeros((n, rows, 3), np.float32)
        _check(self._L.p3d_host_scene_nearest_k(self._h, n, k & 0xffffffff, p.ctypes.data, m.ctypes.data if m is not None else None,
                                                count.ctypes.data, obj.ctypes.data, dist.ctypes.data, closest.ctypes.data))
        return count, obj, dist, closest

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


def tree_cost(tree):
    """The SAH cost p3d_scene_bvh_cost reports (include/p3d.h), evaluated in float64 on a tree with the bvh_* keys of
    DeviceScene.export_bvh() or HostScene.arrays(bvh=True): A = (dx dy + dy dz) + dz dx per node, inner nodes count once, a
    leaf once per object, over A(root).  No nodes or a root without area: 0."""
    lo, hi = np.asarray(tree["bvh_bmin"], np.float32).reshape(-1, 3), np.asarray(tree["bvh_bmax"], np.float32).reshape(-1, 3)
    if len(lo) == 0:
        return 0.0
    d = hi.astype(np.float64) - lo.astype(np.float64)
    area = (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2]) + d[:, 2] * d[:, 0]
    count_leaf = np.asarray(tree["bvh_count_leaf"], np.uint32)
    weight = np.where(count_leaf & np.uint32(0x80000000), (count_leaf & np.uint32(0x7fffffff)).astype(np.float64), 1.0)
    return float((weight * area).sum() / area[0]) if area[0] > 0 else 0.0


class DeviceScene:
    """p3d_scene_create: the flattened scene resident in HBM of one MI355X."""

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

    def close(self):
        if getattr(self, "_h", None):
            self._L.p3d_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

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
        if len(r) and (r.min() < 0 or r.max() > 0xffffffff):
            raise P3DError(-1, "transform_prims: a range does not fit uint32")
        rg = (XformRange * max(len(r), 1))()
        for i, (first, count, x) in enumerate(r):
            rg[i] = XformRange(int(first), int(count), int(x), 0)
        xf = (Xform * max(len(m), 1))()
        for i in range(len(m)):
            xf[i].m[:] = m[i].tolist()
            xf[i].sphere_scale = float(sc[i])
        ms = C.c_float(0)
        _check(self._L.p3d_scene_transform_prims(self._h, len(r), C.cast(rg, C.c_void_p) if len(r) else None, len(m),
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
        src = list(sources)
        arr = (GeomSource * max(len(src), 1))(*src)
        ms = C.c_float(0)
        _check(self._L.p3d_scene_update_geometry_device(self._h, len(src), C.cast(arr, C.c_void_p) if src else None, int(mode), C.byref(ms)))
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
        src = list(sources)
        arr = (GeomSource * max(len(src), 1))(*src)
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_scene_refit_device(self._h, len(src), C.cast(arr, C.c_void_p) if src else None, C.c_void_p(raw or None)))

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
        if len(r) and (r.min() < 0 or r.max() > 0xffffffff):
            raise P3DError(-1, "set_rig: a range does not fit uint32")
        rg = (XformRange * max(len(r), 1))()
        for i, (first, count, x) in enumerate(r):
            rg[i] = XformRange(int(first), int(count), int(x), 0)
        _check(self._L.p3d_scene_set_rig(self._h, len(r), C.cast(rg, C.c_void_p) if len(r) else None, int(n_xforms)))

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
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_scene_pose_device(self._h, k, C.c_void_p(d_x), C.c_void_p(d_s) if d_s else None, C.c_void_p(raw or None)))

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
        rgb = np.zeros((t.h, t.w, 3), np.float32)
        hit = np.zeros((t.h, t.w), np.int32)
        rgb8 = np.zeros((t.h, t.w, 3), np.uint8) if want_rgb8 else None
        st = Stats()
        _check(self._L.p3d_render_tile(self._h, C.byref(cfg), C.byref(t), rgb.ctypes.data, hit.ctypes.data,
                                       rgb8.ctypes.data if want_rgb8 else None, C.byref(st) if stats else None))
        if want_rgb8:
            return rgb, hit, rgb8, st
        return rgb, hit, st

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
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_scene_set_tail_stream(self._h, C.c_void_p(raw) if raw else None))

    def join(self, stream=None, host_wait=False):
        """p3d_scene_join: make `stream` (or, with host_wait, the calling thread) wait for the scene's last frame, tail included."""
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_scene_join(self._h, C.c_void_p(raw) if raw else None, 1 if host_wait else 0))

    def debug_limits(self, trip_bound=0, max_rounds=0, halo_chain=0, leftover_pool=0):
        """Tests only (csrc/p3d_debug.h, not part of include/p3d.h): shrink limits of THIS scene so that the device-side
        error paths fire; all 0 = the real limits.  Refused unless the process was started with P3D_TEST_HOOKS=1."""
        lim = (C.c_uint32 * 4)(trip_bound, max_rounds, halo_chain, leftover_pool)
        _check(self._L.p3d_debug_scene_limits(self._h, C.cast(lim, C.c_void_p)))

    def staged_f4(self, cfg, tile=None):
        """csrc/p3d_debug.h, read-only: the float4s a frame of `cfg` over `tile` copies into LDS (0: the scene is not
        staged, the kernels traverse it from global memory)."""
        n = C.c_uint32(0)
        self._L.p3d_debug_staged_f4.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
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
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_render_features_device(self._h, C.byref(cfg), C.byref(tile or self.full_tile()), int(samples),
                                                  C.c_void_p(d_normal_depth or None), C.c_void_p(d_albedo_cov or None),
                                                  C.c_void_p(raw or None)))

    def render_device(self, cfg, tile, d_rgb=0, d_hit=0, d_rgb8=0, stream=0, stats=None):
        """Device-buffer form: raw HBM addresses (e.g. torch.Tensor.data_ptr()) and a hipStream_t."""
        _check(self._L.p3d_render_tile_device(self._h, C.byref(cfg), C.byref(tile), C.c_void_p(d_rgb or None),
                                              C.c_void_p(d_hit or None), C.c_void_p(d_rgb8 or None),
                                              C.c_void_p(stream or None), C.byref(stats) if stats is not None else None))

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

    def _device_rays(self, who, origin, direction, t_max):
        """(address of origin, of direction, of t_max or None, n) of the rays of a device query, or P3DError"""
        d_o, n = _device_rows(origin, who + ": origin", 3, ("float32",), self.device)
        d_d, n_d = _device_rows(direction, who + ": direction", 3, ("float32",), self.device)
        d_tm, n_tm = _device_vector(t_max, who + ": t_max", ("float32",), self.device) if t_max is not None else (None, n)
        if n_d != n or n_tm != n:
            raise P3DError(-1, "%s: %d origins, %d directions%s" % (who, n, n_d, "" if t_max is None else ", %d limits" % n_tm))
        return d_o, d_d, d_tm, n

    def _device_outputs(self, who, names, n, out, like, table, rows_of):
        """name -> (tensor or None, address) for the outputs `names`: taken from the dict `out` (tensors or raw (address, rows)
        pairs, checked like the inputs), or allocated on the scene's device when `out` is None"""
        res = {}
        for name in names:
            dtype, cols = table[name]
            if out is None:
                import torch
                dev = like.device if hasattr(like, "device") else torch.device("cuda", self.device)
                tail = () if cols is None else tuple(cols) if isinstance(cols, tuple) else (cols,)
                tensor = torch.empty((n,) + tail, dtype=getattr(torch, dtype), device=dev)
            else:
                if name not in out:
                    raise P3DError(-1, "%s: out has no %r" % (who, name))
                tensor = out[name]
            what = "%s: out[%r]" % (who, name)
            if cols is None:
                ptr, rows = _device_vector(tensor, what, (dtype,), self.device)
            elif isinstance(cols, tuple):
                ptr, rows = _device_blocks(tensor, what, cols, (dtype,), self.device)
            else:
                ptr, rows = _device_rows(tensor, what, cols, (dtype,), self.device)
            if rows != n:
                raise P3DError(-1, "%s: %d rows for %d %s" % (what, rows, n, rows_of))
            res[name] = (tensor, ptr)
        return res

    def _device_points(self, who, points, max_dist):
        """(address of points, of max_dist or None, n) of the points of a device query, or P3DError"""
        d_p, n = _device_rows(points, who + ": points", 3, ("float32",), self.device)
        d_m, n_m = _device_vector(max_dist, who + ": max_dist", ("float32",), self.device) if max_dist is not None else (None, n)
        if n_m != n:
            raise P3DError(-1, "%s: %d points, %d limits" % (who, n, n_m))
        return d_p, d_m, n

    def _device_query(self, who, accel, inputs, table, names, want, order, stream, out, like, rows_of="rays", k=None, known=None, refusal=None):
        """What the *_device queries share.  In this order: a name in `want` that `known` (default: `table`) does not hold is
        refused; inputs() gives the input addresses and, last, n; `refusal`, the caller's own (about k), is raised if there is
        one; the outputs `names` are resolved against `table`; and L.p3d_<who> is called with (scene, accel, n, [k,] inputs,
        the outputs in the C order `order` - null where not in names -, stream) -> {name: tensor}"""
        unknown = [w for w in want if w not in (table if known is None else known)]
        if unknown:
            raise P3DError(-1, "%s: unknown output %r" % (who, unknown[0]))
        *addresses, n = inputs()
        if refusal:
            raise P3DError(-1, "%s: %s" % (who, refusal))
        res = self._device_outputs(who, names, n, out, like, table, rows_of)
        args = ([] if k is None else [k & 0xffffffff]) + [C.c_void_p(a) for a in addresses]
        args += [C.c_void_p(res[name][1]) if name in res else None for name in order]
        raw = getattr(stream, "cuda_stream", stream)
        _check(getattr(self._L, "p3d_" + who)(self._h, int(accel), n, *args, C.c_void_p(raw or None)))
        return {name: v[0] for name, v in res.items()}

    def trace_closest_device(self, accel, origin, direction, t_max=None, want=("hit_id", "t"), stream=0, out=None):
        """p3d_trace_closest_device: the closest hits of n rays held in device memory, enqueued on `stream` (a torch.cuda.Stream
        or a raw hipStream_t; 0 = the default stream) without a wait -> {name: tensor} for the names in `want` ("hit_id", always
        there, "t", "hit_point", "normal").  origin, direction: contiguous float32 (n, 3) CUDA/HIP tensors on the scene's device,
        or raw (address, rows) pairs; t_max: float32 (n,), a hit is kept only if t < t_max.  `out`: a dict of tensors (or raw
        pairs) to write into instead of new ones.  A tensor on the host, of another dtype or shape, not contiguous, or row
        counts that differ raise P3DError before the library is called.  Read the results once the stream has passed the call."""
        who = "trace_closest_device"
        names = ["hit_id"] + [w for w in ("t", "hit_point", "normal") if w in want]
        return self._device_query(who, accel, lambda: self._device_rays(who, origin, direction, t_max), _TRACE_OUTPUTS, names, want,
                                  ("hit_id", "t", "hit_point", "normal"), stream, out, origin)

    def trace_any_device(self, accel, origin, direction, t_max=None, stream=0, out=None):
        """p3d_trace_any_device -> {"occluded": uint8 (n,) tensor}.  Without t_max the reference's shadow feeler (trace_any: no
        distance limit); with t_max (float32 (n,)) the segment query: 1 iff some object is hit at t < t_max, for ACCEL_NONE and
        ACCEL_BVH (the grid is refused).  Arguments and stream as trace_closest_device."""
        who = "trace_any_device"
        return self._device_query(who, accel, lambda: self._device_rays(who, origin, direction, t_max), {"occluded": ("uint8", None)},
                                  ["occluded"], (), ("occluded",), stream, out, origin)

    def nearest_device(self, accel, points, max_dist=None, want=("object", "dist"), stream=0, out=None):
        """p3d_nearest_device: for n points held in device memory the object whose surface is nearest, enqueued on `stream`
        without a wait -> {name: tensor} for the names in `want` ("object", always there, "dist", "closest", "normal").  points:
        a contiguous float32 (n, 3) CUDA/HIP tensor on the scene's device, or a raw (address, rows) pair; max_dist: float32 (n,),
        an object counts only nearer than it.  ACCEL_NONE and ACCEL_BVH (not over a scene with planes); the answers are
        HostScene.nearest's, bit for bit.  `out`, `stream` and the refusals as trace_closest_device."""
        who = "nearest_device"
        names = ["object"] + [w for w in ("dist", "closest", "normal") if w in want]
        return self._device_query(who, accel, lambda: self._device_points(who, points, max_dist), _NEAREST_OUTPUTS, names, want,
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
        return self._device_query(who, accel, lambda: self._device_points(who, points, max_dist), _nearest_k_outputs(max(k, 0)), names, want,
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
        return self._device_query(who, accel, lambda: self._device_rays(who, origin, direction, t_max), _trace_hits_outputs(max(k, 0)), names, want,
                                  ("count", "total", "object", "t", "hit_point", "normal"), stream, out, origin, k=k, known=_trace_hits_outputs(1),
                                  refusal=refusal)


class Accumulator:
    """p3d_accum (include/p3d.h): one anti-aliased frame of a DeviceScene rendered in passes over its samples, the running
    sums kept on the device.  Every pass renders samples [samples_done, samples_done + n) of every pixel; rgb is the mean of
    the samples so far, hit_id the first sample's hit.  Close it (or let it go) before the scene."""

    def __init__(self, scene, cfg, tile):
        self._L = scene._L
        self.scene = scene  # (keeps the scene alive while the accumulator is)
        self.cfg = cfg
        self.tile = tile
        self.total = int(cfg.spp_sqrt) ** 2
        h = C.c_void_p()
        _check(self._L.p3d_accum_create(scene._h, C.byref(cfg), C.byref(tile), C.byref(h)))
        self._h = h

    @property
    def samples_done(self):
        return int(self._L.p3d_accum_samples_done(self._h))

    def reset(self):
        """Back to 0 samples (also what lets an accumulator whose pass failed render again)."""
        _check(self._L.p3d_accum_reset(self._h))

    def render(self, n, want_rgb8=False, stats=True):
        """p3d_accum_render: the next n samples; returns numpy arrays, the same tuple as DeviceScene.render."""
        t = self.tile
        rgb = np.zeros((t.h, t.w, 3), np.float32)
        hit = np.zeros((t.h, t.w), np.int32)
        rgb8 = np.zeros((t.h, t.w, 3), np.uint8) if want_rgb8 else None
        st = Stats()
        _check(self._L.p3d_accum_render(self._h, int(n), rgb.ctypes.data, hit.ctypes.data,
                                        rgb8.ctypes.data if want_rgb8 else None, C.byref(st) if stats else None))
        if want_rgb8:
            return rgb, hit, rgb8, st
        return rgb, hit, st

    def render_device(self, n, d_rgb=0, d_hit=0, d_rgb8=0, stream=0, stats=None):
        """p3d_accum_render_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); without stats the pass
        is only enqueued - DeviceScene.status() reports what the device detected."""
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_accum_render_device(self._h, int(n), C.c_void_p(d_rgb or None), C.c_void_p(d_hit or None),
                                               C.c_void_p(d_rgb8 or None), C.c_void_p(raw or None),
                                               C.byref(stats) if stats is not None else None))

    def close(self):
        if getattr(self, "_h", None):
            self._L.p3d_accum_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AdaptiveAccumulator:
    """p3d_adaptive (include/p3d.h): a progressive path-traced frame whose pixels stop taking samples once converged.
    Every pass renders samples [samples_done, samples_done + n) of the still-active pixels and writes every pixel: a
    pixel that stopped after k samples holds the bits a plain Accumulator holds after k.  Close it before the scene."""

    def __init__(self, scene, cfg, tile, rel_error, min_samples=16, reserved=(0, 0)):
        self._L = scene._L
        self.scene = scene
        self.cfg = cfg
        self.tile = tile
        self.total = int(cfg.spp_sqrt) ** 2
        prm = AdaptiveParams(float(rel_error), int(min_samples), (C.c_uint32 * 2)(*reserved))
        h = C.c_void_p()
        _check(self._L.p3d_adaptive_create(scene._h, C.byref(cfg), C.byref(tile), C.byref(prm), C.byref(h)))
        self._h = h

    @property
    def samples_done(self):
        return int(self._L.p3d_adaptive_samples_done(self._h))

    @property
    def active_pixels(self):
        """Pixels the next pass renders (waits for the device)."""
        n = C.c_uint32()
        _check(self._L.p3d_adaptive_active_pixels(self._h, C.byref(n)))
        return int(n.value)

    def reset(self):
        """Back to 0 samples, every pixel active (also what lets an object whose pass failed render again)."""
        _check(self._L.p3d_adaptive_reset(self._h))

    def render(self, n, want_rgb8=False, stats=True):
        """p3d_adaptive_render: the next n samples of the active pixels -> (rgb, hit, samples, [rgb8,] stats)."""
        t = self.tile
        rgb = np.zeros((t.h, t.w, 3), np.float32)
        hit = np.zeros((t.h, t.w), np.int32)
        samples = np.zeros((t.h, t.w), np.uint32)
        rgb8 = np.zeros((t.h, t.w, 3), np.uint8) if want_rgb8 else None
        st = Stats()
        _check(self._L.p3d_adaptive_render(self._h, int(n), rgb.ctypes.data, hit.ctypes.data,
                                           rgb8.ctypes.data if want_rgb8 else None, samples.ctypes.data,
                                           C.byref(st) if stats else None))
        if want_rgb8:
            return rgb, hit, samples, rgb8, st
        return rgb, hit, samples, st

    def render_device(self, n, d_rgb=0, d_hit=0, d_rgb8=0, d_samples=0, stream=0, stats=None):
        """p3d_adaptive_render_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); without stats the
        pass is only enqueued - DeviceScene.status() reports what the device detected."""
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_adaptive_render_device(self._h, int(n), C.c_void_p(d_rgb or None), C.c_void_p(d_hit or None),
                                                  C.c_void_p(d_rgb8 or None), C.c_void_p(d_samples or None),
                                                  C.c_void_p(raw or None), C.byref(stats) if stats is not None else None))

    def read_state(self):
        """p3d_adaptive_read_state (waits for the device): {"sum": (h, w, 3) float32, "sum_y2": (h, w) float32,
        "samples": (h, w) uint32, "rel_err": (h, w) float32}."""
        t = self.tile
        out = {"sum": np.zeros((t.h, t.w, 3), np.float32), "sum_y2": np.zeros((t.h, t.w), np.float32),
               "samples": np.zeros((t.h, t.w), np.uint32), "rel_err": np.zeros((t.h, t.w), np.float32)}
        _check(self._L.p3d_adaptive_read_state(self._h, out["sum"].ctypes.data, out["sum_y2"].ctypes.data,
                                               out["samples"].ctypes.data, out["rel_err"].ctypes.data))
        return out

    def variance(self):
        """p3d_denoise_variance (waits for the device): per pixel the variance of its mean luminance, (h, w) float32 - the
        variance buffer of Denoiser.run; 0 where a pixel has fewer than 2 samples."""
        t = self.tile
        var = np.zeros((t.h, t.w), np.float32)
        _check(self._L.p3d_denoise_variance(self._h, var.ctypes.data))
        return var

    def variance_device(self, d_var, stream=0):
        """p3d_denoise_variance_device: the same into HBM (w*h float), enqueued on `stream` behind the pass."""
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_denoise_variance_device(self._h, C.c_void_p(d_var or None), C.c_void_p(raw or None)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.p3d_adaptive_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Denoiser:
    """p3d_denoiser (include/p3d.h): the edge-avoiding a-trous filter for w x h images on one device.  Inputs are the
    linear rgb of a frame, its feature buffers (DeviceScene.render_features) and optionally a variance buffer
    (AdaptiveAccumulator.variance); the device form neither allocates nor waits."""

    def __init__(self, device, w, h):
        self._L = lib()
        self.w, self.h = int(w), int(h)
        hd = C.c_void_p()
        _check(self._L.p3d_denoiser_create(int(device), self.w, self.h, C.byref(hd)))
        self._h = hd

    def _shape(self, a, shape, dtype, what):
        a = np.ascontiguousarray(a, dtype)
        if a.shape != shape:
            raise ValueError("%s: shape %s, the denoiser is for %s" % (what, a.shape, shape))
        return a

    def run(self, rgb, normal_depth, albedo_cov, variance=None, params=None, want_rgb8=False):
        """p3d_denoise: -> rgb (h, w, 3) float32, and with want_rgb8 (rgb, rgb8)."""
        h, w = self.h, self.w
        rgb = self._shape(rgb, (h, w, 3), np.float32, "rgb")
        nd = self._shape(normal_depth, (h, w, 4), np.float32, "normal_depth")
        ac = self._shape(albedo_cov, (h, w, 4), np.float32, "albedo_cov")
        var = None if variance is None else self._shape(variance, (h, w), np.float32, "variance")
        prm = params if params is not None else denoise_params()
        out = np.zeros((h, w, 3), np.float32)
        out8 = np.zeros((h, w, 3), np.uint8) if want_rgb8 else None
        _check(self._L.p3d_denoise(self._h, C.byref(prm), rgb.ctypes.data, var.ctypes.data if var is not None else None,
                                   nd.ctypes.data, ac.ctypes.data, out.ctypes.data, out8.ctypes.data if want_rgb8 else None))
        return (out, out8) if want_rgb8 else out

    def run_device(self, d_rgb, d_normal_depth, d_albedo_cov, d_out_rgb=0, d_out_rgb8=0, d_var=0, params=None, stream=0):
        """p3d_denoise_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); enqueued, not waited for."""
        prm = params if params is not None else denoise_params()
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_denoise_device(self._h, C.byref(prm), C.c_void_p(d_rgb or None), C.c_void_p(d_var or None),
                                          C.c_void_p(d_normal_depth or None), C.c_void_p(d_albedo_cov or None),
                                          C.c_void_p(d_out_rgb or None), C.c_void_p(d_out_rgb8 or None), C.c_void_p(raw or None)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.p3d_denoiser_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Temporal:
    """p3d_temporal (include/p3d.h): temporal accumulation of w x h frames on one device - every frame's colour blended with
    the previous frames' history reprojected into its view, plus a luminance variance for Denoiser.run.  Inputs per frame:
    the Camera the frame was rendered with (DeviceScene.camera), its linear rgb and its feature buffers
    (DeviceScene.render_features).  The device form neither allocates nor waits."""

    def __init__(self, device, w, h):
        self._L = lib()
        self.w, self.h = int(w), int(h)
        hd = C.c_void_p()
        _check(self._L.p3d_temporal_create(int(device), self.w, self.h, C.byref(hd)))
        self._h = hd

    @property
    def frames(self):
        """Frames accumulated since create / reset."""
        return int(self._L.p3d_temporal_frames(self._h))

    def reset(self):
        """Forget the history: the next frame starts it again."""
        _check(self._L.p3d_temporal_reset(self._h))

    def _shape(self, a, shape, what):
        a = np.ascontiguousarray(a, np.float32)
        if a.shape != shape:
            raise ValueError("%s: shape %s, the object is for %s" % (what, a.shape, shape))
        return a

    def run(self, camera, rgb, normal_depth, albedo_cov, params=None):
        """p3d_temporal_accumulate -> (rgb (h, w, 3), var (h, w), history (h, w)), float32."""
        h, w = self.h, self.w
        rgb = self._shape(rgb, (h, w, 3), "rgb")
        nd = self._shape(normal_depth, (h, w, 4), "normal_depth")
        ac = self._shape(albedo_cov, (h, w, 4), "albedo_cov")
        prm = params if params is not None else temporal_params()
        out = np.zeros((h, w, 3), np.float32)
        var = np.zeros((h, w), np.float32)
        hist = np.zeros((h, w), np.float32)
        _check(self._L.p3d_temporal_accumulate(self._h, C.byref(prm), C.byref(camera), rgb.ctypes.data, nd.ctypes.data,
                                               ac.ctypes.data, out.ctypes.data, var.ctypes.data, hist.ctypes.data))
        return out, var, hist

    def run_device(self, camera, d_rgb, d_normal_depth, d_albedo_cov, d_out_rgb, d_out_var=0, d_out_history=0, params=None,
                   stream=0):
        """p3d_temporal_accumulate_device: raw HBM addresses and a hipStream_t (or a torch.cuda.Stream); enqueued, not waited
        for."""
        prm = params if params is not None else temporal_params()
        raw = getattr(stream, "cuda_stream", stream)
        _check(self._L.p3d_temporal_accumulate_device(self._h, C.byref(prm), C.byref(camera), C.c_void_p(d_rgb or None),
                                                      C.c_void_p(d_normal_depth or None), C.c_void_p(d_albedo_cov or None),
                                                      C.c_void_p(d_out_rgb or None), C.c_void_p(d_out_var or None),
                                                      C.c_void_p(d_out_history or None), C.c_void_p(raw or None)))

    def close(self):
        if getattr(self, "_h", None):
            self._L.p3d_temporal_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stripe_tile(res, rank, world, stripe_h=16):
    """Tile of rank `rank` in an N-rank job: every world-th stripe of stripe_h rows (DESIGN.md multi-GPU).
    Requires res_y % (stripe_h * world) == 0 so that every rank renders the same number of rows."""
    rx, ry = res
    if ry % (stripe_h * world) != 0:
        raise ValueError("res_y=%d must be a multiple of stripe_h*world=%d" % (ry, stripe_h * world))
    return Tile(0, rank * stripe_h, rx, ry // world, stripe_h, world)


def stripe_rows(res, rank, world, stripe_h=16):
    """Image rows (bottom-up numbering) that `stripe_tile` renders, in local-row order."""
    t = stripe_tile(res, rank, world, stripe_h)
    r = np.arange(t.h)
    return t.y0 + (r // stripe_h) * stripe_h * world + (r % stripe_h)


# ---- multi-GPU helpers (one process per GPU; torch.distributed moves the bytes) ----
def packed_bytes(n_pixels):
    """Per-rank framebuffer layout used for the gather: [rgb float32 x3 | hit int32] = 16 B/pixel."""
    return n_pixels * 16


def assemble_frame(gathered, res, world, stripe_h, frame_rgb=None, frame_hit=None, batch=1):
    """De-interleave the per-rank stripe buffers (torch uint8 tensors, `batch` consecutive frames each
    laid out as packed_bytes) into full frames: stripe s of rank r holds frame rows
    (s*world + r)*stripe_h ... +stripe_h.  Returns (rgb, hit) of shape (ry, rx, 3) / (ry, rx), with a
    leading batch axis when batch > 1."""
    import torch
    rx, ry = res
    n_str = ry // (stripe_h * world)
    n_local = rx * (ry // world)
    dev = gathered[0].device
    if frame_rgb is None:
        frame_rgb = torch.empty((batch, ry, rx, 3), dtype=torch.float32, device=dev)
    if frame_hit is None:
        frame_hit = torch.empty((batch, ry, rx), dtype=torch.int32, device=dev)
    per_frame = [g.view(batch, n_local * 16) for g in gathered]
    parts = [g[:, : n_local * 12].contiguous().view(torch.float32).view(batch, n_str, stripe_h, rx, 3) for g in per_frame]
    frame_rgb.view(batch, n_str, world, stripe_h, rx, 3).copy_(torch.stack(parts, dim=2))
    hits = [g[:, n_local * 12:].contiguous().view(torch.int32).view(batch, n_str, stripe_h, rx) for g in per_frame]
    frame_hit.view(batch, n_str, world, stripe_h, rx).copy_(torch.stack(hits, dim=2))
    if batch == 1:
        return frame_rgb.view(ry, rx, 3), frame_hit.view(ry, rx)
    return frame_rgb, frame_hit


_GATHER_MODE = {"mode": "gather"}


def gather_frame(local_buf, res, rank, world, stripe_h, dst=0, gathered=None, async_op=False):
    """One collective for a frame (or a batch of frames, rendered back to back into one buffer): every
    rank's packed stripe buffer to rank `dst` (RCCL on GPUs, gloo in the CPU tests).  Returns (work handle or None, gather list or None).
    `gather` is the natural all-to-one; should a backend build not provide it, the first failure
    switches this process group to `all_gather` (same bytes into rank `dst`, the other ranks simply
    ignore what they receive) - every rank hits the same error at the same call, so they switch
    together."""
    import torch
    import torch.distributed as dist
    if _GATHER_MODE["mode"] == "gather":
        if rank == dst and gathered is None:
            gathered = [torch.empty_like(local_buf) for _ in range(world)]
        try:
            work = dist.gather(local_buf, gathered if rank == dst else None, dst=dst, async_op=async_op)
            return work, gathered
        except (RuntimeError, NotImplementedError):
            _GATHER_MODE["mode"] = "all_gather"
    if gathered is None:
        gathered = [torch.empty_like(local_buf) for _ in range(world)]
    work = dist.all_gather(gathered, local_buf, async_op=async_op)
    return work, gathered


def assemble_frame8(gathered, res, world, stripe_h, frame8=None, batch=1):
    """Same de-interleave for u8 frames (img_Data, 3 B/pixel): the payload bench.py gathers by default."""
    import torch
    rx, ry = res
    n_str = ry // (stripe_h * world)
    if frame8 is None:
        frame8 = torch.empty((batch, ry, rx, 3), dtype=torch.uint8, device=gathered[0].device)
    parts = [g.view(batch, n_str, stripe_h, rx, 3) for g in gathered]
    frame8.view(batch, n_str, world, stripe_h, rx, 3).copy_(torch.stack(parts, dim=2))
    return frame8.view(ry, rx, 3) if batch == 1 else frame8


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
