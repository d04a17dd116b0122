"""The C-ABI of include/p3d.h as ctypes sees it: where the library is, the constants, the structures, the one table of
prototypes, build() / lib() / _check(), and what every wrapper of a C handle shares (_ptr, _stream, _Handle)."""
import collections
import ctypes as C
import os
import subprocess

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


class OcclusionParams(C.Structure):
    """p3d_occlusion_params (include/p3d_occlusion.h)"""
    _fields_ = [("seed", C.c_uint64), ("samples", C.c_uint32), ("sample_begin", C.c_uint32), ("point_offset", C.c_uint32),
                ("flags", C.c_uint32), ("bias", C.c_float), ("team", C.c_uint32)]


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

VP, U32, I32, F32, F3, PTR = C.c_void_p, C.c_uint32, C.c_int32, C.c_float, C.c_float * 3, C.POINTER
DEFAULT = "ctypes' own restype, a C int: lib() leaves it alone"

# The one table of C prototypes: name -> (restype or DEFAULT, argtypes or None = none are set, ctypes converts what it is
# given).  In the order of include/p3d.h's history; the test hooks of csrc/p3d_debug.h come last.  A new entry point is one
# line here.  Some tests call the raw library with None handles and plain ints: a stricter prototype changes what they see.
PROTOTYPES = {
    "p3d_abi_version": (U32, None),
    "p3d_last_error": (C.c_char_p, None),
    "p3d_device_count": (DEFAULT, None),
    "p3d_config_default": (DEFAULT, None),
    "p3d_scene_create": (DEFAULT, [PTR(SceneDesc), C.c_int, PTR(VP)]),
    "p3d_scene_create_device_bvh": (DEFAULT, None),
    "p3d_scene_destroy": (DEFAULT, [VP]),
    "p3d_scene_set_skybox": (DEFAULT, [VP, PTR(SkyboxDesc)]),
    "p3d_render_tile": (DEFAULT, [VP, PTR(Config), PTR(Tile)] + [VP] * 3 + [PTR(Stats)]),
    "p3d_render_tile_device": (DEFAULT, [VP, PTR(Config), PTR(Tile)] + [VP] * 4 + [PTR(Stats)]),
    "p3d_scene_status": (DEFAULT, [VP]),
    "p3d_scene_set_tail_stream": (DEFAULT, [VP, VP]),
    "p3d_scene_join": (DEFAULT, [VP, VP, C.c_int]),
    "p3d_object_intercepts": (DEFAULT, [VP, U32, U32] + [VP] * 4),
    "p3d_object_normal": (DEFAULT, [VP, U32, U32, VP, VP]),
    "p3d_skybox_color": (DEFAULT, [VP, U32, VP, VP]),
    "p3d_trace_closest": (DEFAULT, [VP, U32, U32] + [VP] * 5),
    "p3d_trace_any": (DEFAULT, [VP, U32, U32] + [VP] * 3),
    "p3d_host_scene_load": (DEFAULT, [C.c_char_p, U32, PTR(VP)]),
    "p3d_host_scene_destroy": (DEFAULT, [VP]),
    "p3d_host_scene_set_resolution": (DEFAULT, [VP, I32, I32]),
    "p3d_host_scene_set_lens": (DEFAULT, [VP, F32, F32]),
    "p3d_host_scene_replicate_lights": (DEFAULT, [VP, U32, F32]),
    "p3d_host_scene_desc": (DEFAULT, [VP, C.c_int, C.c_int, PTR(PTR(SceneDesc))]),
    "p3d_host_scene_bind_device": (DEFAULT, [VP, VP]),
    "p3d_host_scene_has_skybox": (DEFAULT, [VP]),
    "p3d_host_scene_load_skybox": (DEFAULT, [VP, C.c_char_p]),
    "p3d_host_scene_skybox_face": (DEFAULT, [VP, C.c_int, PTR(PTR(C.c_uint8)), PTR(U32), PTR(U32)]),
    "p3d_accum_create": (DEFAULT, [VP, PTR(Config), PTR(Tile), PTR(VP)]),
    "p3d_accum_destroy": (None, [VP]),
    "p3d_accum_reset": (DEFAULT, [VP]),
    "p3d_accum_samples_done": (U32, [VP]),
    "p3d_accum_render": (DEFAULT, [VP, U32] + [VP] * 3 + [PTR(Stats)]),
    "p3d_accum_render_device": (DEFAULT, [VP, U32] + [VP] * 4 + [PTR(Stats)]),
    "p3d_adaptive_create": (DEFAULT, [VP, PTR(Config), PTR(Tile), PTR(AdaptiveParams), PTR(VP)]),
    "p3d_adaptive_destroy": (None, [VP]),
    "p3d_adaptive_reset": (DEFAULT, [VP]),
    "p3d_adaptive_samples_done": (U32, [VP]),
    "p3d_adaptive_active_pixels": (DEFAULT, [VP, PTR(U32)]),
    "p3d_adaptive_render": (DEFAULT, [VP, U32] + [VP] * 4 + [PTR(Stats)]),
    "p3d_adaptive_render_device": (DEFAULT, [VP, U32] + [VP] * 5 + [PTR(Stats)]),
    "p3d_adaptive_read_state": (DEFAULT, [VP] * 5),
    "p3d_render_features": (DEFAULT, [VP, PTR(Config), PTR(Tile), U32, VP, VP]),
    "p3d_render_features_device": (DEFAULT, [VP, PTR(Config), PTR(Tile), U32, VP, VP, VP]),
    "p3d_denoise_params_default": (None, [PTR(DenoiseParams)]),
    "p3d_denoiser_create": (DEFAULT, [C.c_int, I32, I32, PTR(VP)]),
    "p3d_denoiser_destroy": (None, [VP]),
    "p3d_denoise": (DEFAULT, [VP, PTR(DenoiseParams)] + [VP] * 6),
    "p3d_denoise_device": (DEFAULT, [VP, PTR(DenoiseParams)] + [VP] * 7),
    "p3d_denoise_variance": (DEFAULT, [VP, VP]),
    "p3d_denoise_variance_device": (DEFAULT, [VP, VP, VP]),
    "p3d_camera_look_at": (DEFAULT, [F3, F3, F3, F32, I32, I32, F32, F32, PTR(Camera)]),
    "p3d_scene_set_camera": (DEFAULT, [VP, PTR(Camera)]),
    "p3d_scene_camera": (DEFAULT, [VP, PTR(Camera)]),
    "p3d_host_scene_view": (DEFAULT, [VP, F3, F3, F3, PTR(F32), PTR(F32), PTR(F32)]),
    "p3d_temporal_params_default": (None, [PTR(TemporalParams)]),
    "p3d_temporal_create": (DEFAULT, [C.c_int, I32, I32, PTR(VP)]),
    "p3d_temporal_destroy": (None, [VP]),
    "p3d_temporal_reset": (DEFAULT, [VP]),
    "p3d_temporal_frames": (U32, [VP]),
    "p3d_temporal_accumulate": (DEFAULT, [VP, PTR(TemporalParams), PTR(Camera)] + [VP] * 6),
    "p3d_temporal_accumulate_device": (DEFAULT, [VP, PTR(TemporalParams), PTR(Camera)] + [VP] * 7),
    "p3d_scene_update_prims": (DEFAULT, [VP, U32, VP, VP, U32, PTR(F32)]),
    "p3d_scene_export_bvh": (DEFAULT, [VP, VP, PTR(U32), VP, PTR(U32), PTR(U32)]),
    "p3d_host_scene_set_geometry": (DEFAULT, [VP, U32, VP, VP]),
    "p3d_scene_build_grid": (DEFAULT, [VP, PTR(F32)]),
    "p3d_scene_export_grid": (DEFAULT, [VP, PTR(GridDesc), VP, PTR(U32), VP, PTR(U32)]),
    "p3d_scene_transform_prims": (DEFAULT, [VP, U32, VP, U32, VP, U32, PTR(F32)]),
    "p3d_scene_bvh_cost": (DEFAULT, [VP, PTR(BvhCost)]),
    "p3d_scene_set_auto_rebuild": (DEFAULT, [VP, F32]),
    "p3d_scene_auto_rebuild": (DEFAULT, [VP, PTR(F32)]),
    "p3d_scene_update_geometry_device": (DEFAULT, [VP, U32, VP, U32, PTR(F32)]),
    "p3d_trace_closest_device": (DEFAULT, [VP, U32, U32] + [VP] * 8),
    "p3d_trace_any_device": (DEFAULT, [VP, U32, U32] + [VP] * 5),
    "p3d_scene_refit_device": (DEFAULT, [VP, U32, VP, VP]),
    "p3d_scene_set_rig": (DEFAULT, [VP, U32, VP, U32]),
    "p3d_scene_rig": (DEFAULT, [VP, PTR(U32), PTR(U32), PTR(U32)]),
    "p3d_scene_pose_device": (DEFAULT, [VP, U32, VP, VP, VP]),
    "p3d_host_scene_nearest": (DEFAULT, [VP, U32] + [VP] * 5),
    "p3d_nearest_device": (DEFAULT, [VP, U32, U32] + [VP] * 7),
    "p3d_host_scene_nearest_k": (DEFAULT, [VP, U32, U32] + [VP] * 6),
    "p3d_nearest_k_device": (DEFAULT, [VP, U32, U32, U32] + [VP] * 8),
    "p3d_trace_hits_device": (DEFAULT, [VP, U32, U32, U32] + [VP] * 10),
    "p3d_trace_radiance_device": (DEFAULT, [VP, U32, U32, VP, VP, I32, U32, VP, VP, VP]),
    "p3d_camera_rays_device": (DEFAULT, [VP, PTR(Camera), PTR(Tile), VP, VP, VP]),
    "p3d_trace_path_device": (DEFAULT, [VP, U32, U32, VP, VP, I32, U32, U32, C.c_uint64, VP, U32, VP, VP, VP]),
    "p3d_camera_sample_rays_device": (DEFAULT, [VP, PTR(Camera), PTR(Tile), PTR(Config), U32, VP, VP, VP, VP]),
    "p3d_occlusion_device": (DEFAULT, [VP, U32, U32, VP, VP, VP, PTR(OcclusionParams), VP, VP, VP]),
    "p3d_occlusion_rays_device": (DEFAULT, [VP, U32, VP, VP, PTR(OcclusionParams), VP, VP, VP]),
    "p3d_occlusion_rays": (DEFAULT, [U32, VP, VP, PTR(OcclusionParams), VP, VP]),
    "p3d_scene_set_materials": (DEFAULT, [VP, U32, U32, VP]),
    "p3d_scene_set_lights": (DEFAULT, [VP, U32, U32, VP]),
    "p3d_scene_materials": (DEFAULT, [VP, U32, U32, VP]),
    "p3d_scene_lights": (DEFAULT, [VP, U32, U32, VP]),
    "p3d_scene_set_shading_device": (DEFAULT, [VP, U32, U32, VP, U32, U32, VP, VP]),
    "p3d_host_scene_set_materials": (DEFAULT, [VP, U32, U32, VP]),
    "p3d_host_scene_set_lights": (DEFAULT, [VP, U32, U32, VP]),
    "p3d_sweep_sphere_device": (DEFAULT, [VP, U32, U32] + [VP] * 10),
    "p3d_host_scene_sweep_sphere": (DEFAULT, [VP, U32] + [VP] * 8),
    "p3d_nearest_k_filtered_device": (DEFAULT, [VP, U32, U32, U32, VP, VP, VP, U32, VP] + [VP] * 6),
    "p3d_sweep_sphere_filtered_device": (DEFAULT, [VP, U32, U32, VP, VP, VP, VP, VP, U32, VP] + [VP] * 6),
    "p3d_host_scene_nearest_k_filtered": (DEFAULT, [VP, U32, U32, VP, VP, VP, U32, VP] + [VP] * 4),
    "p3d_host_scene_sweep_sphere_filtered": (DEFAULT, [VP, U32, VP, VP, VP, VP, VP, U32, VP] + [VP] * 4),
    "p3d_trace_any_filtered_device": (DEFAULT, [VP, U32, U32, VP, VP, VP, VP, U32, VP, VP, VP]),
    "p3d_trace_hits_filtered_device": (DEFAULT, [VP, U32, U32, U32, VP, VP, VP, VP, U32, VP] + [VP] * 7),
    "p3d_occlusion_filtered_device": (DEFAULT, [VP, U32, U32, VP, VP, VP, PTR(OcclusionParams), VP, U32, VP, VP, VP, VP]),
    "p3d_nearest_segment_k_device": (DEFAULT, [VP, U32, U32, U32, VP, VP, VP, VP, U32, VP] + [VP] * 8),
    "p3d_host_scene_nearest_segment_k": (DEFAULT, [VP, U32, U32, VP, VP, VP, VP, U32, VP] + [VP] * 6),
    "p3d_overlap_box_device": (DEFAULT, [VP, U32, U32, U32, VP, VP, VP, U32, VP, U32, VP, VP, VP]),
    "p3d_host_scene_overlap_box": (DEFAULT, [VP, U32, U32, VP, VP, VP, U32, VP, U32, VP, VP]),
    "p3d_debug_segment_box_d2": (DEFAULT, [U32] + [VP] * 5),
    "p3d_debug_scene_limits": (DEFAULT, [VP, VP]),
    "p3d_debug_frame_plan": (DEFAULT, [VP, PTR(Config), PTR(Tile), U32, U32, U32, PTR(DebugPlan)]),
    "p3d_debug_frame_plan_size": (U32, None),
    "p3d_debug_staged_f4": (DEFAULT, [VP, VP, VP, PTR(U32)]),
}
# EXPORTS: what include/p3d.h itself declares, the entry points of the recorded surface (tests/python_api_surface.json holds the
# list to what it was).  EXPORTS_ADDED: those declared since, in include/p3d_radiance.h, p3d_occlusion.h and p3d_shading.h, which
# p3d.h includes, and in p3d_sweep.h, p3d_filter.h, p3d_segment.h and p3d_overlap.h likewise; detected by their symbols
EXPORTS_ADDED = ["p3d_trace_radiance_device", "p3d_camera_rays_device", "p3d_trace_path_device", "p3d_camera_sample_rays_device",
                 "p3d_occlusion_device", "p3d_occlusion_rays_device", "p3d_occlusion_rays",
                 "p3d_scene_set_materials", "p3d_scene_set_lights", "p3d_scene_materials", "p3d_scene_lights",
                 "p3d_scene_set_shading_device", "p3d_host_scene_set_materials", "p3d_host_scene_set_lights",
                 "p3d_sweep_sphere_device", "p3d_host_scene_sweep_sphere",
                 "p3d_nearest_k_filtered_device", "p3d_sweep_sphere_filtered_device", "p3d_host_scene_nearest_k_filtered",
                 "p3d_host_scene_sweep_sphere_filtered",
                 "p3d_trace_any_filtered_device", "p3d_trace_hits_filtered_device", "p3d_occlusion_filtered_device",
                 "p3d_nearest_segment_k_device", "p3d_host_scene_nearest_segment_k",
                 "p3d_overlap_box_device", "p3d_host_scene_overlap_box"]
EXPORTS = [name for name in PROTOTYPES if not name.startswith("p3d_debug_") and name not in EXPORTS_ADDED]


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
        for name, (restype, argtypes) in PROTOTYPES.items():
            f = getattr(L, name)
            if restype is not DEFAULT:
                f.restype = restype
            if argtypes is not None:
                f.argtypes = argtypes
        _lib = L
    return _lib


def _check(rc):
    if rc != 0:
        raise P3DError(rc, lib().p3d_last_error().decode("utf-8", "replace"))


def _ptr(address):
    """An address (of device or host memory; 0 or None: null) as the c_void_p argument of a call"""
    return C.c_void_p(address or None)


def _stream(stream):
    """`stream` (a torch.cuda.Stream, a raw hipStream_t, 0 or None: the default stream, or "off" where a call says so) as
    the c_void_p argument of a call"""
    return C.c_void_p(getattr(stream, "cuda_stream", stream) or None)


class _Handle:
    """What the classes that own a C handle share: `_L`, the library; `_h`, the handle, None once closed; `_destroy`, the
    name of the entry point that frees it."""
    _destroy = None

    def close(self):
        h = getattr(self, "_h", None)  # (a constructor that raised has not set it)
        if h:
            self._h = None
            getattr(self._L, self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    n = lib().p3d_device_count()
    return max(n, 0)

