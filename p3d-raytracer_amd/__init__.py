"""p3d-raytracer_amd — Python face of libp3d.so (the C-ABI of include/p3d.h).

Thin ctypes plumbing only: the product is the shared library (host C++ loader / BVH /
grid builders + gfx950 HIP kernels).  Nothing here computes pixels, and nothing here
touches oracle/: if libp3d.so is missing, or there is no HIP device, calls fail loudly.

The directory name has a hyphen, so import it through the root-level shim:

    import p3d_amd as p3d        # repo root on sys.path
    hs = p3d.HostScene("scene.p3f")
    dev = p3d.DeviceScene(hs, bvh=True)
    rgb, hit, stats = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4))

One module per concern (DESIGN.md "Python package: one module per concern"); this file only gathers their names, private
ones included, because the shim hands every one of them on as p3d_amd.<name>.
"""
from ._abi import (ACCEL_BVH, ACCEL_GRID, ACCEL_NONE, CHAIN_AUTO, CHAIN_MEGAKERNEL, CHAIN_PER_LEVEL, DEBUG_DEPTH_MAP, DEBUG_NONE,
                   DEBUG_TEST_INTERSECT, EXPORTS, EXPORTS_ADDED, HANDOFF_COMPACT, HANDOFF_DENSE, HERE, LIB_PATH, LOAD_LEGACY_F11, PATHTRACE,
                   PLAN_MODES, PROTOTYPES, SAMPLE_JITTER, SAMPLE_TENT, STACK_LDS6, STACK_LDS8, STACK_LITERAL, STACK_PER_PIXEL, STACK_WINDOW,
                   TILE_ORDER_COST, TILE_ORDER_FRAME, UPDATE_REBUILD, UPDATE_REFIT, WHITTED, AdaptiveParams, BvhCost, BvhNode, Camera,
                   Config, DebugPlan, DenoiseParams, FramePlan, GeomSource, GridDesc, Light, Material, OcclusionParams, P3DError, Prim, SceneDesc,
                   SkyboxDesc, SkyboxFace, Stats, TemporalParams, Tile, Xform, XformRange, _check, _Handle, _lib, _ptr, _stream, build,
                   device_count, lib)
from ._device_args import (NEAREST_K_MAX, OCCLUSION_ACCUMULATE, PATH_ACCUMULATE, PATH_MAX_DEPTH, RADIANCE_MAX_DEPTH, RADIANCE_SKYBOX, TRACE_HITS_K_MAX,
                           _CAMERA_RAYS_OUTPUTS, _CAMERA_SAMPLE_RAYS_OUTPUTS, _NEAREST_OUTPUTS, _OCCLUSION_OUTPUTS, _OCCLUSION_RAYS_OUTPUTS, _PATH_OUTPUTS, _RADIANCE_OUTPUTS, _SWEEP_OUTPUTS, _TRACE_OUTPUTS,
                           _device_blocks, _device_rows, _device_vector, _nearest_k_outputs, _trace_hits_outputs)
from .config import _f3, default_config, denoise_params, look_at, pathtrace_config, temporal_params, whitted_config
from .device_queries import (camera_rays_device, camera_sample_rays_device, occlusion_device, occlusion_rays, occlusion_rays_device,
                             trace_path_device, trace_radiance_device)
from .sweep import host_sweep_sphere, sweep_sphere_device
from .filtered import (FILTER_SKIP_MAX, host_nearest_k_filtered, host_sweep_sphere_filtered, nearest_k_filtered_device,
                       occlusion_filtered_device, sweep_sphere_filtered_device, trace_any_filtered_device, trace_hits_filtered_device)
from .segment_queries import _nearest_segment_k_outputs, host_nearest_segment_k, nearest_segment_k_device, segment_box_d2
from .overlap import OVERLAP_SOLID, _overlap_outputs, host_overlap_box, overlap_box_device
from .device_scene import SKYBOX_FACE_FILES, DeviceScene, load_skybox_dir
from .geometry import _xform_arrays, deformed, deformed_spheres, transformed, tree_cost
from .host_scene import HostScene
from .multigpu import _GATHER_MODE, assemble_frame, assemble_frame8, gather_frame, packed_bytes, stripe_rows, stripe_tile
from .passes import Accumulator, AdaptiveAccumulator, Denoiser, Temporal
from .shading import (LIGHT_FLOATS, MATERIAL_FLOATS, host_set_lights, host_set_materials, scene_lights, scene_materials, set_lights, set_materials,
                      set_shading_device)
