// p3d_capi.hip — device half of include/p3d.h and the one device translation unit of libp3d.so: it includes the kernels
// (through capi_common.hpp) and the host code of every object kind, one file per concern.  There is no CPU fallback
// anywhere in these files: every entry point needs a HIP device and fails with P3D_ERR_NO_DEVICE otherwise.
#include "capi_common.hpp"        // error macro, Scratch, p3d_scene, shared checks
#include "capi_scene_layout.hpp"  // descriptor validation, BVH relabelling, blob assembly (host only)
#include "capi_scene.hpp"         // scene create / destroy / skybox
#include "capi_frame_plan.hpp"    // FramePlan: the decisions of one render call (host only)
#include "capi_dispatch.hpp"      // the kernel of every launch step: LiteralStep, the choosers, enqueue (host only)
#include "capi_frame.hpp"         // tile schedules, the enqueue steps, p3d_render_tile*
#include "capi_grid.hpp"          // the device-built uniform grid: build, rebuild, export
#include "capi_update.hpp"        // camera and geometry updates, BVH export
#include "shading_update.hpp"     // set_shading (the kernel of the stream form), the rules of the derived facts
#include "capi_shading.hpp"       // the lights and materials of a live scene: set, read back
#include "capi_accum.hpp"         // p3d_accum
#include "capi_adaptive.hpp"      // p3d_adaptive
#include "capi_denoise.hpp"       // feature buffers, a-trous filter, variance
#include "capi_temporal.hpp"      // p3d_temporal
#include "ray_query.hpp"          // ray_query_kernel, bvh_segment_any (kernels of the batched ray queries)
#include "hit_list_query.hpp"     // trace_hits_kernel, bvh_segment_hits (the hits in order along a ray)
#include "radiance_query.hpp"     // radiance_query_kernel (the Whitted chain for rays in device memory), camera_rays_kernel
#include "path_query.hpp"         // path_query_kernel (the path tracer for rays in device memory), camera_sample_rays_kernel
#include "overlap_query.hpp"      // overlap_box_device_kernel, bvh_overlap_box (the objects that touch a box)
#include "capi_query.hpp"         // p3d_trace_*, p3d_object_*, p3d_skybox_color
#include "capi_proximity.hpp"     // p3d_nearest_*, p3d_sweep_sphere_*, p3d_nearest_segment_k_device, p3d_overlap_box_device
#include "capi_debug.hpp"         // test hooks, instrumented builds
