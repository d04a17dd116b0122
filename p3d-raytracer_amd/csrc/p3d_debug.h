/* p3d_debug.h — test hooks of libp3d.so.  NOT part of the drop-in boundary (include/p3d.h) and not installed with it:
 * nothing a maintainer of the reference would call.  The GPU tests use them to prove that the device-side error paths
 * fire (tests/test_gpu_parity.py).  The entry point is refused (P3D_ERR_UNSUPPORTED) unless the process was started
 * with P3D_TEST_HOOKS=1 in its environment, and what it sets belongs to ONE scene: no process-wide state. */
#ifndef P3D_DEBUG_H
#define P3D_DEBUG_H
#include "p3d.h"
#ifdef __cplusplus
extern "C" {
#endif
typedef struct p3d_debug_limits {
  uint32_t trip_bound;     /* trip bound of the four-lanes-per-pixel sample loops (0 = the real bound) */
  uint32_t max_rounds;     /* round bound of the hit_stack hand-off (0 = the real bound, min(units + 2, 4096)) */
  uint32_t halo_chain;     /* frame pixels the search in front of a row of a stripe / sub-rectangle may collect (0 = 16) */
  uint32_t leftover_pool;  /* entries of the pool of COMPACT hit_stack leftover records (0 = 8 per pixel, at least 65536) */
} p3d_debug_limits;
/* NULL limits = all real again. */
int p3d_debug_scene_limits(p3d_scene* scene, const p3d_debug_limits* limits);
/* Read-only, works without P3D_TEST_HOOKS: the float4s a frame of `cfg` over `tile` stages in LDS (0: the scene is not staged). */
int p3d_debug_staged_f4(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile, uint32_t* staged_f4);
/* What the kernel choosers (csrc/capi_dispatch.hpp) read of the plan of one launch: flags are 0 / 1 */
typedef struct p3d_debug_plan {
  uint32_t pt, literal;            /* path tracer; hit_stack handed from pixel to pixel */
  uint32_t lds_scene, lds_spill;   /* scene staged in LDS; ... with the spilling stack */
  uint32_t sub4, per_level;        /* four lanes per pixel; one launch per chain level */
  uint32_t repair_tiles;           /* round 0 of the hand-off checks and repairs over the tiles */
  uint32_t stack_mode;             /* 0 = whole stack in LDS, six-byte entries; 1 = LDS window + backing array; 2 = whole stack in LDS, eight-byte entries */
  uint32_t spill_entries;          /* rows of the backing array (0: nothing can sink out of the window) */
  uint32_t bound, cap;             /* worst-case stack height; entries held in LDS */
  uint32_t zero_weight_reflections;  /* the scene has a transmissive and reflective material (GHOSTS) */
} p3d_debug_plan;
#define P3D_DEBUG_PLAN_FRAME 0u    /* p3d_render_tile / p3d_accum_render: samples [sample_begin, sample_end) */
#define P3D_DEBUG_PLAN_ADAPTIVE 1u /* one pass of p3d_adaptive_render */
#define P3D_DEBUG_PLAN_FEATURES 2u /* p3d_render_features: samples [0, sample_end) */
/* Read-only, works without P3D_TEST_HOOKS, no device call: the plan of that launch.  Refusals are those of the frame check
 * (scene, config, tile) and of the plan itself; what the entry points refuse on their own - p3d_adaptive_create a Whitted
 * integrator or antialiasing = 0, p3d_render_features a striped tile - is not looked at: ask for the plan of a launch that exists. */
int p3d_debug_frame_plan(p3d_scene* scene, const p3d_config* cfg, const p3d_tile* tile, uint32_t sample_begin, uint32_t sample_end,
                         uint32_t mode, p3d_debug_plan* out);
uint32_t p3d_debug_frame_plan_size(void); /* sizeof(p3d_debug_plan) as the library was compiled */
#ifdef __cplusplus
}
#endif
#endif
