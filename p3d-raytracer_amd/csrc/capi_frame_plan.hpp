// capi_frame_plan.hpp — FramePlan: the staging, stack, LDS, tile and launch-size decisions of one render call, made by plan_frame()
// without any call of the HIP runtime; capi_frame.hpp enqueues what the plan says
#pragma once
#include "capi_common.hpp"

namespace {

#ifndef P3D_PT_SUB4_MIN_SPP_SQRT
#define P3D_PT_SUB4_MIN_SPP_SQRT 4
#endif
#ifndef P3D_WHITTED_SUB4_MIN_SPP_SQRT
#define P3D_WHITTED_SUB4_MIN_SPP_SQRT 2
#endif
constexpr uint32_t kWhittedSub4MinSppSqrt = P3D_WHITTED_SUB4_MIN_SPP_SQRT;
constexpr uint32_t kPtSub4MinSppSqrt = P3D_PT_SUB4_MIN_SPP_SQRT;  // from 16 samples per pixel: 4 lanes per pixel
constexpr uint32_t kLdsSceneLimitBytesPt = 16 * 1024;  // same for the path tracer (not re-tuned: its packaged scenes are 1-2 KB)
constexpr uint32_t kLdsSceneLimitBytes = 26 * 1024;  // stage the scene in LDS up to this size
static_assert(kLdsSceneLimitBytes / 32 < 4096 && kLdsSceneLimitBytesPt / 32 < 4096, "the 6-byte stack entries of LDS-staged scenes keep 12 index bits (device_core.hpp Stack)");
// A frame is rendered by as few launches as the per-thread scratch (level records + stack spill)
// allows: every launch ends with a tail of partly idle CUs (2048x2048, 100k triangles: 30.3 ms in
// two launches, 28.1 ms in one).
constexpr size_t kLaunchScratchBudget = (size_t)4 << 30;
constexpr uint32_t kMaxLaunchThreads = 1u << 24;

// Tile of a wave of the one-lane-per-pixel Whitted kernels over a scene traversed from L2 (see plan_frame).
// P3D_TILE_SHAPE = 88 | 84 | 44 in the environment overrides the rule (experiments).
void tile_shape(uint64_t pixels, uint32_t& w, uint32_t& h) {
  static const int forced = env_int("P3D_TILE_SHAPE", 0);
  int shape = forced;
  if (shape != 88 && shape != 84 && shape != 44) shape = 88;
  w = shape == 44 ? 4 : 8;
  h = shape == 88 ? 8 : 4;
  (void)pixels;
}

// What a plan needs to know of a scene
struct SceneFacts {
  uint32_t off_nodes, off_ogeom, blob_f4;  // the float4 blob (capi_scene_layout.hpp)
  uint32_t bvh_max_depth, n_lights;
  bool zero_weight_reflections;
};
inline SceneFacts scene_facts(const p3d_scene* s) {
  return SceneFacts{s->off_nodes, s->off_ogeom, s->blob_f4, s->bvh_max_depth, s->dev.n_lights, s->zero_weight_reflections};
}

// worst-case node-stack height: each shadow feeler that returns `true` may leave up to
// depth-1 entries behind (Q2) and the next closest-hit query adds depth-1 more
uint32_t stack_bound(const SceneFacts& s, uint32_t accel, bool whitted) {
  if (accel != P3D_ACCEL_BVH) return 1;
  const uint32_t per = s.bvh_max_depth > 1 ? s.bvh_max_depth - 1 : 1;
  return whitted ? (s.n_lights + 1) * per : per;
}

// kFrame: p3d_render_tile_device and p3d_accum_render_device (samples [sample_begin, sample_end) of an anti-aliased frame).
// kAdaptivePass: p3d_adaptive_render_device (path tracer only), one launch over a pixel list sized to the resident waves.
// kFeatures: p3d_render_features_device, the primary rays of samples [0, sample_end) on an empty stack in one launch: the
// same scene staging, stack and LDS as the frame, no hit_stack hand-off, no per-level chain, nothing counted.
enum FrameMode { kFrame, kAdaptivePass, kFeatures };

struct FramePlan {
  FrameMode mode;
  bool pt, literal;            // path tracer; hit_stack handed from pixel to pixel (P3D_STACK_LITERAL where it applies)
  uint32_t bound;              // stack_bound()
  uint32_t stage_lo, stage_hi; // blob[stage_lo, stage_hi) is what an LDS-staged launch copies
  bool lds_scene, lds_spill;   // scene staged in LDS; ... with the spilling stack
  uint32_t window, cap, spill_entries;
  int stack_mode;              // kStackWindow / kStackLds8 / kStackLds6
  bool sub4, cold_lds;         // four lanes per pixel; cold shading state behind the stack in LDS
  uint32_t tpw, tph;           // pixels per wave tile
  size_t lds_bytes;
  uint32_t levels, deferred;   // per-thread float4 records in global scratch
  bool per_level;              // one launch per chain level (wavefront.hpp)
  int sh, ss;                  // stripe height and stride in rows (1, 1 without stripes)
  uint32_t tiles_x, total_bands, bands_per_launch, xcd_chunk;
  uint32_t halo_blocks_max, adapt_blocks, feat_blocks, max_threads;
  size_t levels_bytes, spill_bytes, deferred_bytes;  // the scene's scratch this call needs
  bool sched_ok, repair_tiles;

  uint32_t blocks_for(uint32_t ntiles) const {  // grid covering ntiles under the chunked XCD map
    const uint32_t groups = (ntiles + 8 * xcd_chunk - 1) / (8 * xcd_chunk);
    return groups * 8 * xcd_chunk;
  }
};

// resident: workgroups the device holds at once (kAdaptivePass only)
int plan_frame(const SceneFacts& s, const p3d_config* cfg, const p3d_tile* tile, uint32_t sample_begin, uint32_t sample_end, FrameMode mode,
               uint32_t resident, FramePlan& plan) {
  const bool feat = mode == kFeatures, adapt = mode == kAdaptivePass;
  const uint32_t chain_launch = feat ? (uint32_t)P3D_CHAIN_AUTO : cfg->chain_launch;
  const int sh = tile->stripe_h > 0 ? tile->stripe_h : 1, ss = tile->stripe_h > 0 ? tile->stripe_stride : 1;
  // main.cpp:804-812: without ANTIALIASING the frame loop always calls rayTracing
  const bool pt = cfg->integrator == P3D_PATHTRACE && cfg->antialiasing;
  // Only rayTracing over the BVH has a stack that survives a query (bvh.cpp:86,322); Radiance asks closest-hit
  // queries only, which leave it empty (bvh.cpp:256-274), the grid and the object loop have none.
  const bool literal = !feat && cfg->stack_mode == P3D_STACK_LITERAL && !pt && cfg->accel == P3D_ACCEL_BVH;
  // worst-case node-stack height (stack_bound).  LDS-staged scenes keep the WHOLE stack in LDS
  // (kernel variant without a spill path); deep trees / many lights use the global-memory variant,
  // which holds the first `cap` entries in LDS and spills the rest.
  const uint32_t bound = stack_bound(s, cfg->accel, !pt);
  // A scene of up to 26 KB is staged in LDS (beyond that the waves a CU can hold get too few: 37 KB staged
  // 1.22 ms, from L2 0.76 ms).  If scene + worst-case stack fit 20 KB and the stack has at most 24 entries, the
  // whole stack lives in LDS too (kernel without a spill path); otherwise (Whitted, several lights, deeper tree)
  // the staged scene is combined with the spilling stack: balls_medium 0.48 -> 0.40 ms, balls_box 0.42 -> 0.32 ms,
  // 96 / 128 random objects 0.49 -> 0.42 / 0.75 -> 0.66 ms against traversing those 14-25 KB from L2.
  // (staged: blob[off_nodes, stage_hi) - not the alignment pad in front of the nodes, and not the object-order geometry when
  // the kernel walks the BVH and is not the path tracer, which looks its emitters up by object)
  const uint32_t stage_lo = s.off_nodes, stage_hi = (cfg->accel == P3D_ACCEL_BVH && !pt) ? s.off_ogeom : s.blob_f4;
  const size_t stage_bytes = (size_t)(stage_hi - stage_lo) * sizeof(float4);
  const bool lds_scene = stage_bytes <= (pt ? kLdsSceneLimitBytesPt : kLdsSceneLimitBytes) && (bound <= 24 || !pt);
  const bool lds_spill = lds_scene && !pt && (bound > 24 || stage_bytes + (size_t)stack_lds_f4(false, bound) * sizeof(float4) > 20 * 1024);
  // Spilling stack (scenes traversed from L2; LDS-staged scenes whose worst case does not fit): LDS holds a window of the
  // most recent `window` entries (a power of two, device_core.hpp "Stack"), older entries sink into a per-thread column of
  // a global backing array.  8 entries = 4 KB per wave; the Whitted kernels that trade registers for waves keep 2.3 KB of
  // cold shading state behind it (cold_lds below): 6.4 KB per wave = 25 waves per CU by LDS, one more than the 24 (6 per
  // SIMD) those kernels' registers allow.
  uint32_t window = 8;
  if (const char* e = getenv("P3D_LDS_STACK_ENTRIES")) {  // experiments: LDS entries per lane (rounded up to a power of two)
    window = 1;
    while (window < (uint32_t)std::max(1, atoi(e)) && window < 1024) window *= 2;
  }
  const bool spilling = cfg->accel == P3D_ACCEL_BVH && !(lds_scene && !lds_spill);
  const uint32_t cap = cfg->accel == P3D_ACCEL_BVH ? (spilling ? window : bound) : 1;
  const uint32_t spill_entries = (spilling && bound > cap) ? bound : 0;  // rows of the backing array (entry e in row e)
  const uint32_t lds_scene_f4 = lds_scene ? stage_hi - stage_lo : 0;
  // path tracer with >= 16 samples per pixel in the launch: four lanes per pixel, 4x4-pixel tiles (pt_kernel SUB = 4)
  // ... and anti-aliased Whitted launches with >= 4 samples per pixel over a scene traversed from L2 (whitted_kernel SUB = 4),
  // unless the samples of a pixel have to hand the stack to each other in order (LITERAL).  Counted in the samples of THIS
  // launch (a pass of an accumulated frame may have fewer than the frame): both loops add the same values in the same order.
  const uint32_t launch_samples = sample_end - sample_begin;
  // (feature launches: one lane per pixel, 8x8 tiles)
  const bool sub4 = !feat && ((pt && launch_samples >= kPtSub4MinSppSqrt * kPtSub4MinSppSqrt) ||
                              (!pt && !literal && !lds_scene && cfg->antialiasing && launch_samples >= kWhittedSub4MinSppSqrt * kWhittedSub4MinSppSqrt));
  // ... and behind the node stack: the sample ring of the four-lanes-per-pixel kernels, or the cold shading state of the
  // Whitted kernels that traverse the scene from L2 without anti-aliasing (ColdState<true>, device_core.hpp)
  const bool cold_lds = !pt && !lds_scene && !cfg->antialiasing;
  // Pixels per wave.  Four lanes per pixel: 4x4.  One lane per pixel: 8x8, or - Whitted over a scene traversed from L2,
  // where a wave is as long as the slowest of its lanes in every query - 8x4 / 4x4 when the launch has too few 8x8 tiles
  // to keep the wave slots busy for several rounds (stripes of a multi-GPU frame, small frames): quarter waves are
  // shorter and four times as many, at the price of issue slots the chip then has to spare (tile_shape()).
  uint32_t tpw = sub4 ? 4 : 8, tph = sub4 ? 4 : 8;
  if (!feat && !sub4 && !pt && !lds_scene && !cfg->antialiasing && chain_launch != P3D_CHAIN_PER_LEVEL) tile_shape((uint64_t)tile->w * tile->h, tpw, tph);
  const uint32_t tp = tph;  // rows per tile band
  // (entry size: what the kernel's SPILL parameter says - the window for every kernel over a scene that is not staged and for
  // lds_spill; whole stack in LDS: eight-byte entries for the path tracer, six-byte ones for Whitted)
  const int stack_mode = (!lds_scene || lds_spill) ? kStackWindow : (pt ? kStackLds8 : kStackLds6);
  const size_t lds_bytes = (size_t)lds_scene_f4 * sizeof(float4) + (size_t)stack_lds_f4(stack_mode, cap) * sizeof(float4) +
                           (sub4 ? sizeof(PtPixelShared) : 0) + (cold_lds ? (size_t)kColdDwords * kBlock * sizeof(float) : 0);

  // rows per launch: whole 8-row tile bands, at most kMaxLaunchThreads threads
  const uint32_t tiles_x = ((uint32_t)tile->w + tpw - 1) / tpw;
  // per-thread global scratch: Whitted level records (+ the zero-weight reflection rays a LITERAL launch puts aside),
  // or the path tracer's two deferred dielectric branches
  const uint32_t levels = feat ? 0u : (pt ? 2 * 3 : (uint32_t)cfg->max_depth);
  const uint32_t deferred = (literal && s.zero_weight_reflections) ? 2u * (uint32_t)std::max(cfg->max_depth, 1) : 0u;
  // One launch per chain level (wf_level_kernel) where the lanes of a megakernel wave die off in the reflection levels:
  // Whitted without anti-aliasing over a BVH read from L2.  Not for the zero-weight reflection rays of LITERAL frames
  // (they make the chain a tree) and not for a grid or the object loop (no stack record to carry between launches).
  bool per_level = !pt && !cfg->antialiasing && cfg->accel == P3D_ACCEL_BVH && !lds_scene && cfg->max_depth >= 1 && cfg->max_depth <= 64 &&
                   !(literal && s.zero_weight_reflections) && chain_launch == P3D_CHAIN_PER_LEVEL;
  if (chain_launch == P3D_CHAIN_PER_LEVEL && !per_level)
    return fail(P3D_ERR_UNSUPPORTED, "chain_launch = PER_LEVEL needs Whitted without anti-aliasing over a BVH too big for LDS (and no transmissive + reflective material under P3D_STACK_LITERAL)");
  // per-level launches keep their level records per pixel, not per launch thread
  size_t scratch_per_thread = (size_t)((per_level ? 0 : levels) + deferred) * sizeof(float4) + (size_t)spill_entries * sizeof(uint2);
  const uint32_t launch_threads = (uint32_t)std::min<size_t>(per_level ? (1u << 23) : kMaxLaunchThreads, kLaunchScratchBudget / std::max<size_t>(scratch_per_thread, 1));
  uint32_t bands_per_launch = std::max<uint32_t>(1, launch_threads / (tiles_x * kBlock));
  const uint32_t total_bands = ((uint32_t)tile->h + tp - 1) / tp;
  if (tile->stripe_h > 0 && sh % (int)tp == 0 && bands_per_launch >= (uint32_t)sh / tp)
    bands_per_launch = (bands_per_launch / ((uint32_t)sh / tp)) * ((uint32_t)sh / tp);  // chunks start on a stripe boundary
  bands_per_launch = std::min(bands_per_launch, total_bands);
  if (per_level && bands_per_launch < total_bands) {  // the per-level path renders the tile in one go
    if (chain_launch == P3D_CHAIN_PER_LEVEL) return fail(P3D_ERR_CAPACITY, "chain_launch = PER_LEVEL: tile too large for one launch");
    per_level = false;
    scratch_per_thread += (size_t)levels * sizeof(float4);
    const uint32_t lt = (uint32_t)std::min<size_t>(kMaxLaunchThreads, kLaunchScratchBudget / std::max<size_t>(scratch_per_thread, 1));
    bands_per_launch = std::min(std::max<uint32_t>(1, lt / (tiles_x * kBlock)), total_bands);
    if (tile->stripe_h > 0 && sh % (int)tp == 0 && bands_per_launch >= (uint32_t)sh / tp)
      bands_per_launch = (bands_per_launch / ((uint32_t)sh / tp)) * ((uint32_t)sh / tp);
  }
  plan.mode = mode; plan.pt = pt; plan.literal = literal; plan.bound = bound; plan.stage_lo = stage_lo; plan.stage_hi = stage_hi;
  plan.lds_scene = lds_scene; plan.lds_spill = lds_spill; plan.window = window; plan.cap = cap; plan.spill_entries = spill_entries;
  plan.stack_mode = stack_mode; plan.sub4 = sub4; plan.cold_lds = cold_lds; plan.tpw = tpw; plan.tph = tph; plan.lds_bytes = lds_bytes;
  plan.levels = levels; plan.deferred = deferred; plan.per_level = per_level; plan.sh = sh; plan.ss = ss;
  plan.tiles_x = tiles_x; plan.total_bands = total_bands; plan.bands_per_launch = bands_per_launch;
  plan.xcd_chunk = lds_scene ? 1u : tiles_x;
  // Cost-ordered tiles (DESIGN.md "Tile schedule"): the frame order leaves a tail of a few long-running tiles.  Since
  // round 3 also for scenes traversed from L2 (100k triangles 2048x2048 18.25 -> 16.9 ms, 1024x1024 7.2 -> 6.5 ms; in
  // round 2, with child pairs straddling cache lines, the lost L2 locality cost more than the tail: 7.2 -> 7.5-7.9 ms).
  plan.sched_ok = cfg->tile_order == P3D_TILE_ORDER_COST && cfg->max_depth > 0;
  // LITERAL: workgroups behind the tile grid of the first launch render the halo chains (8 chains of 8 pixels per wave)
  const uint32_t halo_blocks_max = plan.halo_blocks_max = literal ? ((uint32_t)tile->h * kHaloChain + kBlock - 1) / kBlock : 0;
  // (an adaptive pass: one launch of at most `resident` workgroups, each working through groups of the pixel list)
  const uint32_t adapt_blocks = plan.adapt_blocks = adapt ? std::max<uint32_t>(1, std::min<uint32_t>(resident, (uint32_t)(((size_t)tile->w * tile->h + (sub4 ? 15 : 63)) / (sub4 ? 16 : 64)))) : 0;
  // (feature buffers: one launch over every tile of the tile, one lane per pixel)
  const uint32_t feat_blocks = plan.feat_blocks = feat ? plan.blocks_for(tiles_x * total_bands) : 0;
  if (feat && (uint64_t)feat_blocks * kBlock * std::max<uint32_t>(spill_entries, 1) > 0xffffffffull)  // (32-bit stack offsets, device_core.hpp Stack)
    return fail(P3D_ERR_CAPACITY, "p3d_render_features: tile too large for one launch over a tree this deep (split the tile)");
  const uint32_t max_threads = plan.max_threads = adapt ? adapt_blocks * kBlock : (feat ? feat_blocks * kBlock : (plan.blocks_for(tiles_x * bands_per_launch) + halo_blocks_max) * kBlock);
  const size_t tile_units = (size_t)tile->h * ((size_t)tile->w + kHaloChain);  // upper bound of Handoff::n_units
  // per-level launches keep one record per (level, unit); the work-list launches of a LITERAL frame behind them are the
  // megakernel and index [level][launch thread] with up to max_threads threads, whatever the size of the tile
  const size_t level_cols = per_level ? std::max<size_t>(tile_units, literal ? (size_t)max_threads : 0) : (size_t)max_threads;
  plan.levels_bytes = std::max<size_t>(16, (size_t)levels * level_cols * sizeof(float4));
  // (+ halo_find_kernel: one traversal per chain row on an empty stack, window of 8 entries, the rest of a tree path here)
  const size_t halo_backing = literal && s.bvh_max_depth > 8 ? (size_t)s.bvh_max_depth * tile->h * kBlock * sizeof(uint2) : 0;
  plan.spill_bytes = std::max<size_t>(16, std::max((size_t)spill_entries * max_threads * sizeof(uint2), halo_backing));
  plan.deferred_bytes = std::max<size_t>(16, (size_t)deferred * max_threads * sizeof(float4));
  // Round 0 of the hand-off over an LDS-staged scene: check AND repair over the tiles in one launch (whitted_kernel LIT = 3)
  // instead of a check launch that fills a list and a launch that renders the listed units again, 64 unrelated pixels per wave.
  plan.repair_tiles = literal && lds_scene && !per_level;
  return P3D_OK;
}

}  // namespace
