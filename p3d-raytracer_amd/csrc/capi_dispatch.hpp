// capi_dispatch.hpp — the one place that names a templated render kernel: each chooser turns a FramePlan's run-time flags into
// the kernel pointer of one launch step, and enqueue() launches it.  Host only; every chooser is a pure function.
#pragma once
#include "capi_frame_plan.hpp"

namespace {

// One pointer type per argument list
using FrameKernel = void (*)(const RenderParams);  // whitted_kernel, pt_kernel, wf_level_kernel, the three handoff_check_* kernels
using AdaptKernel = void (*)(const RenderParams, const PtAdaptParams);
using FeatureKernel = void (*)(const RenderParams, const FeatureParams);

// Run-time flags to template arguments, in the style of with_accel (capi_common.hpp): f is called with one
// std::bool_constant per flag, in the order given.  Every combination of f is instantiated: what a combination must not
// instantiate stands behind `if constexpr` in f.
template <class F>
auto with_flags(F&& f) { return f(); }
template <class F, class... Rest>
auto with_flags(F&& f, bool flag, Rest... rest) {
  auto bind = [&](auto B) { return with_flags([&](auto... more) { return f(B, more...); }, rest...); };
  return flag ? bind(std::true_type{}) : bind(std::false_type{});
}

// Launches `kernel`; a null kernel is a combination its chooser says the plan cannot make
template <class... Params, class... Args>
hipError_t enqueue(void (*kernel)(Params...), uint32_t blocks, uint32_t threads, size_t lds, hipStream_t st, const Args&... args) {
  if (!kernel) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), lds, st, args...);
  return hipGetLastError();
}

// The SPILL argument of a Whitted or check kernel: a scene traversed from L2 always has the spilling stack, a staged one
// when its worst-case stack does not fit LDS (FramePlan::lds_spill, which implies lds_scene)
constexpr bool spill_of(bool lds, bool lds_spill) { return !lds || lds_spill; }

// pt_kernel and the whitted_kernel variants of a frame that hands no stack from pixel to pixel (every accel).
// Four lanes per pixel (SUB = 4): the path tracer from 16 samples per pixel; Whitted only anti-aliased over a scene traversed
// from L2 (100k triangles 512x512 2x2 AA 11.17 -> 6.84 ms, but a staged scene pays for one LDS copy per 16 pixels instead
// of per 64: balls_medium 3x3 AA 3.48 -> 5.17 ms, balls_low 2x2 0.60 -> 0.65 ms) - plan_frame sets sub4 for nothing else.
inline FrameKernel frame_kernel(uint32_t accel, const FramePlan& plan, bool aa, bool stats) {
  return with_accel(accel, [&](auto A) {
    return with_flags([](auto PT, auto SUB4, auto LDS, auto LDS_SPILL, auto AA, auto STATS) -> FrameKernel {
      constexpr int ACCEL = decltype(A)::value;
      if constexpr (PT) return pt_kernel<ACCEL, LDS, STATS, SUB4 ? 4 : 1>;
      else if constexpr (!SUB4) return whitted_kernel<ACCEL, LDS, STATS, AA, spill_of(LDS, LDS_SPILL)>;
      else if constexpr (AA && !LDS) return whitted_kernel<ACCEL, false, STATS, true, true, 4>;
      else return nullptr;
    }, plan.pt, plan.sub4, plan.lds_scene, plan.lds_spill, aa, stats);
  });
}

// The launches of a P3D_STACK_LITERAL frame (BVH only), in frame order.  Lists A-D and the rounds: FrameLaunch::handoff_rounds.
enum class LiteralStep {
  Pass1,         // whitted_kernel LIT 1, every scene: the tiles on an empty stack; writes the leftover records, and over a scene traversed from L2 with compact records the units to check (Handoff::check_list)
  CheckTiles,    // handoff_check_kernel, scenes traversed from L2 with dense records: checks every unit over the tiles, writes list A
  CheckList,     // handoff_check_list_kernel, scenes traversed from L2 with compact records: checks the units pass 1 announced, writes list A
  RepairTiles,   // whitted_kernel LIT 3, LDS-staged scenes: check and repair over the tiles in one launch (round 0), writes list B
  RepairList,    // whitted_kernel LIT 2, every scene: renders the units of a list again; A -> B (round 0, scenes traversed from L2), C -> D -> C ... (one persistent workgroup)
  CheckEntries,  // handoff_check_entries_kernel, every scene: round 1, re-traces the first hits of list B's units, writes list C
};

// Which step which scene can get, from plan_frame's rules (capi_frame_plan.hpp) and FrameLaunch::setup_handoff:
//  - per_level needs !lds_scene, and repair_tiles = literal && lds_scene && !per_level: a literal frame over an LDS-staged
//    scene always has repair_tiles, one over a scene traversed from L2 never.
//  - Handoff::check_list is null for an LDS-staged scene and for dense records.
//  - render_frame runs bands(1) when there is no check list: RepairTiles with repair_tiles, CheckTiles without; and
//    handoff_rounds runs CheckList when there is one, and round 0 as RepairList only without repair_tiles.
// So over an LDS-staged scene the frame is Pass1, RepairTiles, CheckEntries, RepairList and never CheckTiles or CheckList;
// over a scene traversed from L2 it is Pass1 (or the per-level chain), CheckTiles or CheckList, RepairList, CheckEntries,
// RepairList and never RepairTiles.  Hence no whitted_kernel LIT 3 without LDS, and no handoff_check_kernel or
// handoff_check_list_kernel with LDS: those return null and are not instantiated.
// ghosts: the scene has zero-weight reflection rays to trace (a transmissive AND reflective material).
inline FrameKernel literal_kernel(LiteralStep step, bool lds_scene, bool lds_spill, bool ghosts, bool aa, bool stats) {
  return with_flags([step](auto LDS, auto LDS_SPILL, auto GHOSTS, auto AA, auto STATS) -> FrameKernel {
    constexpr int A = P3D_ACCEL_BVH;
    constexpr bool SPILL = spill_of(LDS, LDS_SPILL);
    switch (step) {
      case LiteralStep::Pass1: return whitted_kernel<A, LDS, STATS, AA, SPILL, 1, 1, GHOSTS>;
      case LiteralStep::RepairList: return whitted_kernel<A, LDS, STATS, AA, SPILL, 1, 2, GHOSTS>;
      case LiteralStep::CheckEntries: return handoff_check_entries_kernel<LDS, SPILL, STATS>;
      case LiteralStep::RepairTiles:
        if constexpr (LDS) return whitted_kernel<A, true, STATS, AA, SPILL, 1, 3, GHOSTS>;
        break;
      case LiteralStep::CheckTiles:
        if constexpr (!LDS) return handoff_check_kernel<false, true, STATS>;
        break;
      case LiteralStep::CheckList:
        if constexpr (!LDS) return handoff_check_list_kernel<false, true, STATS>;
        break;
    }
    return nullptr;
  }, lds_scene, lds_spill, ghosts, aa, stats);
}

// One chain level of the per-level launches (wavefront.hpp); literal: the level records feed the hit_stack hand-off
inline FrameKernel level_kernel(bool stats, bool literal) {
  return with_flags([](auto STATS, auto LIT) -> FrameKernel { return wf_level_kernel<STATS, LIT ? 1 : 0>; }, stats, literal);
}

// Adaptive passes (pt_adaptive_kernel): the grid is sized to the resident waves, not to the frame
inline AdaptKernel adaptive_kernel(uint32_t accel, const FramePlan& plan, bool stats) {
  return with_accel(accel, [&](auto A) {
    return with_flags([](auto SUB4, auto LDS, auto STATS) -> AdaptKernel {
      return pt_adaptive_kernel<decltype(A)::value, LDS, STATS, SUB4 ? 4 : 1>;
    }, plan.sub4, plan.lds_scene, stats);
  });
}

// Feature buffers (features.hpp): the frame's staging and stack; a scene that is not staged has the window (plan_frame)
inline FeatureKernel feature_kernel_of(uint32_t accel, const FramePlan& plan) {
  return with_accel(accel, [&](auto A) {
    return with_flags([](auto LDS, auto WINDOW, auto LDS8) -> FeatureKernel {
      if constexpr (!LDS) return feature_kernel<decltype(A)::value, false, kStackWindow>;
      else return feature_kernel<decltype(A)::value, true, WINDOW ? kStackWindow : (LDS8 ? kStackLds8 : kStackLds6)>;
    }, plan.lds_scene, plan.stack_mode == kStackWindow, plan.stack_mode == kStackLds8);
  });
}

}  // namespace
