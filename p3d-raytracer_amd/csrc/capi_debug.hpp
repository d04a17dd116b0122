// capi_debug.hpp — the test hooks of p3d_debug.h and the entry points of the instrumented builds
#pragma once
#include "capi_common.hpp"

extern "C" {

// csrc/p3d_debug.h (not part of include/p3d.h): refused unless the process was started with P3D_TEST_HOOKS=1
int p3d_debug_scene_limits(p3d_scene* s, const p3d_debug_limits* limits) {
  static const bool enabled = [] { const char* e = getenv("P3D_TEST_HOOKS"); return e && e[0] == '1' && e[1] == 0; }();
  if (!enabled) return fail(P3D_ERR_UNSUPPORTED, "p3d_debug_scene_limits: test hooks are off (start the process with P3D_TEST_HOOKS=1)");
  if (!s) return fail(P3D_ERR_INVALID, "p3d_debug_scene_limits: null scene");
  s->dbg = limits ? *limits : p3d_debug_limits{0, 0, 0, 0};
  return P3D_OK;
}

// What a frame of `cfg` over `tile` copies into LDS: the float4s of the staged range, 0 when the scene is traversed from
// global memory (plan_frame's decision; read-only, no device call, no test-hook switch needed)
int p3d_debug_staged_f4(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, uint32_t* staged_f4) {
  if (!s || !cfg || !tile || !staged_f4) return fail(P3D_ERR_INVALID, "p3d_debug_staged_f4: null argument");
  if (int rc = check_frame(s, cfg, tile)) return rc;
  FramePlan plan{};
  const uint32_t samples = cfg->antialiasing ? cfg->spp_sqrt * cfg->spp_sqrt : 1u;
  if (int rc = plan_frame(scene_facts(s), cfg, tile, 0, samples, kFrame, 0, plan)) return rc;
  *staged_f4 = plan.lds_scene ? plan.stage_hi - plan.stage_lo : 0u;
  return P3D_OK;
}

// What the choosers of capi_dispatch.hpp read of the plan of one launch (read-only like p3d_debug_staged_f4)
int p3d_debug_frame_plan(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, uint32_t sample_begin, uint32_t sample_end, uint32_t mode,
                         p3d_debug_plan* out) {
  if (!s || !cfg || !tile || !out) return fail(P3D_ERR_INVALID, "p3d_debug_frame_plan: null argument");
  if (mode > P3D_DEBUG_PLAN_FEATURES) return fail(P3D_ERR_INVALID, "p3d_debug_frame_plan: unknown mode " + std::to_string(mode));
  if (int rc = check_frame(s, cfg, tile)) return rc;
  const uint32_t total = cfg->antialiasing ? cfg->spp_sqrt * cfg->spp_sqrt : 1u;
  if (sample_begin >= sample_end || sample_end > total)
    return fail(P3D_ERR_INVALID, "p3d_debug_frame_plan: samples [" + std::to_string(sample_begin) + ", " + std::to_string(sample_end) + ") of a frame of " + std::to_string(total));
  FramePlan plan{};
  const FrameMode fm = mode == P3D_DEBUG_PLAN_ADAPTIVE ? kAdaptivePass : (mode == P3D_DEBUG_PLAN_FEATURES ? kFeatures : kFrame);
  if (int rc = plan_frame(scene_facts(s), cfg, tile, sample_begin, sample_end, fm, 1, plan)) return rc;
  *out = p3d_debug_plan{plan.pt, plan.literal, plan.lds_scene, plan.lds_spill, plan.sub4, plan.per_level, plan.repair_tiles, (uint32_t)plan.stack_mode,
                        plan.spill_entries, plan.bound, plan.cap, s->zero_weight_reflections};
  return P3D_OK;
}
uint32_t p3d_debug_frame_plan_size(void) { return (uint32_t)sizeof(p3d_debug_plan); }

#ifdef P3D_PT_PROFILE
int p3d_debug_set_pt_prof(void* device_ptr) {
  unsigned long long* p = static_cast<unsigned long long*>(device_ptr);
  return hipMemcpyToSymbol(HIP_SYMBOL(p3d::g_pt_prof), &p, sizeof(p)) == hipSuccess ? P3D_OK : P3D_ERR_NO_DEVICE;
}
#endif
#ifdef P3D_ENTRY_CLOCK
int p3d_debug_set_entry_clock(void* device_ptr, uint32_t half) {
  unsigned long long* p = static_cast<unsigned long long*>(device_ptr);
  if (hipMemcpyToSymbol(HIP_SYMBOL(p3d::g_entry_clock), &p, sizeof(p)) != hipSuccess) return P3D_ERR_NO_DEVICE;
  return hipMemcpyToSymbol(HIP_SYMBOL(p3d::g_entry_half), &half, sizeof(half)) == hipSuccess ? P3D_OK : P3D_ERR_NO_DEVICE;
}
#endif
#ifdef P3D_TIMELINE
int p3d_debug_set_timeline(void* device_ptr) {
  unsigned long long* p = static_cast<unsigned long long*>(device_ptr);
  return hipMemcpyToSymbol(HIP_SYMBOL(p3d::g_timeline), &p, sizeof(p)) == hipSuccess ? P3D_OK : P3D_ERR_NO_DEVICE;
}
int p3d_debug_copy_sched(p3d_scene* s, uint32_t* host_sched, size_t n_sched, uint32_t* host_cost, size_t n_cost) {
  if (s->sched.empty()) return P3D_ERR_INVALID;
  (void)hipDeviceSynchronize();
  if (hipMemcpy(host_sched, s->sched[0].sched.p, n_sched * 4, hipMemcpyDeviceToHost) != hipSuccess) return P3D_ERR_NO_DEVICE;
  return hipMemcpy(host_cost, s->sched[0].cost.p, n_cost * 4, hipMemcpyDeviceToHost) == hipSuccess ? P3D_OK : P3D_ERR_NO_DEVICE;
}
#endif

}  // extern "C"
