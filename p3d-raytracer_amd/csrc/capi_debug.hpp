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

#ifdef P3D_PT_PROFILE
int p3d_debug_set_pt_prof(void* device_ptr) {
  unsigned long long* p = static_cast<unsigned long long*>(device_ptr);
  return hipMemcpyToSymbol(HIP_SYMBOL(p3d::g_pt_prof), &p, sizeof(p)) == hipSuccess ? P3D_OK : P3D_ERR_NO_DEVICE;
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
