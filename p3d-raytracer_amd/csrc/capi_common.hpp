// capi_common.hpp — shared by the host files of the device translation unit: error macro, self-freeing device buffers, p3d_scene and its checks
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "../host/p3d_error.hpp"
#include "kernels.hpp"
#include "lbvh.hpp"
#include "grid_build.hpp"
#include "update_kernels.hpp"
#include "shading_update.hpp"
#include "p3d.h"
#include "p3d_debug.h"
#include "wavefront.hpp"
#include "queries.hpp"
#include "pt_kernel.hpp"
#include "adaptive.hpp"
#include "features.hpp"
#include "denoise.hpp"
#include "temporal.hpp"

using namespace p3d;

namespace {

#define P3D_HIP(call)                                                                        \
  do {                                                                                       \
    hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return fail(P3D_ERR_NO_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_));     \
  } while (0)

inline F3 to_f3(const float v[3]) { return F3{v[0], v[1], v[2]}; }

// A device buffer that grows on demand and is freed with its owner.  Move-only: the owner is deleted (or the vector that
// holds it shrinks) with its device current - every destroy entry point calls hipSetDevice first.
struct Scratch {
  void* p = nullptr;
  size_t bytes = 0;
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  Scratch(Scratch&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  Scratch& operator=(Scratch&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p; bytes = o.bytes;
      o.p = nullptr; o.bytes = 0;
    }
    return *this;
  }
  ~Scratch() { release(); }
  int ensure(size_t need) {
    if (need <= bytes) return P3D_OK;
    release();
    P3D_HIP(hipMalloc(&p, need));
    bytes = need;
    return P3D_OK;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// One memoised tile schedule.  The cost of a tile is a function of the scene (camera included),
// the chain depth, the back end, the sampling and the pixel rectangle: the first launch with a
// given key runs in frame order and records what every tile cost, the launches after it take
// the tiles most-expensive-class first.
struct SchedEntry {
  uint32_t accel = 0, aa = 0, spp = 0, pt = 0, tiles_x = 0, tiles_y = 0;  // (tiles: 8x8 or 4x4 pixels, by kernel variant)
  int32_t max_depth = 0, x0 = 0, y0 = 0, w = 0, h = 0, stripe_h = 0, stripe_stride = 0;
  Scratch cost, sched;
  hipEvent_t ready = nullptr;
  hipStream_t built_on = nullptr;
  uint64_t last_use = 0;
  bool built = false;  // the recording launch and sched_build_kernel were enqueued: `sched` may be used
  bool same_key(const SchedEntry& o) const {
    return accel == o.accel && aa == o.aa && spp == o.spp && pt == o.pt && tiles_x == o.tiles_x && tiles_y == o.tiles_y && max_depth == o.max_depth && x0 == o.x0 && y0 == o.y0 &&
           w == o.w && h == o.h && stripe_h == o.stripe_h && stripe_stride == o.stripe_stride;
  }
};

}  // namespace

struct p3d_scene {
  int device = 0;
  std::vector<SchedEntry> sched;
  uint64_t sched_clock = 0;
  float4* d_blob = nullptr;
  uint32_t blob_f4 = 0;
  uint32_t off_nodes = 0, off_bgeom = 0, off_ogeom = 0, off_normals = 0, off_mats = 0, off_lights = 0;
  uint32_t* d_cell_start = nullptr;
  uint32_t* d_cell_items = nullptr;
  uint32_t* d_emitters = nullptr;
  uint32_t emitters_cap = 0;             // words allocated there: p3d_scene_set_materials may grow the list
  uint32_t* d_sky[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool has_sky = false;
  DevScene dev{};
  bool has_bvh = false, has_grid = false;
  uint32_t bvh_max_depth = 0;
  float device_bvh_ms = 0;  // GPU time of lbvh::build, 0 for an uploaded tree
  Scratch levels, spill, deferred, wf_rays, wf_keys, wf_sorted, wf_final, out_rgb, out_hit, out_rgb8, q_in, q_out;
  // P3D_STACK_LITERAL (csrc/handoff.hpp): leftovers, per-unit records, work lists, counters
  Scratch ho_where, ho_entries, ho_meta, ho_first, ho_first_sample, ho_touched, ho_lists, ho_check, ho_counters, ho_row_chain, ho_halo_pix, ho_ucount;
  std::vector<int64_t> ho_chain_key;     // what the row_chain flags and halo pixels on the device were worked out for
  bool has_spheres = false;              // (halo_find_kernel: only a sphere test re-normalises a ray)
  bool has_planes = false;               // (p3d_nearest_device: the tree cannot find a plane, Q12; an update never changes a kind)
  int64_t first_box = -1;                // (p3d_sweep_sphere_device: a box is not swept) the first box among obj_tm, or -1
  uint32_t* d_halo_verdict = nullptr;    // kHoErrHalo if the memoised halo search could not start some row exactly
  float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};  // box of BVH node 0 (bins of the per-level ray queue)
  bool zero_weight_reflections = false;  // some material is transmissive AND reflective (main.cpp:282,290-300)
  unsigned long long* d_stats = nullptr;
  uint32_t* d_status = nullptr;          // kHoErr* bits raised by kernels; read and cleared by check_status()
  uint32_t last_status = 0;              // the bits check_status() found last (what the host-buffer call decides its DENSE retry on)
  p3d_debug_limits dbg{0, 0, 0, 0};      // tests only (csrc/p3d_debug.h): shrunken limits of THIS scene, all 0 = the real ones
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mid = nullptr, ev_p1 = nullptr;
  // p3d_scene_set_tail_stream: the dependent launches of a LITERAL frame go to a stream of their own
  hipStream_t tail_stream = nullptr;
  hipEvent_t ev_tail_go = nullptr, ev_tail_done = nullptr;
  bool tail_pending = false;  // ev_tail_done was recorded by the last frame: the next launch on this scene waits for it
  uint64_t cam_gen = 0;       // bumped by every p3d_scene_set_camera that changes the camera (p3d_accum / p3d_adaptive check it)
  // p3d_scene_update_prims (scenes of p3d_scene_create_device_bvh only)
  bool device_bvh = false;
  uint64_t geom_gen = 0;               // bumped by every update; checked like cam_gen
  std::vector<uint32_t> obj_tm;        // type | material << 8 of every object (of every scene): what an update may not change
  std::vector<float4> create_boxes;    // the object boxes the tree was built from, until the first update moves them to the device
  lbvh::Workspace lbvh_ws;             // allocated by the first update: object boxes and the topology of the tree in d_blob
  bool lbvh_topology = false;          // lbvh_ws.sorted / children / parent describe the tree in d_blob
  bool lbvh_fitted = false;            // ... and lbvh_ws.node_box holds its boxes: lbvh::enqueue_cost may run
  // p3d_scene_bvh_cost, p3d_scene_set_auto_rebuild (the same scenes)
  float auto_rebuild = 0.0f;           // 0: off; otherwise a REFIT whose tree costs more than this x sah_baseline rebuilds
  double sah_baseline = 0.0;           // 0: none recorded
  uint32_t refits_since_build = 0;
  bool last_update_rebuilt = false;
  // the geometry updates: p3d_scene_update_prims, p3d_scene_transform_prims, p3d_scene_update_geometry_device (the same scenes)
  Scratch stage;                       // the call in progress: a 16-byte counter block | the route's payload (capi_update.hpp)
  std::vector<uint4> stage_host;       // what is uploaded there
  Scratch rest;                        // object-order geometry of the rest pose, 3 float4 per object; made by the first transform
  // p3d_scene_refit_device (the same scenes)
  uint32_t* d_refit_skipped = nullptr; // {triangles with an index >= n_elems, objects with an unusable box} since the last check_status();
                                       // allocated by the first call, added to by its kernel together with upd::kStatusRefitSkipped in d_status
  bool root_stale = false;             // root_min / root_max are those of an older fit: refresh_root_box() before they are used
  // p3d_scene_set_rig, p3d_scene_pose_device (the same scenes)
  Scratch rig;                         // one uint32 per object: its transform slot or upd::kRigNotPosed; null: no rig
  uint32_t rig_ranges = 0, rig_xforms = 0, rig_posed = 0;  // what p3d_scene_rig answers
  Scratch pose_skipped;                // {objects with an unusable transform, objects with an unusable box} since the last check_status();
                                       // made by p3d_scene_set_rig, added to by upd::pose_rig together with upd::kStatusPoseSkipped in d_status
  // p3d_scene_set_shading_device (every scene)
  Scratch shading_skipped;             // {materials that would flip their emissive predicate, ... their transmissive-and-reflective one}
                                       // since the last check_status(); made by the first call, added to by shade::set_shading
                                       // together with shade::kStatusShadingSkipped in d_status
  // p3d_scene_build_grid (the same scenes): d_cell_start / d_cell_items above are then the device-built grid
  bool uploaded_grid = false;          // the descriptor carried the host's grid: it cannot follow updates and is never rebuilt
  uint64_t cell_start_cap = 0, cell_items_cap = 0;  // words allocated; they grow when a build needs more and are kept otherwise
  uint32_t grid_items = 0;             // cell_start[n_cells] of the device-built grid
  grid_build::Workspace grid_ws;       // allocated by the first build
};

namespace {

// Forgets the memoised tile schedules (their costs were recorded for one camera, among other things).
void drop_schedules(p3d_scene* s) {
  for (SchedEntry& e : s->sched)
    if (e.ready) (void)hipEventDestroy(e.ready);
  s->sched.clear();
}

// The same without freeing anything (a hipFree waits for the device): every schedule is recorded again by the next frame with
// its key, in the memory it holds (schedule_lookup)
void void_schedules(p3d_scene* s) {
  for (SchedEntry& e : s->sched) e.built = false;
}

// Puts `st` behind the previous frame's tail (p3d_scene_set_tail_stream), if one is still pending.  Enqueues a wait only
int wait_for_tail(p3d_scene* s, hipStream_t st) {
  if (s->tail_pending) {
    P3D_HIP(hipStreamWaitEvent(st, s->ev_tail_done, 0));
    s->tail_pending = false;
  }
  return P3D_OK;
}

// root_min / root_max from the node array, if a fit has been enqueued since they were read.  The caller has waited for the
// stream(s) that fit ran on
int refresh_root_box(p3d_scene* s) {
  if (!s->root_stale) return P3D_OK;
  float4 root[2];
  P3D_HIP(hipMemcpy(root, s->d_blob + s->off_nodes, sizeof(root), hipMemcpyDeviceToHost));
  s->root_min[0] = root[0].x; s->root_min[1] = root[0].y; s->root_min[2] = root[0].z;
  s->root_max[0] = root[1].x; s->root_max[1] = root[1].y; s->root_max[2] = root[1].z;
  s->root_stale = false;
  return P3D_OK;
}

// Every float field of a camera is finite, and the view window and plane distance are positive
bool camera_usable(const p3d_camera& c) {
  const float f[17] = {c.eye[0], c.eye[1], c.eye[2], c.u[0], c.u[1], c.u[2], c.v[0], c.v[1], c.v[2], c.n[0], c.n[1], c.n[2],
                       c.plane_dist, c.w, c.h, c.focal_ratio, c.aperture};
  for (float x : f)
    if (!std::isfinite(x)) return false;
  return c.w > 0.0f && c.h > 0.0f && c.plane_dist > 0.0f;
}

DevCamera dev_camera(const p3d_camera& c) {
  DevCamera d{};
  d.eye = to_f3(c.eye); d.u = to_f3(c.u); d.v = to_f3(c.v); d.n = to_f3(c.n);
  d.w = c.w; d.h = c.h; d.plane_dist = c.plane_dist; d.focal_ratio = c.focal_ratio; d.aperture = c.aperture;
  d.res_x = c.res_x; d.res_y = c.res_y;
  return d;
}

// An integer read from the environment: `def` when the variable is unset or its value lies outside [lo, hi].  Callers
// keep the result in a function-local static: one read per process.
inline int env_int(const char* name, int def, int lo = INT_MIN, int hi = INT_MAX) {
  const char* e = getenv(name);
  const int n = e ? atoi(e) : def;
  return n >= lo && n <= hi ? n : def;
}

int check_accel(const p3d_scene* s, uint32_t accel) {
  if (accel == P3D_ACCEL_BVH && !s->has_bvh) return fail(P3D_ERR_INVALID, "accel = Bvh but the scene was created without BVH arrays");
  if (accel == P3D_ACCEL_GRID && !s->has_grid) return fail(P3D_ERR_INVALID, "accel = UGrid but the scene was created without a grid");
  if (accel > P3D_ACCEL_BVH) return fail(P3D_ERR_INVALID, "unknown accel");
  return P3D_OK;
}

// The one place where a run-time p3d_config.accel picks the ACCEL template argument of a launch: f is called with a
// std::integral_constant of P3D_ACCEL_BVH, _GRID or _NONE.
template <class F>
auto with_accel(uint32_t accel, F&& f) {
  switch (accel) {
    case P3D_ACCEL_BVH: return f(std::integral_constant<int, P3D_ACCEL_BVH>{});
    case P3D_ACCEL_GRID: return f(std::integral_constant<int, P3D_ACCEL_GRID>{});
    default: return f(std::integral_constant<int, P3D_ACCEL_NONE>{});
  }
}

// Device-detected errors (sample hand-out loop hit its trip bound, a leftover outgrew its slot, the hand-off found no
// fixed point): read and clear the status word.  Call only where the stream has been synchronised.
// render_call: the check behind a render call with `stats` - the objects p3d_scene_refit_device or p3d_scene_pose_device
// skipped, and the materials p3d_scene_set_shading_device skipped, are not the frame's fault: their bits stay pending for
// p3d_scene_status.
int check_status(p3d_scene* s, bool render_call = false) {
  constexpr uint32_t kSkipped = upd::kStatusRefitSkipped | upd::kStatusPoseSkipped | shade::kStatusShadingSkipped;
  uint32_t h = 0;
  P3D_HIP(hipMemcpy(&h, s->d_status, sizeof(h), hipMemcpyDeviceToHost));
  if (render_call) {
    const uint32_t pending = h & kSkipped;
    h &= ~kSkipped;
    s->last_status = h;
    if (!h) return P3D_OK;
    P3D_HIP(hipMemcpy(s->d_status, &pending, sizeof(pending), hipMemcpyHostToDevice));
  } else {
    s->last_status = h;
    if (!h) return P3D_OK;
    P3D_HIP(hipMemset(s->d_status, 0, sizeof(uint32_t)));
  }
  static_assert((upd::kStatusRefitSkipped & (kHoErrLeftoverCap | kHoErrNoFixedPoint | kHoErrTrips | kHoErrList | kHoErrHalo)) == 0 &&
                    (upd::kStatusPoseSkipped & (upd::kStatusRefitSkipped | kHoErrLeftoverCap | kHoErrNoFixedPoint | kHoErrTrips | kHoErrList | kHoErrHalo)) == 0,
                "one word, distinct bits");
  static_assert((shade::kStatusShadingSkipped & (upd::kStatusPoseSkipped | upd::kStatusRefitSkipped | kHoErrLeftoverCap | kHoErrNoFixedPoint | kHoErrTrips | kHoErrList | kHoErrHalo)) == 0,
                "one word, distinct bits");
  std::string skipped;  // p3d_scene_refit_device, p3d_scene_pose_device: objects their kernels did not write
  if ((h & upd::kStatusRefitSkipped) && s->d_refit_skipped) {
    uint32_t bad[2] = {0, 0};
    P3D_HIP(hipMemcpy(bad, s->d_refit_skipped, sizeof(bad), hipMemcpyDeviceToHost));
    P3D_HIP(hipMemset(s->d_refit_skipped, 0, sizeof(bad)));
    skipped = " p3d_scene_refit_device: " + std::to_string(bad[0]) + " triangle(s) with an index >= n_elems, " + std::to_string(bad[1]) +
              " object(s) with a non-finite or inverted box: they keep their geometry; the others are updated;";
  }
  if ((h & upd::kStatusPoseSkipped) && s->pose_skipped.p) {
    uint32_t bad[2] = {0, 0};
    P3D_HIP(hipMemcpy(bad, s->pose_skipped.p, sizeof(bad), hipMemcpyDeviceToHost));
    P3D_HIP(hipMemset(s->pose_skipped.p, 0, sizeof(bad)));
    skipped += " p3d_scene_pose_device: " + std::to_string(bad[0]) +
               " object(s) with an unusable transform (a non-finite entry, a sphere_scale that is not finite and > 0, or a box under a matrix that is not positive-diagonal), " +
               std::to_string(bad[1]) + " object(s) with a non-finite or inverted box: they keep their geometry; the others are updated;";
  }
  if ((h & shade::kStatusShadingSkipped) && s->shading_skipped.p) {
    uint32_t bad[2] = {0, 0};
    P3D_HIP(hipMemcpy(bad, s->shading_skipped.p, sizeof(bad), hipMemcpyDeviceToHost));
    P3D_HIP(hipMemset(s->shading_skipped.p, 0, sizeof(bad)));
    skipped += " p3d_scene_set_shading_device: " + std::to_string(bad[0]) + " material(s) that would change whether they emit, " + std::to_string(bad[1]) +
               " material(s) that would change whether they are transmissive and reflective: they keep their records (p3d_scene_set_materials"
               " makes such a change); the others are updated;";
  }
  if (!skipped.empty() && !(h & ~kSkipped)) return fail(P3D_ERR_INVALID, "device-detected error:" + skipped);
  std::string what = skipped;
  if (h & kHoErrTrips) what += " sample hand-out loop reached its trip bound (pixels would miss samples);";
  if (h & kHoErrLeftoverCap) what += " the hit_stack leftovers of this frame do not fit their records (p3d_config.handoff_records = P3D_HANDOFF_DENSE has room for the worst case);";
  if (h & kHoErrNoFixedPoint) what += " hit_stack hand-off did not reach a fixed point;";
  if (h & kHoErrHalo) what += " a row of a stripe / sub-rectangle could not be started on the hit_stack the serial frame hands it (no pixel in front of it certifiably independent of its own incoming stack): render it with more rows in front, as part of the whole frame, or with P3D_STACK_PER_PIXEL;";
  if (h & kHoErrList) what += " a work list of the hit_stack hand-off or a ray queue segment of the per-level launches overflowed;";
  return fail(P3D_ERR_CAPACITY, "device-detected error:" + what);
}

}  // namespace
