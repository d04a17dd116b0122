// capi_update.hpp — a live scene changes: camera, geometry (p3d_scene_update_prims, p3d_scene_transform_prims,
// p3d_scene_update_geometry_device, and p3d_scene_refit_device and p3d_scene_set_rig / p3d_scene_pose_device on the caller's
// stream), and the export of a device-built tree
#pragma once
#include "capi_grid.hpp"

namespace {

// What every geometry update does before the scene changes: the waits, the builder's state, and for a refit the topology
int begin_update(p3d_scene* s, uint32_t mode, const char* who) {
  P3D_HIP(hipSetDevice(s->device));
  // enqueued frames read the geometry, the tree and the scene's memos: the tail stream, then the whole device
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  if (int rc = ensure_box_workspace(s, who)) return rc;  // first update: the builder's state
  lbvh::Workspace& w = s->lbvh_ws;
  if (mode == P3D_UPDATE_REFIT && !s->lbvh_topology) {
    // the keys, children and parents of the tree in d_blob, from the boxes it was built from: the build's own first half
    // (deterministic: unique keys), outside the timed part - a scene pays it once
    if (hipError_t e = lbvh::enqueue_topology(w, w.boxes); e != hipSuccess)
      return fail(P3D_ERR_NO_DEVICE, std::string(who) + ": topology: " + hipGetErrorString(e));
    P3D_HIP(hipDeviceSynchronize());
    s->lbvh_topology = true;
  }
  return P3D_OK;
}

// sah of include/p3d.h from what the cost kernels left
double sah_of(const lbvh::CostResult& c) { return c.root_area > 0.0 ? c.sum / c.root_area : 0.0; }

// The cost of the tree lbvh_ws describes, behind whatever is enqueued on the null stream; waits for it
hipError_t read_cost(lbvh::Workspace& w, lbvh::CostResult* out) {
  if (hipError_t e = lbvh::enqueue_cost(w); e != hipSuccess) return e;
  return hipMemcpy(out, w.cost_result, sizeof(*out), hipMemcpyDeviceToHost);
}

// The builder's state describes the tree in d_blob, boxes included.  A scene that was never updated recovers the topology and
// runs the fit over the boxes the tree was built from: the node array is rewritten with the same bits.  The device is idle.
int ensure_fitted_workspace(p3d_scene* s, const char* who) {
  if (int rc = ensure_box_workspace(s, who)) return rc;
  lbvh::Workspace& w = s->lbvh_ws;
  if (s->lbvh_topology && s->lbvh_fitted) return P3D_OK;
  hipError_t e = hipSuccess;
  if (!s->lbvh_topology) e = lbvh::enqueue_topology(w, w.boxes);
  if (e == hipSuccess) e = lbvh::enqueue_fit(w, w.boxes, s->d_blob + s->off_ogeom, s->d_blob + s->off_nodes, s->d_blob + s->off_bgeom);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string(who) + ": fit: " + hipGetErrorString(e));
  s->lbvh_topology = s->lbvh_fitted = true;
  return P3D_OK;
}

// What every geometry update does behind the kernel that wrote the new object-order geometry, normals and boxes (`e`: what
// enqueueing that gave; ev0 is recorded): the BVH, the device-built grid, the waits and the scene's bookkeeping.
// With p3d_scene_set_auto_rebuild on, a REFIT reads the cost of the refitted tree back and runs the builder in the same
// call if it has grown past the ratio; the grid is built once, over the final tree's boxes.
int finish_update(p3d_scene* s, uint32_t mode, hipError_t e, const char* who, float* update_ms) {
  lbvh::Workspace& w = s->lbvh_ws;
  float4* blob = s->d_blob;
  const bool policy = s->auto_rebuild > 0.0f;
  bool rebuilt = mode == P3D_UPDATE_REBUILD;
  auto build = [&]() {
    s->lbvh_topology = false;
    e = lbvh::enqueue_topology(w, w.boxes);
  };
  auto fit = [&]() { e = lbvh::enqueue_fit(w, w.boxes, blob + s->off_ogeom, blob + s->off_nodes, blob + s->off_bgeom); };
  if (e == hipSuccess && rebuilt) build();
  if (e == hipSuccess) fit();
  lbvh::CostResult cost{};
  if (e == hipSuccess && policy && !rebuilt) {
    e = read_cost(w, &cost);
    if (e == hipSuccess && sah_of(cost) > (double)s->auto_rebuild * s->sah_baseline) {  // (+inf x 0 is NaN: never)
      rebuilt = true;
      build();
      if (e == hipSuccess) fit();
    }
  }
  if (e == hipSuccess && policy && rebuilt) e = read_cost(w, &cost);  // the new baseline
  // a device-built grid follows in full, in both modes; if that fails the grid is dropped and the rest of the update stands
  int grid_rc = P3D_OK;
  if (e == hipSuccess && s->has_grid) grid_rc = rebuild_grid(s, who);
  if (e == hipSuccess) e = hipEventRecord(s->ev1, 0);
  if (e == hipSuccess) e = hipEventSynchronize(s->ev1);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, s->ev0, s->ev1);
  uint32_t depth = 0;
  float4 root[2];
  if (e == hipSuccess) e = hipMemcpy(&depth, w.depth, sizeof(depth), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(root, blob + s->off_nodes, sizeof(root), hipMemcpyDeviceToHost);
  // whatever happened, the old geometry's memos are void
  ++s->geom_gen;
  drop_schedules(s);
  s->ho_chain_key.clear();
  s->lbvh_fitted = e == hipSuccess;
  if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string(who) + ": update: " + hipGetErrorString(e));
  if (rebuilt) {
    s->lbvh_topology = true;
    s->bvh_max_depth = depth;
  }
  s->last_update_rebuilt = rebuilt;
  s->refits_since_build = rebuilt ? 0u : s->refits_since_build + 1u;
  // with the policy off nothing was measured: what was recorded for the old boxes is void
  s->sah_baseline = !policy ? 0.0 : rebuilt ? sah_of(cost) : s->sah_baseline;
  s->root_min[0] = root[0].x; s->root_min[1] = root[0].y; s->root_min[2] = root[0].z;
  s->root_max[0] = root[1].x; s->root_max[1] = root[1].y; s->root_max[2] = root[1].z;
  s->root_stale = false;
  if (update_ms) *update_ms = ms;
  return grid_rc;  // (rebuild_grid has recorded its message)
}

// A caller's buffer that a kernel of scene `s` is about to read: refused if the runtime says it is host memory (pinned, or
// memory it has never seen) or memory of another device, or if it reports the allocation and the buffer ends behind it.  A
// pointer the runtime cannot answer for is let through: an allocator may hand out memory the queries do not know.
int device_buffer_usable(const p3d_scene* s, const void* p, size_t bytes, const std::string& what) {
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return P3D_OK;
  }
  if (attr.type == hipMemoryTypeHost || attr.type == hipMemoryTypeUnregistered) return fail(P3D_ERR_INVALID, what + " is host memory");
  if (attr.type == hipMemoryTypeDevice && attr.device != s->device)
    return fail(P3D_ERR_INVALID, what + " is memory of device " + std::to_string(attr.device) + ", the scene is on device " + std::to_string(s->device));
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();
    return P3D_OK;
  }
  const uintptr_t end = (uintptr_t)base + size, at = (uintptr_t)p;
  if (at < (uintptr_t)base || at > end || bytes > end - at)
    return fail(P3D_ERR_INVALID, what + " ends behind its allocation (" + std::to_string(bytes) + " bytes needed, " + std::to_string(at <= end ? end - at : 0) + " there)");
  return P3D_OK;
}

// What p3d_scene_bvh_cost and p3d_scene_set_auto_rebuild share: the waits, the builder's state, the two launches, 32 bytes back
int measure_cost(p3d_scene* s, const char* who, lbvh::CostResult* out) {
  P3D_HIP(hipSetDevice(s->device));
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  if (int rc = refresh_root_box(s)) return rc;
  if (int rc = ensure_fitted_workspace(s, who)) return rc;
  if (hipError_t e = read_cost(s->lbvh_ws, out); e != hipSuccess)
    return fail(P3D_ERR_NO_DEVICE, std::string(who) + ": cost: " + hipGetErrorString(e));
  return P3D_OK;
}

// What every geometry update refuses first, in this order; `null_arrays`: the route's own text if a counted array is null
int update_refused(const p3d_scene* s, uint32_t mode, const std::string& pre, const char* null_arrays) {
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  if (null_arrays) return fail(P3D_ERR_INVALID, pre + null_arrays);
  if (mode != P3D_UPDATE_REFIT && mode != P3D_UPDATE_REBUILD) return fail(P3D_ERR_INVALID, pre + "unknown mode");
  if (!s->device_bvh)
    return fail(P3D_ERR_INVALID, pre + "the scene was not created by p3d_scene_create_device_bvh (an uploaded tree cannot follow its objects)");
  if (s->uploaded_grid) return fail(P3D_ERR_INVALID, pre + "the scene carries the host's grid, which would go stale");
  return P3D_OK;
}

// Staged spans (upd::StagedRange, upd::StagedSource; each non-empty and inside the scene) as upd::find_span searches them:
// sorted by `first`, refused if two overlap (`noun`: "ranges", "sources"), `before` filled; `each` checks a span once it is
// known to be disjoint from those in front of it.  *total: the objects covered
template <class Span, class Each>
int sort_spans(std::vector<Span>& spans, const std::string& pre, const char* noun, uint32_t* total, Each&& each) {
  std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.first < b.first; });
  *total = 0;
  for (size_t r = 0; r < spans.size(); ++r) {
    Span& g = spans[r];
    if (r && spans[r - 1].first + spans[r - 1].count > g.first)
      return fail(P3D_ERR_INVALID, pre + "object " + std::to_string(g.first) + " is in two " + noun);
    g.before = *total;
    *total += g.count;  // (disjoint spans inside n_objs: no overflow)
    if (int rc = each(g)) return rc;
  }
  return P3D_OK;
}

// The rest copy of the transform routes, from the geometry of this moment if the scene has none.  The device is idle
int ensure_rest(p3d_scene* s, const char* who) {
  if (s->rest.p) return P3D_OK;
  const size_t rest_bytes = (size_t)3 * s->dev.n_objs * sizeof(float4);
  if (int rc = s->rest.ensure(rest_bytes)) return rc;
  if (hipError_t e = hipMemcpy(s->rest.p, s->d_blob + s->off_ogeom, rest_bytes, hipMemcpyDeviceToDevice); e != hipSuccess) {
    s->rest.release();
    return fail(P3D_ERR_NO_DEVICE, std::string(who) + ": rest copy: " + hipGetErrorString(e));
  }
  return P3D_OK;
}

// A geometry update from "validated, and s->stage_host holds a zeroed counter block and the payload" (or nothing: no upload)
// to the return code.  `launch(grid, block, payload, counters)` enqueues the route's kernel over `total` objects, if there
// are any.  make_rest: the route reads the rest pose, which until its first call IS the object-order geometry.  `failed`
// (null: the route counts nothing) words what the kernel left in the counter block, if anything.
template <class Launch>
int run_update(p3d_scene* s, uint32_t mode, const char* who, float* update_ms, uint32_t total, bool make_rest, Launch&& launch,
               const std::function<std::string(const uint32_t*)>& failed) {
  const size_t bytes = s->stage_host.size() * sizeof(uint4);
  if (int rc = begin_update(s, mode, who)) return rc;
  if (int rc = s->stage.ensure(bytes)) return rc;
  if (make_rest)
    if (int rc = ensure_rest(s, who)) return rc;
  // from here on the scene changes
  hipError_t e = hipEventRecord(s->ev0, 0);
  if (e == hipSuccess && bytes) e = hipMemcpyAsync(s->stage.p, s->stage_host.data(), bytes, hipMemcpyHostToDevice, 0);
  if (e == hipSuccess && total) {
    launch(dim3((total + lbvh::kThreads - 1) / lbvh::kThreads), dim3(lbvh::kThreads), (const uint4*)s->stage.p + 1, (uint32_t*)s->stage.p);
    e = hipGetLastError();
  }
  const int rc = finish_update(s, mode, e, who, update_ms);
  if (rc == P3D_ERR_NO_DEVICE || !failed) return rc;
  uint32_t bad[2] = {0, 0};
  P3D_HIP(hipMemcpy(bad, s->stage.p, sizeof(bad), hipMemcpyDeviceToHost));
  if (rc || !(bad[0] | bad[1])) return rc;  // (a failed grid rebuild has recorded its message)
  return fail(P3D_ERR_INVALID, std::string(who) + ": " + failed(bad));
}

// The sources of p3d_scene_update_geometry_device / p3d_scene_refit_device, each checked against the scene and its buffers
// against what the runtime knows of them, then sorted as find_span wants them; *total: the objects covered.  Makes the
// scene's device current (the pointer queries answer for the current device's context)
int stage_sources(const p3d_scene* s, const std::string& pre, uint32_t n_sources, const p3d_geom_source* sources,
                  std::vector<upd::StagedSource>& sorted, uint32_t* total) {
  const uint32_t n_objs = s->dev.n_objs;
  P3D_HIP(hipSetDevice(s->device));
  sorted.resize(n_sources);
  for (uint32_t r = 0; r < n_sources; ++r) {
    const p3d_geom_source& g = sources[r];
    const std::string at = pre + "source " + std::to_string(r);
    if (g.count == 0) return fail(P3D_ERR_INVALID, at + " is empty");
    if ((uint64_t)g.first + g.count > n_objs) return fail(P3D_ERR_INVALID, at + " ends behind the last object");
    if (g.kind != P3D_PRIM_TRIANGLE && g.kind != P3D_PRIM_SPHERE) return fail(P3D_ERR_INVALID, at + ": kind must be P3D_PRIM_TRIANGLE or P3D_PRIM_SPHERE");
    if (g.reserved[0] | g.reserved[1]) return fail(P3D_ERR_INVALID, at + ": reserved must be 0");
    if (!g.d_data) return fail(P3D_ERR_INVALID, at + ": null d_data");
    if (((uintptr_t)g.d_data | (uintptr_t)g.d_index) & 3u) return fail(P3D_ERR_INVALID, at + ": d_data and d_index must be 4-byte aligned");
    if (g.n_elems == 0) return fail(P3D_ERR_INVALID, at + ": n_elems is 0");
    if (g.kind == P3D_PRIM_SPHERE) {
      if (g.d_index) return fail(P3D_ERR_INVALID, at + ": d_index given for spheres");
      if (g.n_elems != g.count) return fail(P3D_ERR_INVALID, at + ": spheres need n_elems == count");
    } else if (!g.d_index && (uint64_t)g.n_elems != 3 * (uint64_t)g.count) {
      return fail(P3D_ERR_INVALID, at + ": a soup (d_index NULL) needs n_elems == 3 * count");
    }
    for (uint32_t o = g.first; o < g.first + g.count; ++o)
      if ((s->obj_tm[o] & 0xffu) != g.kind) return fail(P3D_ERR_INVALID, at + ": object " + std::to_string(o) + " is of another type");
    const size_t data_bytes = g.kind == P3D_PRIM_SPHERE ? (size_t)16 * g.count : (size_t)12 * g.n_elems;
    if (int rc = device_buffer_usable(s, g.d_data, data_bytes, at + ": d_data")) return rc;
    if (g.d_index)
      if (int rc = device_buffer_usable(s, g.d_index, (size_t)12 * g.count, at + ": d_index")) return rc;
    sorted[r] = upd::StagedSource{g.first, g.count, g.kind, 0u, (const float*)g.d_data, g.d_index, g.n_elems, {0u, 0u, 0u}};
  }
  return sort_spans(sorted, pre, "sources", total, [](const upd::StagedSource&) { return (int)P3D_OK; });
}

// What the stream forms (p3d_scene_refit_device, p3d_scene_pose_device) do behind their kernel on `st`, which wrote the
// object-order geometry, normals and boxes and zeroed the fit's arrival counters (`e`: what enqueueing it gave): the fit of
// the kept topology, and the scene's bookkeeping as after a waiting REFIT with the policy off.  Nothing here allocates,
// frees, waits or reads back
int finish_stream_refit(p3d_scene* s, hipStream_t st, hipError_t e, const std::string& pre) {
  lbvh::Workspace& w = s->lbvh_ws;
  float4* blob = s->d_blob;
  if (e == hipSuccess) e = lbvh::enqueue_fit(w, w.boxes, blob + s->off_ogeom, blob + s->off_nodes, blob + s->off_bgeom, st, true, true);
  // the old geometry's memos are void, as after every update
  ++s->geom_gen;
  void_schedules(s);
  s->ho_chain_key.clear();
  s->root_stale = true;
  s->lbvh_fitted = e == hipSuccess;
  if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, pre + "update: " + hipGetErrorString(e));
  s->last_update_rebuilt = false;
  ++s->refits_since_build;
  s->sah_baseline = 0.0;  // (the policy is off: nothing was measured)
  return P3D_OK;
}

// What the stream forms refuse behind their arguments, in the same words
int stream_form_unsupported(const p3d_scene* s, const std::string& pre, const char* waiting_form) {
  if (s->has_grid)
    return fail(P3D_ERR_UNSUPPORTED, pre + "the scene has a device-built grid, whose rebuild reads sizes back (" + waiting_form + " follows it)");
  if (s->auto_rebuild != 0.0f)
    return fail(P3D_ERR_UNSUPPORTED, pre + "the auto-rebuild policy is on and needs the cost on the host (" + waiting_form +
                                         " applies it, p3d_scene_set_auto_rebuild(0) switches it off)");
  return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_scene_camera(p3d_scene* s, p3d_camera* out) {
  if (!s || !out) return fail(P3D_ERR_INVALID, "p3d_scene_camera: null argument");
  const DevCamera& c = s->dev.cam;
  *out = p3d_camera{};
  const F3* src[4] = {&c.eye, &c.u, &c.v, &c.n};
  float* dst[4] = {out->eye, out->u, out->v, out->n};
  for (int i = 0; i < 4; ++i) {
    dst[i][0] = src[i]->x; dst[i][1] = src[i]->y; dst[i][2] = src[i]->z;
  }
  out->plane_dist = c.plane_dist; out->w = c.w; out->h = c.h; out->focal_ratio = c.focal_ratio; out->aperture = c.aperture;
  out->res_x = c.res_x; out->res_y = c.res_y;
  return P3D_OK;
}

int p3d_scene_set_camera(p3d_scene* s, const p3d_camera* cam) {
  if (!s || !cam) return fail(P3D_ERR_INVALID, "p3d_scene_set_camera: null argument");
  DevCamera& c = s->dev.cam;
  if (c.res_x <= 0 || c.res_y <= 0) return fail(P3D_ERR_INVALID, "p3d_scene_set_camera: the scene was created without a camera");
  if (cam->res_x != c.res_x || cam->res_y != c.res_y)
    return fail(P3D_ERR_INVALID, "p3d_scene_set_camera: the camera is for " + std::to_string(cam->res_x) + "x" + std::to_string(cam->res_y) +
                                     ", the scene renders " + std::to_string(c.res_x) + "x" + std::to_string(c.res_y) + " (fixed at create)");
  if (!camera_usable(*cam)) return fail(P3D_ERR_INVALID, "p3d_scene_set_camera: every field must be finite, and w, h and plane_dist > 0");
  P3D_HIP(hipSetDevice(s->device));
  // The scene's scratch and memos may still be in use by enqueued work: its tail stream and the caller's streams
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  if (int rc = refresh_root_box(s)) return rc;
  const DevCamera n = dev_camera(*cam);
  if (std::memcmp(&n, &c, sizeof(DevCamera)) == 0) return P3D_OK;  // the same view: nothing to forget
  c = n;
  ++s->cam_gen;
  // what was worked out for the primary rays of the old view: tile costs, the hit_stack hand-off's row chains and halos
  drop_schedules(s);
  s->ho_chain_key.clear();
  return P3D_OK;
}

int p3d_scene_update_prims(p3d_scene* s, uint32_t n, const uint32_t* object, const p3d_prim* prims, uint32_t mode, float* update_ms) {
  const char* who = "p3d_scene_update_prims";
  const std::string pre = std::string(who) + ": ";
  if (int rc = update_refused(s, mode, pre, n && (!object || !prims) ? "null array with n > 0" : nullptr)) return rc;
  const uint32_t n_objs = s->dev.n_objs;
  if (n > n_objs) return fail(P3D_ERR_INVALID, pre + "more records than objects (an index is repeated)");
  {
    std::vector<uint8_t> seen(n_objs, 0);
    for (uint32_t i = 0; i < n; ++i) {
      const p3d_prim& p = prims[i];
      if (object[i] >= n_objs) return fail(P3D_ERR_INVALID, pre + "object index out of range");
      if (seen[object[i]]) return fail(P3D_ERR_INVALID, pre + "object " + std::to_string(object[i]) + " appears twice");
      seen[object[i]] = 1;
      if (p.type > 0xffu || p.material > 0xffffffu || (p.type | (p.material << 8)) != s->obj_tm[object[i]])
        return fail(P3D_ERR_INVALID, pre + "object " + std::to_string(object[i]) + " changes its type or material");
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p.bmin[k]) || !std::isfinite(p.bmax[k]) || !(p.bmin[k] <= p.bmax[k]))
          return fail(P3D_ERR_INVALID, pre + "object " + std::to_string(object[i]) + " has a non-finite or inverted box");
    }
  }
  if (update_ms) *update_ms = 0.0f;
  if (n_objs == 0) return P3D_OK;
  // one upload, or none: the counter block (unused), the records
  static_assert(sizeof(upd::UpdateRecord) == 7 * sizeof(uint4), "the records are staged as uint4");
  s->stage_host.assign(n ? 1 + 7 * (size_t)n : 0, make_uint4(0, 0, 0, 0));
  for (uint32_t i = 0; i < n; ++i) {
    const upd::UpdateRecord rec{prims[i], object[i], {0u, 0u, 0u}};
    std::memcpy(s->stage_host.data() + 1 + 7 * (size_t)i, &rec, sizeof(rec));
  }
  auto launch = [&](dim3 grid, dim3 block, const uint4* payload, uint32_t*) {
    hipLaunchKernelGGL(upd::scatter_prims, grid, block, 0, 0, (const upd::UpdateRecord*)payload, n, n_objs, s->d_blob + s->off_ogeom,
                       s->d_blob + s->off_normals, s->lbvh_ws.boxes, (float4*)s->rest.p);
  };
  return run_update(s, mode, who, update_ms, n, false, launch, nullptr);
}

int p3d_scene_transform_prims(p3d_scene* s, uint32_t n_ranges, const p3d_xform_range* ranges, uint32_t n_xforms, const p3d_xform* xforms,
                              uint32_t mode, float* update_ms) {
  const char* who = "p3d_scene_transform_prims";
  const std::string pre = std::string(who) + ": ";
  if (int rc = update_refused(s, mode, pre, (n_ranges && !ranges) || (n_xforms && !xforms) ? "null array with a non-zero count" : nullptr)) return rc;
  const uint32_t n_objs = s->dev.n_objs;
  if (n_ranges > n_objs) return fail(P3D_ERR_INVALID, pre + "more ranges than objects (ranges overlap or are empty)");
  std::vector<uint8_t> diagonal(n_xforms, 0);  // the transform may move a box
  for (uint32_t x = 0; x < n_xforms; ++x) {
    const p3d_xform& t = xforms[x];
    for (int k = 0; k < 12; ++k)
      if (!std::isfinite(t.m[k])) return fail(P3D_ERR_INVALID, pre + "transform " + std::to_string(x) + " has a non-finite entry");
    if (!std::isfinite(t.sphere_scale) || !(t.sphere_scale > 0.0f))
      return fail(P3D_ERR_INVALID, pre + "transform " + std::to_string(x) + ": sphere_scale must be finite and > 0");
    if (t.reserved[0] | t.reserved[1] | t.reserved[2]) return fail(P3D_ERR_INVALID, pre + "transform " + std::to_string(x) + ": reserved must be 0");
    diagonal[x] = xform_is_positive_diagonal(t.m) ? 1 : 0;
  }
  std::vector<upd::StagedRange> sorted(n_ranges);
  for (uint32_t r = 0; r < n_ranges; ++r) {
    const p3d_xform_range& g = ranges[r];
    const std::string at = pre + "range " + std::to_string(r);
    if (g.count == 0) return fail(P3D_ERR_INVALID, at + " is empty");
    if ((uint64_t)g.first + g.count > n_objs) return fail(P3D_ERR_INVALID, at + " ends behind the last object");
    if (g.xform >= n_xforms) return fail(P3D_ERR_INVALID, at + " names a transform that is not there");
    if (g.reserved) return fail(P3D_ERR_INVALID, at + ": reserved must be 0");
    sorted[r] = upd::StagedRange{g.first, g.count, g.xform, 0u};
  }
  uint32_t total = 0;
  auto movable = [&](const upd::StagedRange& g) {
    for (uint32_t o = g.first; o < g.first + g.count; ++o) {
      const uint32_t type = s->obj_tm[o] & 0xffu;
      if (type == P3D_PRIM_PLANE) return fail(P3D_ERR_INVALID, pre + "object " + std::to_string(o) + " is a plane");
      if (type == P3D_PRIM_BOX && !diagonal[g.xform])
        return fail(P3D_ERR_INVALID, pre + "object " + std::to_string(o) + " is a box, and transform " + std::to_string(g.xform) +
                                         " is not a positive scale per axis and a translation");
    }
    return (int)P3D_OK;
  };
  if (int rc = sort_spans(sorted, pre, "ranges", &total, movable)) return rc;
  if (update_ms) *update_ms = 0.0f;
  if (n_objs == 0) return P3D_OK;
  // one upload: the counter (zero), the ranges, the transforms
  static_assert(sizeof(p3d_xform) == 64 && sizeof(p3d_xform_range) == 16, "p3d_xform is read as four float4, a range as one uint4");
  s->stage_host.assign(1 + (size_t)n_ranges + 4 * (size_t)n_xforms, make_uint4(0, 0, 0, 0));
  if (n_ranges) std::memcpy(s->stage_host.data() + 1, sorted.data(), (size_t)n_ranges * sizeof(uint4));
  if (n_xforms) std::memcpy(s->stage_host.data() + 1 + n_ranges, xforms, (size_t)n_xforms * sizeof(p3d_xform));
  auto launch = [&](dim3 grid, dim3 block, const uint4* payload, uint32_t* skipped) {
    hipLaunchKernelGGL(upd::transform_prims, grid, block, 0, 0, (const float4*)s->rest.p, payload, n_ranges, (const float4*)(payload + n_ranges),
                       n_xforms, total, n_objs, s->d_blob + s->off_ogeom, s->d_blob + s->off_normals, s->lbvh_ws.boxes, skipped);
  };
  return run_update(s, mode, who, update_ms, total, true, launch, [](const uint32_t* bad) {
    return std::to_string(bad[0]) + " object(s) would have a non-finite or inverted box and keep their geometry; the others are updated";
  });
}

int p3d_scene_update_geometry_device(p3d_scene* s, uint32_t n_sources, const p3d_geom_source* sources, uint32_t mode, float* update_ms) {
  const char* who = "p3d_scene_update_geometry_device";
  const std::string pre = std::string(who) + ": ";
  if (int rc = update_refused(s, mode, pre, n_sources && !sources ? "null sources with n_sources > 0" : nullptr)) return rc;
  const uint32_t n_objs = s->dev.n_objs;
  if (n_sources > n_objs) return fail(P3D_ERR_INVALID, pre + "more sources than objects (sources overlap or are empty)");
  std::vector<upd::StagedSource> sorted;
  uint32_t total = 0;
  if (int rc = stage_sources(s, pre, n_sources, sources, sorted, &total)) return rc;
  if (update_ms) *update_ms = 0.0f;
  if (n_objs == 0) return P3D_OK;
  // one upload: the two counters (zero), the sources
  s->stage_host.assign(1 + 3 * (size_t)n_sources, make_uint4(0, 0, 0, 0));
  if (n_sources) std::memcpy(s->stage_host.data() + 1, sorted.data(), (size_t)n_sources * sizeof(upd::StagedSource));
  auto launch = [&](dim3 grid, dim3 block, const uint4* payload, uint32_t* counters) {
    hipLaunchKernelGGL(upd::gather_geometry, grid, block, 0, 0, (const upd::StagedSource*)payload, n_sources, total, n_objs,
                       s->d_blob + s->off_ogeom, s->d_blob + s->off_normals, s->lbvh_ws.boxes, (float4*)s->rest.p, counters);
  };
  return run_update(s, mode, who, update_ms, total, false, launch, [](const uint32_t* bad) {
    return std::to_string(bad[0]) + " triangle(s) with an index >= n_elems, " + std::to_string(bad[1]) +
           " object(s) with a non-finite or inverted box: they keep their geometry; the others are updated";
  });
}

int p3d_scene_refit_device(p3d_scene* s, uint32_t n_sources, const p3d_geom_source* sources, void* hip_stream) {
  const char* who = "p3d_scene_refit_device";
  const std::string pre = std::string(who) + ": ";
  if (int rc = update_refused(s, P3D_UPDATE_REFIT, pre, n_sources && !sources ? "null sources with n_sources > 0" : nullptr)) return rc;
  const uint32_t n_objs = s->dev.n_objs;
  if (n_sources > n_objs) return fail(P3D_ERR_INVALID, pre + "more sources than objects (sources overlap or are empty)");
  if (int rc = stream_form_unsupported(s, pre, "p3d_scene_update_geometry_device")) return rc;
  if (n_sources > upd::kMaxArgSources)
    return fail(P3D_ERR_CAPACITY, pre + std::to_string(n_sources) + " sources, at most " + std::to_string(upd::kMaxArgSources) +
                                      " travel with one call (p3d_scene_update_geometry_device stages any number)");
  std::vector<upd::StagedSource> sorted;
  uint32_t total = 0;
  if (int rc = stage_sources(s, pre, n_sources, sources, sorted, &total)) return rc;
  if (n_objs == 0 || n_sources == 0) return P3D_OK;
  lbvh::Workspace& w = s->lbvh_ws;
  if (!w.n || !s->lbvh_topology || !s->d_refit_skipped) {
    // the setup, as the waiting forms do it: the builder's state and the topology of the tree in d_blob, behind everything
    // enqueued; and the counter block
    if (int rc = begin_update(s, P3D_UPDATE_REFIT, who)) return rc;
    if (!s->d_refit_skipped) {
      P3D_HIP(hipMalloc((void**)&s->d_refit_skipped, 2 * sizeof(uint32_t)));
      P3D_HIP(hipMemset(s->d_refit_skipped, 0, 2 * sizeof(uint32_t)));
    }
  }
  hipStream_t st = (hipStream_t)hip_stream;
  if (int rc = wait_for_tail(s, st)) return rc;  // the previous frame's tail reads the geometry (p3d_scene_set_tail_stream)
  // from here on the scene changes
  upd::ArgSources table{};
  std::copy(sorted.begin(), sorted.end(), table.s);
  float4* blob = s->d_blob;
  // (total <= n_objs = w.n: the grid that gathers also clears the fit's n_objs arrival counters)
  hipLaunchKernelGGL(upd::gather_geometry_args, dim3((n_objs + lbvh::kThreads - 1) / lbvh::kThreads), dim3(lbvh::kThreads), 0, st, table, n_sources,
                     total, n_objs, blob + s->off_ogeom, blob + s->off_normals, w.boxes, (float4*)s->rest.p, s->d_refit_skipped, s->d_status, w.visits);
  return finish_stream_refit(s, st, hipGetLastError(), pre);
}

int p3d_scene_set_rig(p3d_scene* s, uint32_t n_ranges, const p3d_xform_range* ranges, uint32_t n_xforms) {
  const char* who = "p3d_scene_set_rig";
  const std::string pre = std::string(who) + ": ";
  if (int rc = update_refused(s, P3D_UPDATE_REFIT, pre, n_ranges && !ranges ? "null ranges with n_ranges > 0" : nullptr)) return rc;
  if (n_ranges == 0) {  // no rig: the table goes (a hipFree waits for what may still read it)
    P3D_HIP(hipSetDevice(s->device));
    s->rig.release();
    s->rig_ranges = s->rig_xforms = s->rig_posed = 0;
    return P3D_OK;
  }
  const uint32_t n_objs = s->dev.n_objs;
  if (n_xforms == 0) return fail(P3D_ERR_INVALID, pre + "ranges without transforms (n_xforms is 0)");
  if (n_ranges > n_objs) return fail(P3D_ERR_INVALID, pre + "more ranges than objects (ranges overlap or are empty)");
  std::vector<upd::StagedRange> sorted(n_ranges);
  for (uint32_t r = 0; r < n_ranges; ++r) {
    const p3d_xform_range& g = ranges[r];
    const std::string at = pre + "range " + std::to_string(r);
    if (g.count == 0) return fail(P3D_ERR_INVALID, at + " is empty");
    if ((uint64_t)g.first + g.count > n_objs) return fail(P3D_ERR_INVALID, at + " ends behind the last object");
    if (g.xform >= n_xforms) return fail(P3D_ERR_INVALID, at + " names a transform that is not there");
    if (g.reserved) return fail(P3D_ERR_INVALID, at + ": reserved must be 0");
    sorted[r] = upd::StagedRange{g.first, g.count, g.xform, 0u};
  }
  // one word per object, on the host; a box is accepted here: whether its matrix suits it is only known on the device
  std::vector<uint32_t> table(n_objs, upd::kRigNotPosed);
  uint32_t total = 0;
  auto place = [&](const upd::StagedRange& g) {
    for (uint32_t o = g.first; o < g.first + g.count; ++o) {
      if ((s->obj_tm[o] & 0xffu) == P3D_PRIM_PLANE) return fail(P3D_ERR_INVALID, pre + "object " + std::to_string(o) + " is a plane");
      table[o] = g.xform;
    }
    return (int)P3D_OK;
  };
  if (int rc = sort_spans(sorted, pre, "ranges", &total, place)) return rc;
  // what a later pose needs and may not wait for: the builder's state and the topology behind everything enqueued (the
  // device is idle from here on: nothing reads the old table), the rest copy, the counter block, the table on the device
  if (int rc = begin_update(s, P3D_UPDATE_REFIT, who)) return rc;
  if (int rc = ensure_rest(s, who)) return rc;
  if (!s->pose_skipped.p) {
    if (int rc = s->pose_skipped.ensure(2 * sizeof(uint32_t))) return rc;
    P3D_HIP(hipMemset(s->pose_skipped.p, 0, 2 * sizeof(uint32_t)));
  }
  Scratch fresh;
  if (int rc = fresh.ensure((size_t)n_objs * sizeof(uint32_t))) return rc;
  P3D_HIP(hipMemcpy(fresh.p, table.data(), (size_t)n_objs * sizeof(uint32_t), hipMemcpyHostToDevice));
  s->rig = std::move(fresh);
  s->rig_ranges = n_ranges;
  s->rig_xforms = n_xforms;
  s->rig_posed = total;
  return P3D_OK;
}

int p3d_scene_rig(p3d_scene* s, uint32_t* n_ranges, uint32_t* n_xforms, uint32_t* n_posed_objects) {
  if (!s || !n_ranges || !n_xforms || !n_posed_objects) return fail(P3D_ERR_INVALID, "p3d_scene_rig: null argument");
  *n_ranges = s->rig_ranges;
  *n_xforms = s->rig_xforms;
  *n_posed_objects = s->rig_posed;
  return P3D_OK;
}

int p3d_scene_pose_device(p3d_scene* s, uint32_t n_xforms, const void* d_xforms, const void* d_sphere_scale, void* hip_stream) {
  const char* who = "p3d_scene_pose_device";
  const std::string pre = std::string(who) + ": ";
  if (int rc = update_refused(s, P3D_UPDATE_REFIT, pre, nullptr)) return rc;
  const uint32_t n_objs = s->dev.n_objs;
  if (n_objs == 0) return P3D_OK;
  if (!s->rig.p) return fail(P3D_ERR_INVALID, pre + "the scene has no rig (p3d_scene_set_rig)");
  if (n_xforms != s->rig_xforms)
    return fail(P3D_ERR_INVALID, pre + std::to_string(n_xforms) + " transforms, the rig was set for " + std::to_string(s->rig_xforms));
  if (!d_xforms) return fail(P3D_ERR_INVALID, pre + "null d_xforms");
  if (((uintptr_t)d_xforms | (uintptr_t)d_sphere_scale) & 3u) return fail(P3D_ERR_INVALID, pre + "d_xforms and d_sphere_scale must be 4-byte aligned");
  P3D_HIP(hipSetDevice(s->device));
  if (int rc = device_buffer_usable(s, d_xforms, (size_t)48 * n_xforms, pre + "d_xforms")) return rc;
  if (d_sphere_scale)
    if (int rc = device_buffer_usable(s, d_sphere_scale, (size_t)4 * n_xforms, pre + "d_sphere_scale")) return rc;
  if (int rc = stream_form_unsupported(s, pre, "p3d_scene_transform_prims")) return rc;
  lbvh::Workspace& w = s->lbvh_ws;
  if (!w.n || !s->lbvh_topology) {
    // a geometry update has failed with P3D_ERR_NO_DEVICE since the rig was set and voided the topology: the setup again
    if (int rc = begin_update(s, P3D_UPDATE_REFIT, who)) return rc;
  }
  hipStream_t st = (hipStream_t)hip_stream;
  if (int rc = wait_for_tail(s, st)) return rc;  // the previous frame's tail reads the geometry (p3d_scene_set_tail_stream)
  // from here on the scene changes
  float4* blob = s->d_blob;
  hipLaunchKernelGGL(upd::pose_rig, dim3((n_objs + lbvh::kThreads - 1) / lbvh::kThreads), dim3(lbvh::kThreads), 0, st, (const float4*)s->rest.p,
                     (const uint32_t*)s->rig.p, (const float*)d_xforms, (const float*)d_sphere_scale, n_xforms, n_objs, blob + s->off_ogeom,
                     blob + s->off_normals, w.boxes, (uint32_t*)s->pose_skipped.p, s->d_status, w.visits);
  return finish_stream_refit(s, st, hipGetLastError(), pre);
}

int p3d_scene_export_bvh(p3d_scene* s, p3d_bvh_node* nodes, uint32_t* n_nodes, uint32_t* prim_index, uint32_t* n_prim_index, uint32_t* max_depth) {
  if (!s) return fail(P3D_ERR_INVALID, "p3d_scene_export_bvh: null scene");
  if (!n_nodes || !n_prim_index) return fail(P3D_ERR_INVALID, "p3d_scene_export_bvh: null size argument");
  if (nodes && !prim_index) return fail(P3D_ERR_INVALID, "p3d_scene_export_bvh: nodes without prim_index");
  if (!s->device_bvh) return fail(P3D_ERR_INVALID, "p3d_scene_export_bvh: the scene was not created by p3d_scene_create_device_bvh");
  const uint32_t n = s->dev.n_objs;
  if (max_depth) *max_depth = s->bvh_max_depth;
  if (n == 0) {
    *n_nodes = *n_prim_index = 0;
    return P3D_OK;
  }
  P3D_HIP(hipSetDevice(s->device));
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  const uint32_t n_rec = 2 * n - 1;
  std::vector<float4> rec((size_t)2 * n_rec), geom((size_t)3 * n);
  P3D_HIP(hipMemcpy(rec.data(), s->d_blob + s->off_nodes, rec.size() * sizeof(float4), hipMemcpyDeviceToHost));
  P3D_HIP(hipMemcpy(geom.data(), s->d_blob + s->off_bgeom, geom.size() * sizeof(float4), hipMemcpyDeviceToHost));
  if (int rc = refresh_root_box(s)) return rc;  // (a call that waits anyway brings the cached root box up to date)
  // The device numbering (children of Karras node i at 1 + 2 i, 2 + 2 i) does not put children behind their parent, and a
  // pair of leaves emitted as one leaf leaves its child records unused: relabel by a depth-first walk, left child first
  std::vector<p3d_bvh_node> out;
  out.reserve(n_rec);
  out.push_back(p3d_bvh_node{});
  std::vector<std::pair<uint32_t, uint32_t>> todo{{0u, 0u}};  // (record on the device, index in `out`)
  while (!todo.empty()) {
    const auto [at, id] = todo.back();
    todo.pop_back();
    const float4 lo = rec[2 * (size_t)at], hi = rec[2 * (size_t)at + 1];
    uint32_t desc;
    std::memcpy(&desc, &lo.w, 4);
    p3d_bvh_node b{};
    b.bmin[0] = lo.x; b.bmin[1] = lo.y; b.bmin[2] = lo.z;
    b.bmax[0] = hi.x; b.bmax[1] = hi.y; b.bmax[2] = hi.z;
    if (desc & kDescLeaf) {
      b.index = desc_index(desc);
      b.count_leaf = P3D_BVH_LEAF | desc_count(desc);
      if ((uint64_t)b.index + desc_count(desc) > n) return fail(P3D_ERR_INVALID, "p3d_scene_export_bvh: leaf range out of bounds on the device");
    } else {
      if ((uint64_t)desc + 1 >= n_rec || out.size() + 2 > n_rec) return fail(P3D_ERR_INVALID, "p3d_scene_export_bvh: child index out of bounds on the device");
      b.index = (uint32_t)out.size();
      b.count_leaf = 0;
      out.push_back(p3d_bvh_node{});
      out.push_back(p3d_bvh_node{});
      todo.push_back({desc + 1, b.index + 1});
      todo.push_back({desc, b.index});  // on top: the left subtree is numbered first
    }
    out[id] = b;
  }
  const uint32_t have_nodes = *n_nodes, have_prims = *n_prim_index;
  *n_nodes = (uint32_t)out.size();
  *n_prim_index = n;
  if (!nodes) return P3D_OK;
  if (have_nodes < out.size() || have_prims < n)
    return fail(P3D_ERR_CAPACITY, "p3d_scene_export_bvh: the arrays are too small (call with nodes = NULL for the sizes)");
  std::memcpy(nodes, out.data(), out.size() * sizeof(p3d_bvh_node));
  for (uint32_t i = 0; i < n; ++i) std::memcpy(&prim_index[i], &geom[3 * (size_t)i + 2].z, 4);  // geom_of: the object index
  return P3D_OK;
}

int p3d_scene_bvh_cost(p3d_scene* s, p3d_bvh_cost* out) {
  if (!s || !out) return fail(P3D_ERR_INVALID, "p3d_scene_bvh_cost: null argument");
  if (!s->device_bvh) return fail(P3D_ERR_INVALID, "p3d_scene_bvh_cost: the scene was not created by p3d_scene_create_device_bvh");
  p3d_bvh_cost c{};
  if (s->dev.n_objs) {
    lbvh::CostResult r{};
    if (int rc = measure_cost(s, "p3d_scene_bvh_cost", &r)) return rc;
    c.sah = sah_of(r);
    c.n_inner = r.n_inner;
    c.n_leaves = r.n_leaves;
    // a tree that no refit has touched since it was built is its own baseline
    if (s->sah_baseline == 0.0 && s->refits_since_build == 0) s->sah_baseline = c.sah;
  }
  c.sah_baseline = s->sah_baseline;
  c.refits_since_build = s->refits_since_build;
  c.last_update_rebuilt = s->last_update_rebuilt ? 1u : 0u;
  *out = c;
  return P3D_OK;
}

int p3d_scene_set_auto_rebuild(p3d_scene* s, float ratio) {
  if (!s) return fail(P3D_ERR_INVALID, "p3d_scene_set_auto_rebuild: null scene");
  if (!s->device_bvh) return fail(P3D_ERR_INVALID, "p3d_scene_set_auto_rebuild: the scene was not created by p3d_scene_create_device_bvh");
  if (!(ratio == 0.0f || ratio >= 1.0f)) return fail(P3D_ERR_INVALID, "p3d_scene_set_auto_rebuild: the ratio must be 0 (off) or >= 1");
  if (ratio == 0.0f) {
    s->auto_rebuild = 0.0f;
    s->sah_baseline = 0.0;
    return P3D_OK;
  }
  if (s->auto_rebuild == 0.0f && s->dev.n_objs) {  // switched on: the tree of this moment is what later refits are compared with
    lbvh::CostResult r{};
    if (int rc = measure_cost(s, "p3d_scene_set_auto_rebuild", &r)) return rc;
    s->sah_baseline = sah_of(r);
  }
  s->auto_rebuild = ratio;
  return P3D_OK;
}

int p3d_scene_auto_rebuild(p3d_scene* s, float* ratio) {
  if (!s || !ratio) return fail(P3D_ERR_INVALID, "p3d_scene_auto_rebuild: null argument");
  if (!s->device_bvh) return fail(P3D_ERR_INVALID, "p3d_scene_auto_rebuild: the scene was not created by p3d_scene_create_device_bvh");
  *ratio = s->auto_rebuild;
  return P3D_OK;
}

}  // extern "C"
