// capi_query.hpp — batched ray and per-object queries (p3d_trace_*, p3d_trace_hits_device, p3d_trace_radiance_device,
// p3d_camera_rays_device, p3d_trace_path_device, p3d_camera_sample_rays_device, p3d_occlusion_device, p3d_occlusion_rays_device,
// p3d_object_*, p3d_skybox_color, and the filtered forms of the segment family: p3d_trace_any_filtered_device,
// p3d_trace_hits_filtered_device, p3d_occlusion_filtered_device), and what every query over device buffers goes through:
// open_object_query, check_query_buffers, bind_query_stack, enqueue_query, and for a filter FilterArgs, check_filter,
// launch_filterable.  The proximity queries (nearest, sweep, segment, overlap) are capi_proximity.hpp's
#pragma once
#include "capi_dispatch.hpp"  // with_flags
#include "capi_frame_plan.hpp"  // stack_bound
#include "capi_update.hpp"  // device_buffer_usable
#include "hit_list_query.hpp"
#include "nearest_query.hpp"  // nearest_k_lds_bytes
#include "occlusion_query.hpp"
#include "path_query.hpp"
#include "query_refusals.hpp"
#include "radiance_query.hpp"
#include "ray_query.hpp"

namespace {

// What a launcher needs to start a traversing query kernel over n rays or points
struct QueryLaunch {
  QueryStack stack;  // for the kernel's parameters
  uint32_t blocks;
  size_t lds;        // bytes of dynamic LDS: the stack's window and what enqueue_query puts behind it
};

// The stack of one query launch: a 16-entry LDS window (a power of two) and, for a tree deeper than that, its worst case in
// the scene's spill area, which grows here if it has to (the one place a query may wait: in the hipFree of the old area).
// Refuses a batch whose spill entries 32-bit offsets cannot address (device_core.hpp Stack); `what` names its elements.
// chain: the lane runs a Whitted chain on its stack, whose feelers leave entries behind (Q2): the frames' worst case
// (capi_frame_plan.hpp stack_bound), not the depth of one traversal
int bind_query_stack(p3d_scene* s, uint32_t accel, uint32_t n, const std::string& pre, const char* what, QueryLaunch& out, bool chain = false) {
  const uint32_t one = accel == P3D_ACCEL_BVH ? std::max<uint32_t>(1, s->bvh_max_depth) : 1;
  const uint32_t bound = chain ? std::max(one, stack_bound(scene_facts(s), accel, true)) : one;
  const uint32_t cap = 16;
  out.blocks = (n + kBlock - 1) / kBlock;
  const uint64_t spill_entries = (uint64_t)(bound > cap ? bound : 0) * out.blocks * kBlock;
  if (spill_entries > 0xffffffffull)
    return fail(P3D_ERR_CAPACITY, pre + "too many " + what + " for one call over a tree this deep (split the batch)");
  if (int rc = s->spill.ensure(std::max<size_t>(16, (size_t)spill_entries * sizeof(uint2)))) return rc;
  out.stack.spill = (uint2*)s->spill.p; out.stack.spill_stride = out.blocks * kBlock; out.stack.stack_cap = (int32_t)cap;
  out.lds = (size_t)cap * kBlock * sizeof(uint2);
  return P3D_OK;
}

// ray_query_kernel<accel, any, EXTRAS> on `st`
template <bool EXTRAS>
void launch_ray_query(uint32_t accel, bool any, const QueryLaunch& q, hipStream_t st, const RayQueryParams& P) {
  with_accel(accel, [&](auto A) {
    with_flags([&](auto ANY) { hipLaunchKernelGGL((ray_query_kernel<decltype(A)::value, ANY, EXTRAS>), dim3(q.blocks), dim3(kBlock), q.lds, st, P); }, any);
  });
}

// One buffer argument of a device-buffer query: null = not given
struct QueryBuffer {
  const void* p;
  size_t bytes;
  const char* name;
  bool aligned4 = true;  // floats or int32s
  bool aligned8 = false; // uint64s
};

// What the device-buffer queries do once their own refusals have passed: the refusals of the buffers in `bufs`, the stack
// (`what` names the batch's elements), and one launch on the caller's stream; launch(q, st) enqueues the kernel, q.lds being
// the stack window and `list_lds` bytes behind it; `chain`: see bind_query_stack.  No wait anywhere but in a hipFree of a spill
// area that has to grow.
// The refusals of the buffers of a device-buffer call: alignment, then where each lies and how far it reaches
template <size_t N>
int check_query_buffers(p3d_scene* s, const std::string& pre, const QueryBuffer (&bufs)[N]) {
  for (const auto& b : bufs)
    if (b.aligned4 && ((uintptr_t)b.p & 3u)) return fail(P3D_ERR_INVALID, pre + "the float and int32 buffers must be 4-byte aligned");
  for (const auto& b : bufs)
    if (b.aligned8 && ((uintptr_t)b.p & 7u)) return fail(P3D_ERR_INVALID, pre + b.name + " must be 8-byte aligned");
  P3D_HIP(hipSetDevice(s->device));  // the pointer queries below answer for the current device's context
  for (const auto& b : bufs)
    if (b.p)
      if (int rc = device_buffer_usable(s, b.p, b.bytes, pre + b.name)) return rc;
  return P3D_OK;
}

template <size_t N, class Launch>
int enqueue_query(p3d_scene* s, uint32_t accel, uint32_t n, const std::string& pre, const char* what, const QueryBuffer (&bufs)[N],
                  size_t list_lds, void* hip_stream, Launch&& launch, bool chain = false) {
  if (int rc = check_query_buffers(s, pre, bufs)) return rc;
  QueryLaunch q;
  if (int rc = bind_query_stack(s, accel, n, pre, what, q, chain)) return rc;
  q.lds += list_lds;
  hipStream_t st = (hipStream_t)hip_stream;
  if (int rc = wait_for_tail(s, st)) return rc;  // the spill area is in use until the previous frame's tail has run (p3d_scene_set_tail_stream)
  launch(q, st);
  P3D_HIP(hipGetLastError());
  return P3D_OK;
}

// The opening refusals of a per-object query over device buffers, in the one order all of them have: a null scene, the grid
// ("no <noun> through the grid"), check_accel, a box in the scene (no_box: the query's sentence of query_refusals.hpp; null:
// boxes are taken) and, asked for, a plane under P3D_ACCEL_BVH.  Each entry point's own checks follow
int open_object_query(const p3d_scene* s, uint32_t accel, const std::string& pre, const char* noun, const char* no_box = nullptr,
                      bool no_plane_under_tree = false) {
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  if (accel == P3D_ACCEL_GRID) return fail(P3D_ERR_UNSUPPORTED, pre + "no " + noun + " through the grid (use P3D_ACCEL_BVH or P3D_ACCEL_NONE)");
  if (int rc = check_accel(s, accel)) return rc;
  if (no_box && s->first_box >= 0) return fail(P3D_ERR_UNSUPPORTED, pre + refuse_box((int)s->first_box, no_box));
  if (no_plane_under_tree && accel == P3D_ACCEL_BVH && s->has_planes) return fail(P3D_ERR_UNSUPPORTED, pre + kRefusePlaneUnderTree);
  return P3D_OK;
}

// The skip buffers of a *_filtered_device call (include/p3d_filter.h).  The unfiltered entry points pass none: a null
// FilterArgs*, the same checks and launches as before
struct FilterArgs {
  const int32_t* d_skip;  // n x n_skip, or null
  uint32_t n_skip;
  const int32_t* d_skip_range;  // n x 2, or null
  bool absent() const { return n_skip == 0 && !d_skip_range; }  // the call is the unfiltered call: its kernel is launched
};
// What a filtered call refuses of its filter whatever n is, and with n > 0
int check_filter(const FilterArgs& fa, const std::string& pre) {
  if (fa.n_skip > P3D_FILTER_SKIP_MAX) return fail(P3D_ERR_INVALID, pre + kRefuseSkipCount);
  return P3D_OK;
}
int check_filter_buffers(const FilterArgs& fa, const std::string& pre) {
  if (fa.n_skip > 0 && !fa.d_skip) return fail(P3D_ERR_INVALID, pre + "null argument (d_skip is needed with n_skip > 0)");
  return P3D_OK;
}
FilterParams filter_params(const FilterArgs& fa) { return FilterParams{fa.n_skip ? fa.d_skip : nullptr, fa.d_skip_range, fa.n_skip}; }

// One kernel family under P3D_ACCEL_NONE or P3D_ACCEL_BVH, without or with a filter: launch(A, params) is called with the
// accel as a std::integral_constant and with the bare P (no filter given: the unfiltered kernel) or Filtered{P, F}; it names
// the kernel template and launches kernel<decltype(A)::value> with `params`
template <class Filtered, class P, class Launch>
void launch_filterable(uint32_t accel, const FilterArgs& fa, const P& params, Launch&& launch) {
  with_flags([&](auto BVH) {
    constexpr std::integral_constant<int, BVH ? P3D_ACCEL_BVH : P3D_ACCEL_NONE> A{};
    if (fa.absent()) launch(A, params);
    else launch(A, Filtered{params, filter_params(fa)});
  }, accel == P3D_ACCEL_BVH);
}

// p3d_trace_closest_device / p3d_trace_any_device and, with `filter`, p3d_trace_any_filtered_device: the segment query alone
// (the grid and a call without d_t_max are refused), launched with launch_filterable like the other filtered queries
int trace_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, const float* d_t_max,
                 int32_t* d_hit_id, float* d_t, float* d_hit_point, float* d_normal, uint8_t* d_occluded, void* hip_stream, bool any,
                 const FilterArgs* filter = nullptr) {
  const std::string pre = filter ? "p3d_trace_any_filtered_device: " : any ? "p3d_trace_any_device: " : "p3d_trace_closest_device: ";
  const FilterArgs fa = filter ? *filter : FilterArgs{nullptr, 0, nullptr};
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  if (int rc = check_accel(s, accel)) return rc;
  if (accel == P3D_ACCEL_GRID && s->dev.n_objs == 0) return fail(P3D_ERR_UNSUPPORTED, "grid over an empty scene");
  if (any && (d_t_max || filter) && accel == P3D_ACCEL_GRID)
    return fail(P3D_ERR_UNSUPPORTED, pre + "no segment query through the grid (P3D_ACCEL_NONE gives the answer the grid's feeler would: it runs the brute-force loop as well)");
  if (int rc = check_filter(fa, pre)) return rc;
  if (n == 0) return P3D_OK;
  if (!d_origin || !d_direction || (any ? !d_occluded : !d_hit_id)) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (filter && !d_t_max)
    return fail(P3D_ERR_INVALID, pre + "null argument (d_t_max is needed: pass +inf for a half-line; the feeler without a limit has no filtered form)");
  if (int rc = check_filter_buffers(fa, pre)) return rc;
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);
  const FilterParams F = filter_params(fa);  // (null without a filter: a null buffer is not looked at)
  const QueryBuffer bufs[] = {
      {d_origin, vec, "d_origin"}, {d_direction, vec, "d_direction"}, {d_t_max, one, "d_t_max"},
      {F.skip, one * fa.n_skip, "d_skip"}, {F.range, one * 2, "d_skip_range"}, {d_hit_id, one, "d_hit_id"},
      {d_t, one, "d_t"}, {d_hit_point, vec, "d_hit_point"}, {d_normal, vec, "d_normal"}, {d_occluded, (size_t)n, "d_occluded", false}};
  return enqueue_query(s, accel, n, pre, "rays", bufs, 0, hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    RayQueryParams P{};
    P.sc = s->dev; P.n = n; P.origin = d_origin; P.direction = d_direction; P.t_max = d_t_max;
    P.hit_id = d_hit_id; P.t = d_t; P.hit_point = d_hit_point; P.normal = d_normal; P.occluded = d_occluded; P.stack = q.stack;
    if (!filter) return launch_ray_query<true>(accel, any, q, st, P);
    // (the segment any-hit under P3D_ACCEL_NONE or P3D_ACCEL_BVH: an absent filter launches the instantiation launch_ray_query would)
    launch_filterable<RayQueryFilteredParams>(accel, fa, P, [&](auto A, const auto& params) {
      hipLaunchKernelGGL((ray_query_kernel<decltype(A)::value, true, true>), dim3(q.blocks), dim3(kBlock), q.lds, st, params);
    });
  });
}

// What p3d_camera_rays_device and p3d_camera_sample_rays_device refuse alike, and what they then work with: the camera (the
// argument's or the scene's), the tile with its stripes resolved, and the two ray buffers checked for w*h rows
struct CameraRaysCall {
  DevCamera cam;
  p3d_tile tile;  // stripe_h >= 1
  size_t pixels;
};
int check_camera_rays(p3d_scene* s, const p3d_camera* camera, const std::string& pre, CameraRaysCall& out) {
  const DevCamera& own = s->dev.cam;
  if (own.res_x <= 0 || own.res_y <= 0) return fail(P3D_ERR_INVALID, pre + "scene has no camera");
  if (camera) {
    if (camera->res_x != own.res_x || camera->res_y != own.res_y)
      return fail(P3D_ERR_INVALID, pre + "the camera is for " + std::to_string(camera->res_x) + "x" + std::to_string(camera->res_y) +
                                       ", the scene renders " + std::to_string(own.res_x) + "x" + std::to_string(own.res_y));
    if (!camera_usable(*camera)) return fail(P3D_ERR_INVALID, pre + "every field of the camera must be finite, and w, h and plane_dist > 0");
  }
  out.cam = camera ? dev_camera(*camera) : own;
  return P3D_OK;
}
int check_camera_rays_tile(p3d_scene* s, const p3d_tile* tile, float* d_origin, float* d_direction, const std::string& pre, CameraRaysCall& out) {
  const DevCamera& cam = out.cam;
  const p3d_tile whole{0, 0, cam.res_x, cam.res_y, 0, 1};
  const p3d_tile& t = tile ? *tile : whole;
  const int sh = t.stripe_h > 0 ? t.stripe_h : 1, ss = t.stripe_h > 0 ? t.stripe_stride : 1;
  if (t.w <= 0 || t.h <= 0 || t.x0 < 0 || t.y0 < 0 || ss < 1 || t.x0 + t.w > cam.res_x) return fail(P3D_ERR_INVALID, pre + "tile outside the image");
  {
    const int last = t.h - 1;
    const long long ylast = (long long)t.y0 + (long long)(last / sh) * sh * ss + (last % sh);
    if (ylast >= cam.res_y) return fail(P3D_ERR_INVALID, pre + "tile rows outside the image");
  }
  if (!d_origin || !d_direction) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (((uintptr_t)d_origin | (uintptr_t)d_direction) & 3u) return fail(P3D_ERR_INVALID, pre + "the float buffers must be 4-byte aligned");
  out.tile = p3d_tile{t.x0, t.y0, t.w, t.h, sh, ss};
  out.pixels = (size_t)t.w * (size_t)t.h;
  const size_t vec = out.pixels * 3 * sizeof(float);
  P3D_HIP(hipSetDevice(s->device));
  if (int rc = device_buffer_usable(s, d_origin, vec, pre + "d_origin")) return rc;
  if (int rc = device_buffer_usable(s, d_direction, vec, pre + "d_direction")) return rc;
  return P3D_OK;
}

// The lanes of a team (p3d_occlusion_params.team) as the TEAM template argument of a launch: f is called with a
// std::integral_constant of 1, 2, 4, ... 64
template <class F>
void with_team(uint32_t team, F&& f) {
  switch (team) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

// The free samples of the hemisphere above every point, one kernel on the caller's stream (occlusion_query.hpp);
// with `filter`, p3d_occlusion_filtered_device: one filter row per point
int occlusion_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_point, const float* d_normal, const float* d_max_dist,
                     const p3d_occlusion_params* params, uint32_t* d_unoccluded, float* d_bent, void* hip_stream, const FilterArgs* filter) {
  const std::string pre = filter ? "p3d_occlusion_filtered_device: " : "p3d_occlusion_device: ";
  const FilterArgs fa = filter ? *filter : FilterArgs{nullptr, 0, nullptr};
  if (int rc = open_object_query(s, accel, pre, "segment query")) return rc;
  if (const char* why = occlusion_params_refusal(params)) return fail(P3D_ERR_INVALID, pre + why);
  if (int rc = check_filter(fa, pre)) return rc;
  if (n == 0) return P3D_OK;
  if (!d_point || !d_normal || !d_unoccluded) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (int rc = check_filter_buffers(fa, pre)) return rc;
  uint32_t team = params->team;
  if (team == 0)
    for (team = 1; team < std::min<uint32_t>(params->samples, kBlock); team *= 2) {}  // the smallest power of two >= min(samples, 64)
  const uint64_t lanes = (uint64_t)n * team;
  if (lanes > 0xffffffc0ull)  // (whole waves are launched)
    return fail(P3D_ERR_CAPACITY, pre + "n x team lanes do not fit 32 bits (split the batch, or lower team)");
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);
  const FilterParams F = filter_params(fa);  // (null without a filter: a null buffer is not looked at)
  const QueryBuffer bufs[] = {{d_point, vec, "d_point"}, {d_normal, vec, "d_normal"}, {d_max_dist, one, "d_max_dist"},
                              {F.skip, one * fa.n_skip, "d_skip"}, {F.range, one * 2, "d_skip_range"},
                              {d_unoccluded, one, "d_unoccluded"}, {d_bent, vec, "d_bent"}};
  // (a stack per LANE: the spill area is sized by the lanes launched; every sample starts on a cleared stack: one traversal's worst case)
  return enqueue_query(s, accel, (uint32_t)lanes, pre, "lanes", bufs, 0, hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    OcclusionParams P{};
    P.sc = s->dev; P.n = n; P.point = d_point; P.normal = d_normal; P.max_dist = d_max_dist; P.seed = params->seed;
    P.samples = params->samples; P.sample_begin = params->sample_begin; P.point_offset = params->point_offset;
    P.accumulate = (params->flags & P3D_OCCLUSION_ACCUMULATE) ? 1u : 0u; P.bias = params->bias;
    P.unoccluded = d_unoccluded; P.bent = d_bent; P.stack = q.stack;
    launch_filterable<OcclusionFilteredParams>(accel, fa, P, [&](auto A, const auto& launch_params) {
      with_team(team, [&](auto TEAM) {
        hipLaunchKernelGGL((occlusion_kernel<decltype(A)::value, decltype(TEAM)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, launch_params);
      });
    });
  });
}

// k == 0 is the pure count: d_total is required and the row outputs are not looked at.  With `filter`,
// p3d_trace_hits_filtered_device
int trace_hits_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, const float* d_origin, const float* d_direction,
                      const float* d_t_max, int32_t* d_count, int32_t* d_total, int32_t* d_object, float* d_t, float* d_hit_point,
                      float* d_normal, void* hip_stream, const FilterArgs* filter) {
  const std::string pre = filter ? "p3d_trace_hits_filtered_device: " : "p3d_trace_hits_device: ";
  const FilterArgs fa = filter ? *filter : FilterArgs{nullptr, 0, nullptr};
  if (int rc = open_object_query(s, accel, pre, "hit list")) return rc;
  if (k > P3D_TRACE_HITS_K_MAX) return fail(P3D_ERR_INVALID, pre + "k must be 0 .. P3D_TRACE_HITS_K_MAX (16)");
  if (int rc = check_filter(fa, pre)) return rc;
  if (n == 0) return P3D_OK;
  if (k == 0) d_count = d_object = nullptr, d_t = d_hit_point = d_normal = nullptr;
  if (!d_origin || !d_direction) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (k == 0 && !d_total) return fail(P3D_ERR_INVALID, pre + "null argument (k = 0 is the count alone: d_total is needed)");
  if (k > 0 && (!d_count || !d_object)) return fail(P3D_ERR_INVALID, pre + "null argument (d_count and d_object are needed with k >= 1)");
  if (int rc = check_filter_buffers(fa, pre)) return rc;
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);  // (64 bits: n k 12 < 2^40)
  const FilterParams F = filter_params(fa);  // (null without a filter: a null buffer is not looked at)
  const QueryBuffer bufs[] = {
      {d_origin, vec, "d_origin"}, {d_direction, vec, "d_direction"}, {d_t_max, one, "d_t_max"},
      {F.skip, one * fa.n_skip, "d_skip"}, {F.range, one * 2, "d_skip_range"}, {d_count, one, "d_count"},
      {d_total, one, "d_total"}, {d_object, one * k, "d_object"}, {d_t, one * k, "d_t"}, {d_hit_point, vec * k, "d_hit_point"},
      {d_normal, vec * k, "d_normal"}};
  // (the lists of this call's k behind the stack window; none for k = 0)
  return enqueue_query(s, accel, n, pre, "rays", bufs, nearest_k_lds_bytes(k), hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    TraceHitsParams P{};
    P.sc = s->dev; P.n = n; P.k = k; P.origin = d_origin; P.direction = d_direction; P.t_max = d_t_max;
    P.count = d_count; P.total = d_total; P.object = d_object; P.t = d_t; P.hit_point = d_hit_point; P.normal = d_normal; P.stack = q.stack;
    launch_filterable<TraceHitsFilteredParams>(accel, fa, P, [&](auto A, const auto& params) {
      hipLaunchKernelGGL((trace_hits_kernel<decltype(A)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, params);
    });
  });
}

}  // namespace

extern "C" {

int p3d_trace_radiance_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, int32_t max_depth,
                              uint32_t flags, float* d_rgb, int32_t* d_hit_id, void* hip_stream) {
  const std::string pre = "p3d_trace_radiance_device: ";
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  if (int rc = check_accel(s, accel)) return rc;
  if (accel == P3D_ACCEL_GRID && s->dev.n_objs == 0) return fail(P3D_ERR_UNSUPPORTED, "grid over an empty scene");
  if (max_depth < 0 || max_depth > (int32_t)P3D_RADIANCE_MAX_DEPTH) return fail(P3D_ERR_INVALID, pre + "max_depth must be 0 .. P3D_RADIANCE_MAX_DEPTH (16)");
  if (flags & ~P3D_RADIANCE_SKYBOX) return fail(P3D_ERR_INVALID, pre + "unknown flag");
  if ((flags & P3D_RADIANCE_SKYBOX) && !s->has_sky)
    return fail(P3D_ERR_INVALID, pre + "P3D_RADIANCE_SKYBOX but no cubemap was supplied (p3d_scene_set_skybox)");
  if (n == 0) return P3D_OK;
  if (!d_origin || !d_direction || !d_rgb) return fail(P3D_ERR_INVALID, pre + "null argument");
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);
  const QueryBuffer bufs[] = {{d_origin, vec, "d_origin"}, {d_direction, vec, "d_direction"}, {d_rgb, vec, "d_rgb"}, {d_hit_id, one, "d_hit_id"}};
  // (the level records of this call's depth behind the stack window; the stack of a chain)
  return enqueue_query(s, accel, n, pre, "rays", bufs, radiance_lds_bytes((uint32_t)max_depth), hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    RadianceQueryParams P{};
    P.sc = s->dev; P.n = n; P.origin = d_origin; P.direction = d_direction; P.max_depth = max_depth;
    P.skybox = (flags & P3D_RADIANCE_SKYBOX) ? 1u : 0u; P.rgb = d_rgb; P.hit_id = d_hit_id; P.stack = q.stack;
    with_accel(accel, [&](auto A) {
      hipLaunchKernelGGL((radiance_query_kernel<decltype(A)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, P);
    });
  }, true);
}

// One launch on the caller's stream, no wait, nothing of the scene's scratch
int p3d_camera_rays_device(p3d_scene* s, const p3d_camera* camera, const p3d_tile* tile, float* d_origin, float* d_direction, void* hip_stream) {
  const std::string pre = "p3d_camera_rays_device: ";
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  CameraRaysCall call;
  if (int rc = check_camera_rays(s, camera, pre, call)) return rc;
  if (call.cam.aperture != 0.0f) return fail(P3D_ERR_UNSUPPORTED, pre + "a lens camera (aperture != 0): its rays need the sampler");
  if (int rc = check_camera_rays_tile(s, tile, d_origin, d_direction, pre, call)) return rc;
  const p3d_tile& t = call.tile;
  CameraRaysParams C{};
  C.cam = call.cam; C.x0 = t.x0; C.y0 = t.y0; C.w = t.w; C.h = t.h; C.stripe_h = t.stripe_h; C.stripe_stride = t.stripe_stride;
  C.origin = d_origin; C.direction = d_direction;
  hipLaunchKernelGGL(camera_rays_kernel, dim3((uint32_t)((call.pixels + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, C);
  P3D_HIP(hipGetLastError());
  return P3D_OK;
}

// The sum of `samples` path-traced samples per ray, one kernel on the caller's stream
int p3d_trace_path_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, int32_t max_depth,
                          uint32_t sample_begin, uint32_t samples, uint64_t seed, uint64_t* d_rng, uint32_t flags, float* d_rgb,
                          int32_t* d_hit_id, void* hip_stream) {
  const std::string pre = "p3d_trace_path_device: ";
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  if (int rc = check_accel(s, accel)) return rc;
  if (accel == P3D_ACCEL_GRID && s->dev.n_objs == 0) return fail(P3D_ERR_UNSUPPORTED, "grid over an empty scene");
  if (max_depth < 0 || max_depth > 1024) return fail(P3D_ERR_INVALID, pre + "max_depth must be 0 .. 1024, as in a path-traced frame");
  if (samples == 0) return fail(P3D_ERR_INVALID, pre + "samples must be at least 1");
  if ((uint64_t)sample_begin + samples > 0x100000000ull) return fail(P3D_ERR_INVALID, pre + "sample_begin + samples must not pass 2^32");
  if (flags & ~(P3D_RADIANCE_SKYBOX | P3D_PATH_ACCUMULATE)) return fail(P3D_ERR_INVALID, pre + "unknown flag");
  if ((flags & P3D_RADIANCE_SKYBOX) && !s->has_sky)
    return fail(P3D_ERR_INVALID, pre + "P3D_RADIANCE_SKYBOX but no cubemap was supplied (p3d_scene_set_skybox)");
  if (n == 0) return P3D_OK;
  if (!d_origin || !d_direction || !d_rgb) return fail(P3D_ERR_INVALID, pre + "null argument");
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);
  const QueryBuffer bufs[] = {{d_origin, vec, "d_origin"}, {d_direction, vec, "d_direction"}, {d_rgb, vec, "d_rgb"}, {d_hit_id, one, "d_hit_id"},
                              {d_rng, (size_t)n * 2 * sizeof(uint64_t), "d_rng", false, true}};
  // (the pending dielectric branches behind the stack window; the stack of one traversal: closest-hit queries leave it empty)
  return enqueue_query(s, accel, n, pre, "rays", bufs, path_lds_bytes(), hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    PathQueryParams P{};
    P.sc = s->dev; P.n = n; P.origin = d_origin; P.direction = d_direction; P.max_depth = max_depth;
    P.skybox = (flags & P3D_RADIANCE_SKYBOX) ? 1u : 0u; P.accumulate = (flags & P3D_PATH_ACCUMULATE) ? 1u : 0u;
    P.sample_begin = sample_begin; P.samples = samples; P.seed = seed; P.rng = (RngWords*)d_rng;
    P.rgb = d_rgb; P.hit_id = d_hit_id; P.stack = q.stack;
    with_accel(accel, [&](auto A) {
      hipLaunchKernelGGL((path_query_kernel<decltype(A)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, P);
    });
  });
}

// One launch on the caller's stream, no wait, nothing of the scene's scratch
int p3d_camera_sample_rays_device(p3d_scene* s, const p3d_camera* camera, const p3d_tile* tile, const p3d_config* cfg, uint32_t sample,
                                  float* d_origin, float* d_direction, uint64_t* d_rng, void* hip_stream) {
  const std::string pre = "p3d_camera_sample_rays_device: ";
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  CameraRaysCall call;
  if (int rc = check_camera_rays(s, camera, pre, call)) return rc;
  if (!cfg) return fail(P3D_ERR_INVALID, pre + "null config");
  if (cfg->spp_sqrt == 0 || cfg->spp_sqrt > 1024) return fail(P3D_ERR_INVALID, pre + "spp_sqrt out of range");
  if (sample >= cfg->spp_sqrt * cfg->spp_sqrt) return fail(P3D_ERR_INVALID, pre + "sample must be below spp_sqrt * spp_sqrt");
  if (cfg->sample_mode > P3D_SAMPLE_TENT) return fail(P3D_ERR_INVALID, pre + "bad sample_mode");
  // (depth_of_field through a camera without an aperture: the frames take it, and so does this)
  if (int rc = check_camera_rays_tile(s, tile, d_origin, d_direction, pre, call)) return rc;
  if (d_rng) {
    if ((uintptr_t)d_rng & 7u) return fail(P3D_ERR_INVALID, pre + "d_rng must be 8-byte aligned");
    if (int rc = device_buffer_usable(s, d_rng, call.pixels * 2 * sizeof(uint64_t), pre + "d_rng")) return rc;
  }
  const p3d_tile& t = call.tile;
  CameraSampleRaysParams C{};
  C.cam = call.cam; C.x0 = t.x0; C.y0 = t.y0; C.w = t.w; C.h = t.h; C.stripe_h = t.stripe_h; C.stripe_stride = t.stripe_stride;
  C.spp_sqrt = cfg->spp_sqrt; C.antialiasing = cfg->antialiasing; C.depth_of_field = cfg->depth_of_field;
  C.sample_disk = cfg->sample_disk; C.sample_mode = cfg->sample_mode; C.sample = sample; C.seed = cfg->seed;
  C.origin = d_origin; C.direction = d_direction; C.rng = (RngWords*)d_rng;
  hipLaunchKernelGGL(camera_sample_rays_kernel, dim3((uint32_t)((call.pixels + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, C);
  P3D_HIP(hipGetLastError());
  return P3D_OK;
}

int p3d_occlusion_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_point, const float* d_normal, const float* d_max_dist,
                         const p3d_occlusion_params* params, uint32_t* d_unoccluded, float* d_bent, void* hip_stream) {
  return occlusion_device(s, accel, n, d_point, d_normal, d_max_dist, params, d_unoccluded, d_bent, hip_stream, nullptr);
}
int p3d_occlusion_filtered_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_point, const float* d_normal, const float* d_max_dist,
                                  const p3d_occlusion_params* params, const int32_t* d_skip, uint32_t n_skip, const int32_t* d_skip_range,
                                  uint32_t* d_unoccluded, float* d_bent, void* hip_stream) {
  const FilterArgs fa{d_skip, n_skip, d_skip_range};
  return occlusion_device(s, accel, n, d_point, d_normal, d_max_dist, params, d_unoccluded, d_bent, hip_stream, &fa);
}

// One launch on the caller's stream, no wait, nothing of the scene's scratch
int p3d_occlusion_rays_device(p3d_scene* s, uint32_t n, const float* d_point, const float* d_normal, const p3d_occlusion_params* params,
                              float* d_origin, float* d_direction, void* hip_stream) {
  const std::string pre = "p3d_occlusion_rays_device: ";
  if (!s) return fail(P3D_ERR_INVALID, pre + "null scene");
  if (const char* why = occlusion_params_refusal(params)) return fail(P3D_ERR_INVALID, pre + why);
  if (n == 0) return P3D_OK;
  if (!d_point || !d_normal || !d_origin || !d_direction) return fail(P3D_ERR_INVALID, pre + "null argument");
  const uint64_t rows = (uint64_t)n * params->samples;
  if (rows > 0xffffffffull) return fail(P3D_ERR_CAPACITY, pre + "n x samples rows do not fit 32 bits (split the batch)");
  const size_t vec = (size_t)n * 3 * sizeof(float), out = (size_t)rows * 3 * sizeof(float);
  const QueryBuffer bufs[] = {{d_point, vec, "d_point"}, {d_normal, vec, "d_normal"}, {d_origin, out, "d_origin"}, {d_direction, out, "d_direction"}};
  if (int rc = check_query_buffers(s, pre, bufs)) return rc;
  OcclusionRaysParams R{};
  R.n = n; R.point = d_point; R.normal = d_normal; R.seed = params->seed; R.samples = params->samples;
  R.sample_begin = params->sample_begin; R.point_offset = params->point_offset; R.bias = params->bias;
  R.origin = d_origin; R.direction = d_direction;
  hipLaunchKernelGGL(occlusion_rays_kernel, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, R);
  P3D_HIP(hipGetLastError());
  return P3D_OK;
}

static int trace_common(p3d_scene* s, uint32_t accel, uint32_t n, const float* origin, const float* direction, int32_t* hit_id,
                        float* t_host, float* hit_point, uint8_t* occluded, bool any) {
  if (!s || !origin || !direction || (any ? !occluded : !hit_id)) return fail(P3D_ERR_INVALID, "p3d_trace: null argument");
  if (int rc = check_accel(s, accel)) return rc;
  if (accel == P3D_ACCEL_GRID && s->dev.n_objs == 0) return fail(P3D_ERR_UNSUPPORTED, "grid over an empty scene");
  if (n == 0) return P3D_OK;
  P3D_HIP(hipSetDevice(s->device));
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;  // (the queries use the scene's scratch on the null stream)
  const size_t in_bytes = (size_t)n * 6 * sizeof(float);
  const size_t out_bytes = (size_t)n * (sizeof(int32_t) + 4 * sizeof(float) + 1) + 256;
  if (int rc = s->q_in.ensure(in_bytes)) return rc;
  if (int rc = s->q_out.ensure(out_bytes)) return rc;
  float* d_o = (float*)s->q_in.p;
  float* d_d = d_o + (size_t)n * 3;
  int32_t* d_hit = (int32_t*)s->q_out.p;
  float* d_hp = (float*)(d_hit + n);
  float* d_t = d_hp + (size_t)n * 3;
  uint8_t* d_occ = (uint8_t*)(d_t + n);
  P3D_HIP(hipMemcpy(d_o, origin, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  P3D_HIP(hipMemcpy(d_d, direction, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice));
  QueryLaunch q;
  if (int rc = bind_query_stack(s, accel, n, "p3d_trace: ", "rays", q)) return rc;
  RayQueryParams P{};  // the host form: no t_max, no normal
  P.sc = s->dev; P.n = n; P.origin = d_o; P.direction = d_d; P.hit_id = d_hit; P.hit_point = d_hp; P.occluded = d_occ;
  P.t = t_host ? d_t : nullptr; P.stack = q.stack;
  launch_ray_query<false>(accel, any, q, nullptr, P);
  P3D_HIP(hipGetLastError());
  P3D_HIP(hipDeviceSynchronize());
  if (any) {
    P3D_HIP(hipMemcpy(occluded, d_occ, n, hipMemcpyDeviceToHost));
  } else {
    P3D_HIP(hipMemcpy(hit_id, d_hit, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (hit_point) P3D_HIP(hipMemcpy(hit_point, d_hp, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (t_host) P3D_HIP(hipMemcpy(t_host, d_t, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  }
  return P3D_OK;
}

int p3d_trace_closest(p3d_scene* s, uint32_t accel, uint32_t n, const float* origin, const float* direction, int32_t* hit_id,
                      float* t, float* hit_point) {
  return trace_common(s, accel, n, origin, direction, hit_id, t, hit_point, nullptr, false);
}
int p3d_trace_any(p3d_scene* s, uint32_t accel, uint32_t n, const float* origin, const float* direction, uint8_t* occluded) {
  return trace_common(s, accel, n, origin, direction, nullptr, nullptr, nullptr, occluded, true);
}

int p3d_trace_closest_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, const float* d_t_max,
                             int32_t* d_hit_id, float* d_t, float* d_hit_point, float* d_normal, void* hip_stream) {
  return trace_device(s, accel, n, d_origin, d_direction, d_t_max, d_hit_id, d_t, d_hit_point, d_normal, nullptr, hip_stream, false);
}
int p3d_trace_any_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, const float* d_t_max,
                         uint8_t* d_occluded, void* hip_stream) {
  return trace_device(s, accel, n, d_origin, d_direction, d_t_max, nullptr, nullptr, nullptr, nullptr, d_occluded, hip_stream, true);
}

int p3d_trace_any_filtered_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, const float* d_t_max,
                                  const int32_t* d_skip, uint32_t n_skip, const int32_t* d_skip_range, uint8_t* d_occluded, void* hip_stream) {
  const FilterArgs fa{d_skip, n_skip, d_skip_range};
  return trace_device(s, accel, n, d_origin, d_direction, d_t_max, nullptr, nullptr, nullptr, nullptr, d_occluded, hip_stream, true, &fa);
}

int p3d_trace_hits_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, const float* d_origin, const float* d_direction,
                          const float* d_t_max, int32_t* d_count, int32_t* d_total, int32_t* d_object, float* d_t, float* d_hit_point,
                          float* d_normal, void* hip_stream) {
  return trace_hits_device(s, accel, n, k, d_origin, d_direction, d_t_max, d_count, d_total, d_object, d_t, d_hit_point, d_normal, hip_stream, nullptr);
}
int p3d_trace_hits_filtered_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, const float* d_origin, const float* d_direction,
                                   const float* d_t_max, const int32_t* d_skip, uint32_t n_skip, const int32_t* d_skip_range, int32_t* d_count,
                                   int32_t* d_total, int32_t* d_object, float* d_t, float* d_hit_point, float* d_normal, void* hip_stream) {
  const FilterArgs fa{d_skip, n_skip, d_skip_range};
  return trace_hits_device(s, accel, n, k, d_origin, d_direction, d_t_max, d_count, d_total, d_object, d_t, d_hit_point, d_normal, hip_stream, &fa);
}

enum class ObjectQuery { Intercepts = 0, Normal = 1, SkyboxColour = 2 };  // the values are object_query_kernel's WHAT

static int object_query(p3d_scene* s, ObjectQuery what, uint32_t object, uint32_t n, const float* a, float* b, uint8_t* hit, float* t) {
  const bool intercepts = what == ObjectQuery::Intercepts, sky = what == ObjectQuery::SkyboxColour;
  if (!s || !a || !b || (intercepts && (!hit || !t))) return fail(P3D_ERR_INVALID, "p3d object query: null argument");
  if (!sky && object >= s->dev.n_objs) return fail(P3D_ERR_INVALID, "p3d object query: no such object");
  if (sky && !s->has_sky) return fail(P3D_ERR_INVALID, "p3d_skybox_color: no cubemap was supplied (p3d_scene_set_skybox)");
  if (n == 0) return P3D_OK;
  P3D_HIP(hipSetDevice(s->device));
  // (no p3d_scene_join as in trace_common: only q_in / q_out are written here, which no frame launch touches, and a frame does not write the geometry)
  const size_t vec = (size_t)n * 3 * sizeof(float);
  if (int rc = s->q_in.ensure(vec)) return rc;
  if (int rc = s->q_out.ensure(vec + (size_t)n * (sizeof(float) + 1) + 64)) return rc;
  float* d_a = (float*)s->q_in.p;
  float* d_b = (float*)s->q_out.p;
  float* d_t = d_b + (size_t)n * 3;
  uint8_t* d_hit = (uint8_t*)(d_t + n);
  P3D_HIP(hipMemcpy(d_a, a, vec, hipMemcpyHostToDevice));
  if (intercepts) {
    P3D_HIP(hipMemcpy(d_b, b, vec, hipMemcpyHostToDevice));
    P3D_HIP(hipMemcpy(d_t, t, (size_t)n * sizeof(float), hipMemcpyHostToDevice));  // untouched where the test fails
  }
  ObjectQueryParams Q{};
  Q.sc = s->dev; Q.object = object; Q.n = n; Q.a = d_a; Q.b = d_b; Q.hit = d_hit; Q.t = d_t;
  const uint32_t blocks = (n + kBlock - 1) / kBlock;
  with_flags([&](auto INTERCEPTS, auto NORMAL) {
    constexpr ObjectQuery WHAT = INTERCEPTS ? ObjectQuery::Intercepts : (NORMAL ? ObjectQuery::Normal : ObjectQuery::SkyboxColour);
    hipLaunchKernelGGL((object_query_kernel<(int)WHAT>), dim3(blocks), dim3(kBlock), 0, 0, Q);
  }, intercepts, what == ObjectQuery::Normal);
  P3D_HIP(hipGetLastError());
  P3D_HIP(hipDeviceSynchronize());
  P3D_HIP(hipMemcpy(b, d_b, vec, hipMemcpyDeviceToHost));
  if (intercepts) {
    P3D_HIP(hipMemcpy(hit, d_hit, n, hipMemcpyDeviceToHost));
    P3D_HIP(hipMemcpy(t, d_t, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  }
  return P3D_OK;
}
int p3d_object_intercepts(p3d_scene* s, uint32_t object, uint32_t n, const float* origin, float* direction, uint8_t* hit, float* t) {
  return object_query(s, ObjectQuery::Intercepts, object, n, origin, direction, hit, t);
}
int p3d_object_normal(p3d_scene* s, uint32_t object, uint32_t n, const float* point, float* normal) {
  return object_query(s, ObjectQuery::Normal, object, n, point, normal, nullptr, nullptr);
}
int p3d_skybox_color(p3d_scene* s, uint32_t n, const float* direction, float* rgb) {
  return object_query(s, ObjectQuery::SkyboxColour, 0, n, direction, rgb, nullptr, nullptr);
}

}  // extern "C"
