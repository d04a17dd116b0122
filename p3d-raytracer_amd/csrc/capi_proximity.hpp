// capi_proximity.hpp — the proximity queries over device buffers, each with its filtered form (p3d_nearest_device,
// p3d_nearest_k_device, p3d_nearest_k_filtered_device, p3d_sweep_sphere_device, p3d_sweep_sphere_filtered_device,
// p3d_nearest_segment_k_device, p3d_overlap_box_device).  Every one opens with open_object_query, keeps its own k / flag /
// filter / null-argument checks behind it, goes through enqueue_query (capi_query.hpp) and launches with launch_filterable.
#pragma once
#include "capi_query.hpp"  // open_object_query, QueryBuffer, enqueue_query, FilterArgs, check_filter, launch_filterable
#include "nearest_query.hpp"
#include "nearest_segment_query.hpp"
#include "overlap_query.hpp"
#include "query_refusals.hpp"
#include "sweep_query.hpp"

namespace {

// p3d_nearest_device (k_form false: k = 1, no d_count), p3d_nearest_k_device and, with `filter`, p3d_nearest_k_filtered_device.
// One set of checks for all; the outputs hold k rows per point
int nearest_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, bool k_form, const float* d_point, const float* d_max_dist,
                   int32_t* d_count, int32_t* d_object, float* d_dist, float* d_closest, float* d_normal, void* hip_stream,
                   const FilterArgs* filter = nullptr) {
  const std::string pre = filter ? "p3d_nearest_k_filtered_device: " : k_form ? "p3d_nearest_k_device: " : "p3d_nearest_device: ";
  const FilterArgs fa = filter ? *filter : FilterArgs{nullptr, 0, nullptr};
  if (int rc = open_object_query(s, accel, pre, "nearest-surface query", nullptr, true)) return rc;
  if (k == 0 || k > P3D_NEAREST_K_MAX) return fail(P3D_ERR_INVALID, pre + kRefuseNearestK);
  if (int rc = check_filter(fa, pre)) return rc;
  if (n == 0) return P3D_OK;
  if (!d_point || !d_object || (k_form && !d_count)) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (int rc = check_filter_buffers(fa, pre)) return rc;
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);  // (64 bits: n k 12 < 2^40)
  const FilterParams F = filter_params(fa);  // (null without a filter: a null buffer is not looked at)
  const QueryBuffer bufs[] = {
      {d_point, vec, "d_point"}, {d_max_dist, one, "d_max_dist"}, {F.skip, one * fa.n_skip, "d_skip"}, {F.range, one * 2, "d_skip_range"},
      {d_count, one, "d_count"}, {d_object, one * k, "d_object"},
      {d_dist, one * k, "d_dist"}, {d_closest, vec * k, "d_closest"}, {d_normal, vec * k, "d_normal"}};
  // (the lists of this call's k behind the stack window)
  return enqueue_query(s, accel, n, pre, "points", bufs, nearest_k_lds_bytes(k), hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    NearestKParams P{};
    P.sc = s->dev; P.n = n; P.k = k; P.point = d_point; P.max_dist = d_max_dist;
    P.count = d_count; P.object = d_object; P.dist = d_dist; P.closest = d_closest; P.normal = d_normal; P.stack = q.stack;
    launch_filterable<NearestKFilteredParams>(accel, fa, P, [&](auto A, const auto& params) {
      hipLaunchKernelGGL((nearest_k_device_kernel<decltype(A)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, params);
    });
  });
}

// The first contact of n moving balls, one kernel on the caller's stream (sweep_query.hpp); with `filter`,
// p3d_sweep_sphere_filtered_device
int sweep_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, const float* d_radius,
                 const float* d_t_max, int32_t* d_object, float* d_t, float* d_centre, float* d_contact, float* d_normal,
                 void* hip_stream, const FilterArgs* filter) {
  const std::string pre = filter ? "p3d_sweep_sphere_filtered_device: " : "p3d_sweep_sphere_device: ";
  const FilterArgs fa = filter ? *filter : FilterArgs{nullptr, 0, nullptr};
  if (int rc = open_object_query(s, accel, pre, "sphere sweep", kSweepNoBox, true)) return rc;
  if (int rc = check_filter(fa, pre)) return rc;
  if (n == 0) return P3D_OK;
  if (!d_origin || !d_direction || !d_radius || !d_object) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (int rc = check_filter_buffers(fa, pre)) return rc;
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);
  const FilterParams F = filter_params(fa);  // (null without a filter: a null buffer is not looked at)
  const QueryBuffer bufs[] = {
      {d_origin, vec, "d_origin"}, {d_direction, vec, "d_direction"}, {d_radius, one, "d_radius"}, {d_t_max, one, "d_t_max"},
      {F.skip, one * fa.n_skip, "d_skip"}, {F.range, one * 2, "d_skip_range"}, {d_object, one, "d_object"}, {d_t, one, "d_t"}, {d_centre, vec, "d_centre"}, {d_contact, vec, "d_contact"}, {d_normal, vec, "d_normal"}};
  // (the best contact stays in registers: nothing behind the stack window)
  return enqueue_query(s, accel, n, pre, "balls", bufs, 0, hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    SweepParams P{};
    P.sc = s->dev; P.n = n; P.origin = d_origin; P.direction = d_direction; P.radius = d_radius; P.t_max = d_t_max;
    P.object = d_object; P.t = d_t; P.centre = d_centre; P.contact = d_contact; P.normal = d_normal; P.stack = q.stack;
    launch_filterable<SweepFilteredParams>(accel, fa, P, [&](auto A, const auto& params) {
      hipLaunchKernelGGL((sweep_sphere_device_kernel<decltype(A)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, params);
    });
  });
}

}  // namespace

extern "C" {

int p3d_nearest_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_point, const float* d_max_dist, int32_t* d_object,
                       float* d_dist, float* d_closest, float* d_normal, void* hip_stream) {
  return nearest_device(s, accel, n, 1, false, d_point, d_max_dist, nullptr, d_object, d_dist, d_closest, d_normal, hip_stream);
}
int p3d_nearest_k_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, const float* d_point, const float* d_max_dist, int32_t* d_count,
                         int32_t* d_object, float* d_dist, float* d_closest, float* d_normal, void* hip_stream) {
  return nearest_device(s, accel, n, k, true, d_point, d_max_dist, d_count, d_object, d_dist, d_closest, d_normal, hip_stream);
}

int p3d_nearest_k_filtered_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, const float* d_point, const float* d_max_dist,
                                  const int32_t* d_skip, uint32_t n_skip, const int32_t* d_skip_range, int32_t* d_count, int32_t* d_object,
                                  float* d_dist, float* d_closest, float* d_normal, void* hip_stream) {
  const FilterArgs fa{d_skip, n_skip, d_skip_range};
  return nearest_device(s, accel, n, k, true, d_point, d_max_dist, d_count, d_object, d_dist, d_closest, d_normal, hip_stream, &fa);
}

int p3d_sweep_sphere_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction, const float* d_radius,
                            const float* d_t_max, int32_t* d_object, float* d_t, float* d_centre, float* d_contact, float* d_normal,
                            void* hip_stream) {
  return sweep_device(s, accel, n, d_origin, d_direction, d_radius, d_t_max, d_object, d_t, d_centre, d_contact, d_normal, hip_stream, nullptr);
}
int p3d_sweep_sphere_filtered_device(p3d_scene* s, uint32_t accel, uint32_t n, const float* d_origin, const float* d_direction,
                                     const float* d_radius, const float* d_t_max, const int32_t* d_skip, uint32_t n_skip,
                                     const int32_t* d_skip_range, int32_t* d_object, float* d_t, float* d_centre, float* d_contact,
                                     float* d_normal, void* hip_stream) {
  const FilterArgs fa{d_skip, n_skip, d_skip_range};
  return sweep_device(s, accel, n, d_origin, d_direction, d_radius, d_t_max, d_object, d_t, d_centre, d_contact, d_normal, hip_stream, &fa);
}

// The k nearest surfaces to n segments, one kernel on the caller's stream (nearest_segment_query.hpp).  The checks are
// p3d_nearest_k_filtered_device's, and the sweep's refusal of a box
int p3d_nearest_segment_k_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, const float* d_a, const float* d_b, const float* d_max_dist,
                                 const int32_t* d_skip, uint32_t n_skip, const int32_t* d_skip_range, int32_t* d_count, int32_t* d_object,
                                 float* d_dist, float* d_param, float* d_on_segment, float* d_closest, float* d_normal, void* hip_stream) {
  const std::string pre = "p3d_nearest_segment_k_device: ";
  const FilterArgs fa{d_skip, n_skip, d_skip_range};
  if (int rc = open_object_query(s, accel, pre, "nearest-surface query", kSegmentNoBox, true)) return rc;
  if (k == 0 || k > P3D_NEAREST_K_MAX) return fail(P3D_ERR_INVALID, pre + kRefuseNearestK);
  if (int rc = check_filter(fa, pre)) return rc;
  if (n == 0) return P3D_OK;
  if (!d_a || !d_b || !d_count || !d_object) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (int rc = check_filter_buffers(fa, pre)) return rc;
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);  // (64 bits: n k 12 < 2^40)
  const FilterParams F = filter_params(fa);  // (null without a filter: a null buffer is not looked at)
  const QueryBuffer bufs[] = {
      {d_a, vec, "d_a"}, {d_b, vec, "d_b"}, {d_max_dist, one, "d_max_dist"}, {F.skip, one * fa.n_skip, "d_skip"}, {F.range, one * 2, "d_skip_range"},
      {d_count, one, "d_count"}, {d_object, one * k, "d_object"}, {d_dist, one * k, "d_dist"}, {d_param, one * k, "d_param"},
      {d_on_segment, vec * k, "d_on_segment"}, {d_closest, vec * k, "d_closest"}, {d_normal, vec * k, "d_normal"}};
  // (the lists of this call's k behind the stack window)
  return enqueue_query(s, accel, n, pre, "segments", bufs, nearest_k_lds_bytes(k), hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    NearestSegmentParams P{};
    P.sc = s->dev; P.n = n; P.k = k; P.a = d_a; P.b = d_b; P.max_dist = d_max_dist;
    P.count = d_count; P.object = d_object; P.dist = d_dist; P.param = d_param; P.on_segment = d_on_segment; P.closest = d_closest;
    P.normal = d_normal; P.stack = q.stack;
    launch_filterable<NearestSegmentFilteredParams>(accel, fa, P, [&](auto A, const auto& params) {
      hipLaunchKernelGGL((nearest_segment_k_device_kernel<decltype(A)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, params);
    });
  });
}

// The objects that touch n boxes, one kernel on the caller's stream (overlap_query.hpp).  The checks are
// p3d_nearest_segment_k_device's, with p3d_trace_hits_device's k == 0: the count alone, no list behind the stack window
int p3d_overlap_box_device(p3d_scene* s, uint32_t accel, uint32_t n, uint32_t k, const float* d_lo, const float* d_hi, const int32_t* d_skip,
                           uint32_t n_skip, const int32_t* d_skip_range, uint32_t flags, int32_t* d_total, int32_t* d_object, void* hip_stream) {
  const std::string pre = "p3d_overlap_box_device: ";
  const FilterArgs fa{d_skip, n_skip, d_skip_range};
  if (int rc = open_object_query(s, accel, pre, "overlap query", nullptr, true)) return rc;
  if (k > P3D_NEAREST_K_MAX) return fail(P3D_ERR_INVALID, pre + kRefuseOverlapK);
  if (flags & ~P3D_OVERLAP_SOLID) return fail(P3D_ERR_INVALID, pre + kRefuseOverlapFlag);
  if (int rc = check_filter(fa, pre)) return rc;
  if (n == 0) return P3D_OK;
  if (k == 0) d_object = nullptr;
  if (!d_lo || !d_hi || !d_total) return fail(P3D_ERR_INVALID, pre + "null argument");
  if (k > 0 && !d_object) return fail(P3D_ERR_INVALID, pre + "null argument (d_object is needed with k >= 1)");
  if (int rc = check_filter_buffers(fa, pre)) return rc;
  const size_t vec = (size_t)n * 3 * sizeof(float), one = (size_t)n * sizeof(float);  // (64 bits: n k 4 < 2^40)
  const FilterParams F = filter_params(fa);  // (null without a filter: a null buffer is not looked at)
  const QueryBuffer bufs[] = {{d_lo, vec, "d_lo"}, {d_hi, vec, "d_hi"}, {F.skip, one * fa.n_skip, "d_skip"}, {F.range, one * 2, "d_skip_range"},
                              {d_total, one, "d_total"}, {d_object, one * k, "d_object"}};
  // (the lists of this call's k behind the stack window; none for k = 0)
  return enqueue_query(s, accel, n, pre, "boxes", bufs, overlap_lds_bytes(k), hip_stream, [&](const QueryLaunch& q, hipStream_t st) {
    OverlapParams P{};
    P.sc = s->dev; P.n = n; P.k = k; P.flags = flags; P.lo = d_lo; P.hi = d_hi; P.total = d_total; P.object = d_object; P.stack = q.stack;
    launch_filterable<OverlapFilteredParams>(accel, fa, P, [&](auto A, const auto& params) {
      hipLaunchKernelGGL((overlap_box_device_kernel<decltype(A)::value>), dim3(q.blocks), dim3(kBlock), q.lds, st, params);
    });
  });
}

}  // extern "C"
