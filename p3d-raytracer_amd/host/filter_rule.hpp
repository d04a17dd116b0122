// filter_rule.hpp — which objects a filtered query leaves out, in ONE place for its users: p3d_host_scene_nearest_k_filtered and
// p3d_host_scene_sweep_sphere_filtered (host_queries.cpp), which state the semantics by brute force, and the filtered instantiations
// of nearest_k_device_kernel and sweep_sphere_device_kernel (csrc/nearest_query.hpp, csrc/sweep_query.hpp), whose answers must be
// the host forms' bits; the segment and overlap queries (csrc/nearest_segment_query.hpp, csrc/overlap_query.hpp); and the filtered
// instantiations of the segment family of the ray queries, which have no host form: ray_query_kernel's any-hit with a limit,
// trace_hits_kernel and occlusion_kernel (csrc/ray_query.hpp, csrc/hit_list_query.hpp, csrc/occlusion_query.hpp), where the test
// stands in front of the ray-object test.  A filtered query is the unfiltered query over the scene without the objects its filter names: a skipped
// object is never offered, so it is not listed, is not the contact and tightens no bound.  No arithmetic of a query is here, only
// integer comparisons; a filter that names nothing leaves every bit of the unfiltered answer.
#pragma once

#include <cstdint>

#include "p3d.h"
#include "prim_rule.hpp"  // P3D_PRIM_HD

namespace p3d {

static_assert(P3D_FILTER_SKIP_MAX == 8, "QueryFilter and filter_skips spell eight slots out");

// The filter of ONE query.  skip: the row of the skip list, unused slots -1 (no object has that index, and neither has an entry
// < 0 or >= the object count: such an entry names nothing without being looked at).  first, count: the skip range cut to the
// scene, 0 <= first and first + count <= the object count; count == 0: no range.
// The list is eight named slots and not an array walked by a counter: filter_load and filter_skips touch every slot by a
// constant index, fully unrolled, so on the device the filter stays in registers (an array indexed at run time would go to
// scratch memory).
struct QueryFilter {
  static constexpr bool kFilters = true;  // (a user may leave the test out at compile time: NoFilter says false)
  int32_t skip[P3D_FILTER_SKIP_MAX];
  int32_t first, count;
};

// "No filter" as a type: what the unfiltered kernels and host forms are instantiated with.  Nothing is loaded and nothing is
// compared: the code is the code without a filter.
struct NoFilter {
  static constexpr bool kFilters = false;
};

// The filter of query i from the call's arguments: row i of `skip` (n x n_skip, n_skip <= 8; null or n_skip == 0: no list) and
// row i of `skip_range` (n x 2: first, count; null: no range), for a scene of n_objs objects.  The range is cut to
// [0, n_objs) in 64 bits, so that first + count cannot overflow and filter_skips compares 32-bit values
P3D_PRIM_HD inline QueryFilter filter_load(const int32_t* skip, uint32_t n_skip, const int32_t* skip_range, size_t i, uint32_t n_objs) {
  QueryFilter f;
  const int32_t* row = skip ? skip + i * n_skip : nullptr;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t s = 0; s < P3D_FILTER_SKIP_MAX; ++s) f.skip[s] = (row && s < n_skip) ? row[s] : -1;
  f.first = 0; f.count = 0;
  if (skip_range) {
    const int64_t first = skip_range[2 * i], count = skip_range[2 * i + 1];
    if (count > 0) {
      const int64_t lo = first > 0 ? first : 0, end = first + count, hi = end < (int64_t)n_objs ? end : (int64_t)n_objs;
      if (hi > lo) { f.first = (int32_t)lo; f.count = (int32_t)(hi - lo); }
    }
  }
  return f;
}

// Is `object` (0 <= object < the object count) left out?  On the list, or first <= object < first + count
P3D_PRIM_HD inline bool filter_skips(const QueryFilter& f, int32_t object) {
  bool listed = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t s = 0; s < P3D_FILTER_SKIP_MAX; ++s) listed |= f.skip[s] == object;
  return listed | ((uint32_t)(object - f.first) < (uint32_t)f.count);
}
P3D_PRIM_HD inline bool filter_skips(const NoFilter&, int32_t) { return false; }

}  // namespace p3d
