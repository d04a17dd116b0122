// hit_list_query.hpp — the hits along a ray in order, over device buffers (p3d_trace_hits_device): one kernel,
// trace_hits_kernel, and one policy of the culled walk, bvh_segment_hits.  For every ray the (at most) k objects with the smallest
// (t, object) among those its segment hits, in that order, and the number of all of them: the ray-side twin of
// nearest_k_device_kernel.  The per-object predicate is ray_query.hpp's segment test (a fresh copy of the ray per test), the
// candidate list, its admission and its LDS storage are the nearest-k query's (host/nearest_rule.hpp NearestKGate and
// nearest_k_insert, nearest_query.hpp LdsNearestList) with t in the place of d2: `d2` is the name of the list's KEY there.
// Of device_core.hpp the node and geometry records and the slab test are used.
#pragma once

#include "nearest_query.hpp"  // LdsNearestList, nearest_k_lds_bytes
#include "ray_query.hpp"      // the segment query this one follows

namespace p3d {

// The state of one ray's search.  The gate (what a candidate must beat) stays in registers: LDS is touched only when a
// candidate is admitted.  k == 0, the pure count, has the gate (-inf, -1), which nothing beats: no list is touched, none exists.
struct HitListSearch {
  LdsNearestList list;
  NearestKGate gate;      // .d2 holds a t
  uint32_t count, k;
  uint32_t total;         // objects hit in front of the limit
  float limit;            // +inf without one
  bool want_total;        // wave-uniform (a kernel parameter)
  // What a node is culled against: the limit while all hits have to be seen (they are counted, or the list is not full:
  // the gate still is the limit then), the k-th entry's t otherwise
  __device__ __forceinline__ float bound() const { return want_total ? limit : gate.d2; }
};

// The gate of an empty list and the limit; false: the limit keeps nothing (a NaN, or <= 0)
__device__ __forceinline__ bool hit_list_open(const float* t_max, uint32_t i, HitListSearch& s) {
  s.limit = t_max ? t_max[i] : INFINITY;
  s.gate.d2 = s.k ? s.limit : -INFINITY;
  s.gate.object = -1;
  s.count = 0; s.total = 0;
  return !t_max || s.limit > 0.0f;
}

// segment_test, keeping its t: a hit in front of the limit is counted and offered to the list.  While the list is not full
// the gate is (limit, -1) and admission is t < limit once more; a NaN t passes neither comparison.
// An object the lane's filter names is not offered: it is not tested, not counted in total, not listed, and so tightens no
// bound (host/filter_rule.hpp).  NoFilter: the test is not compiled at all (nearest_k_offer has the reason)
template <class Filter, class CT>
__device__ __forceinline__ void hit_list_offer(const Geom& g, uint32_t slot, const RayS& ray, HitListSearch& s, const Filter& f, CT& ct) {
  if constexpr (Filter::kFilters) {
    if (filter_skips(f, (int32_t)geom_object(g))) return;
  }
  RayS r = ray;
  float t;
  if (intercepts(g, r, t, ct) && t < s.limit) {
    ++s.total;
    const int32_t object = (int32_t)geom_object(g);
    if (nearest_k_admits(t, object, s.gate)) nearest_k_insert(s.list, s.count, s.k, s.gate, t, object, slot);
  }
}

// P3D_ACCEL_NONE: every object, planes included
template <class Filter, class CT>
__device__ void brute_segment_hits(const DevScene& sc, const RayS& ray, HitListSearch& s, const Filter& f, CT& ct) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) hit_list_offer(load_geom(sc.ogeom, i), i, ray, s, f, ct);
}

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp) with bvh_segment_any's key of a box, never stopped by a hit.  What differs:
//   - a leaf offers each of its objects to the list; (t, object) is a total order and every object sits in one leaf, so the
//     order of the visits does not show in the answer;
//   - the cull is taken against s.bound(), not a constant.  The bound only shrinks when total is not wanted and the list is full;
//   - so the float of a stack entry is the child's t0, and a popped entry meets the cull again.
// The boxes are the whole scene's: a filter takes objects out of the leaves, never nodes out of the walk, and the bound of a
// filtered search shrinks no sooner than the unfiltered one's.
template <class Filter, class CT>
struct SegmentHitsWalk {
  const RayS& ray;
  HitListSearch& s;
  bool fin;  // slab_fast_path of the ray
  const Filter& f;
  CT& ct;
  __device__ __forceinline__ bool key(const NodeRec& n, float& order, float& stacked) const {
    return segment_box(n, ray, fin, s.bound(), order, stacked);
  }
  __device__ __forceinline__ bool culled(float t0) const { return t0 > s.bound(); }
  __device__ __forceinline__ bool left_first(float l_t, float r_t) const { return l_t < r_t; }
  __device__ __forceinline__ bool leaf(const DevScene& sc, uint32_t first, uint32_t end) {
    for (uint32_t g = first; g < end; ++g) hit_list_offer(load_geom(sc.bgeom, g), g, ray, s, f, ct);
    return false;
  }
};
template <class Filter, class CT>
__device__ void bvh_segment_hits(const DevScene& sc, Stack& st, const RayS& ray, HitListSearch& s, const Filter& f, CT& ct) {
  SegmentHitsWalk<Filter, CT> walk{ray, s, slab_fast_path<true>(sc, ray), f, ct};
  bvh_culled_walk(sc, st, walk, ct);
}

struct TraceHitsParams {
  DevScene sc;
  uint32_t n, k;           // 0 <= k <= P3D_TRACE_HITS_K_MAX
  const float* origin;     // n x 3
  const float* direction;  // n x 3, used as given
  const float* t_max;      // n, or null: no limit
  int32_t* count;          // n; k >= 1: required, like object (n x k).  k == 0: none of the row outputs is read or written
  int32_t* total;          // n, or null: not counted (k == 0: required)
  int32_t* object;
  float* t;                // n x k; optional, like hit_point and normal (n x k x 3)
  float* hit_point;
  float* normal;
  QueryStack stack;
};

// One ray per lane on an empty stack; the dynamic LDS holds the stack window and, behind it, the lists of the call's k (none
// for k == 0).  Row i k + j, j < count: the j-th listed object, its t, and - the test run once more at the listed slot on a
// fresh copy of the ray, nothing of it is carried through the search - o + d t of that copy and get_normal there, not turned.
// Rows j >= count: -1, FLT_MAX, zeros.
// k is a runtime argument, a lane writes its k rows itself, and the rays are read with dword loads: the three choices of
// nearest_k_device_kernel, UNMEASURED here as there (k as a template parameter; row stores through LDS; staged rays).
// Two kernels of one name, told apart by their parameters, for the reason nearest_k_device_kernel has two: the one launched
// without filters holds no filter code.  The filtered one (p3d_trace_hits_filtered_device) reads row i of the skip buffers once,
// before the walk, into ten registers.
struct TraceHitsFilteredParams {
  TraceHitsParams q;
  FilterParams f;
};
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) trace_hits_kernel(const TraceHitsParams P) {
  const NoFilterSource filters{};
#include "trace_hits_body.inc"
}
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) trace_hits_kernel(const TraceHitsFilteredParams PF) {
  const TraceHitsParams& P = PF.q;
  const FilterParams& filters = PF.f;
#include "trace_hits_body.inc"
}

}  // namespace p3d
