// ray_query.hpp — the batched ray queries, from host arrays (p3d_trace_closest, p3d_trace_any) and over device buffers
// (p3d_trace_closest_device, p3d_trace_any_device): ray_query_kernel, one body for both, and bvh_segment_any, the any-hit
// with a distance limit.  The unlimited paths call device_core.hpp's closest_hit / any_hit (bvh.cpp:198-340,
// grid.cpp:71-208, main.cpp:116-124,208-216), the segment query is a policy of the culled walk.  The segment query takes a
// lane's filter (p3d_trace_any_filtered_device); closest_hit and any_hit know none.
#pragma once

#include "queries.hpp"  // QueryStack, bvh_culled_walk, store_f3, FilterParams, NoFilterSource

namespace p3d {

// The segment query (DESIGN.md "Segment occlusion"):
//   occluded = some object j has intercepts(object j, a fresh copy of the ray, t) true and t < t_max.
// Every primitive is tested on a copy of the caller's ray, so a sphere test's re-normalisation (Q8) never reaches a later
// test and the answer does not depend on the order of the visits.  A NaN t (A10) and a NaN t_max keep nothing.
// An object the lane's filter names is not tested at all (host/filter_rule.hpp): the answer is a set over objects, so it is the
// answer over the scene without them.  NoFilter: the test is not compiled (nearest_k_offer has the reason).
template <class Filter, class CT>
__device__ __forceinline__ bool segment_test(const Geom& g, const RayS& ray, float t_max, const Filter& f, CT& ct) {
  if constexpr (Filter::kFilters) {
    if (filter_skips(f, (int32_t)geom_object(g))) return false;
  }
  RayS r = ray;
  float t;
  return intercepts(g, r, t, ct) && t < t_max;
}

// P3D_ACCEL_NONE: every object
template <class Filter, class CT>
__device__ bool brute_segment_any(const DevScene& sc, const RayS& ray, float t_max, const Filter& f, CT& ct) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) {
    const Geom g = load_geom(sc.ogeom, i);
    if (segment_test(g, ray, t_max, f, ct)) return true;
  }
  return false;
}

// The key of a box for a segment traversal: alive if the ray meets it and its slab interval does not begin behind `bound`
// (t0 of aabb_intercepts, the ray as given, as bvh_closest prunes with it; a negative or NaN t0 or bound culls nothing: never
// less conservative than the closest-hit traversal).  t orders the siblings, the nearer first, as everywhere
__device__ __forceinline__ bool segment_box(const NodeRec& n, const RayS& ray, bool fin, float bound, float& t, float& t0) {
  return aabb_intercepts(xyz(n.lo), xyz(n.hi), ray, t, fin, &t0) && !(t0 > bound);
}

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp) with the records, the slab test and the stack of device_core.hpp.  What differs
// from bvh_any, the reference's feeler:
//   - a child whose box the ray misses, or whose slab interval begins behind t_max, is not visited (segment_box);
//   - a primitive counts only with t < t_max, and the first one that does ends the lane;
//   - a dead end pops the next entry: no restart from the bottom-most entry (Q1), so nothing the ray can reach is skipped.
//     t_max never moves, so a popped entry is not tested again; the float that travels with it is the child's t.
// The boxes are the whole scene's: a filter takes objects out of the leaves, never nodes out of the walk.
template <class Filter, class CT>
struct SegmentAnyWalk {
  const RayS& ray;
  float t_max;
  bool fin;  // slab_fast_path of the ray
  const Filter& f;
  CT& ct;
  __device__ __forceinline__ bool key(const NodeRec& n, float& order, float& stacked) const {
    float t0;
    const bool alive = segment_box(n, ray, fin, t_max, order, t0);
    stacked = order;
    return alive;
  }
  __device__ __forceinline__ bool culled(float) const { return false; }
  __device__ __forceinline__ bool left_first(float l_t, float r_t) const { return l_t < r_t; }
  __device__ __forceinline__ bool leaf(const DevScene& sc, uint32_t s, uint32_t end) {
    bool occluded = false, more = s < end;
    while (more) {
      const Geom g = load_geom(sc.bgeom, s);
      occluded = segment_test(g, ray, t_max, f, ct);
      ++s;
      more = !occluded && s < end;
    }
    return occluded;
  }
};
template <class Filter, class CT>
__device__ bool bvh_segment_any(const DevScene& sc, Stack& st, const RayS& ray, float t_max, const Filter& f, CT& ct) {
  SegmentAnyWalk<Filter, CT> walk{ray, t_max, slab_fast_path<true>(sc, ray), f, ct};
  return bvh_culled_walk(sc, st, walk, ct);
}

struct RayQueryParams {
  DevScene sc;
  uint32_t n;
  const float* origin;     // n x 3
  const float* direction;  // n x 3, used as given
  const float* t_max;      // n, or null: no limit (EXTRAS only)
  int32_t* hit_id;         // closest: required
  float* t;                // closest: optional, like hit_point and normal
  float* hit_point;
  float* normal;           // (EXTRAS only)
  uint8_t* occluded;       // any: required
  QueryStack stack;
};

// One ray per lane on an empty stack: closest_hit / any_hit as the frame kernels call them.  EXTRAS = false is the form of
// the host-array calls: t_max and normal are not read.  EXTRAS = true, the device-buffer calls, gives the same bits where
// they are null, and otherwise: with t_max a closest hit is kept only if t < t_max (strict; a NaN limit keeps nothing), and
// the any-hit is the segment query above (the host refuses it for the grid); normal is get_normal of the hit object at the
// reported hit point, not turned against the ray, zero on a miss.  A compile-time switch, not two null pointers: the normal
// keeps the hit's geometry live through the traversal (grid closest hit: 88 VGPRs and 5 waves against 72 and 7).
// A lane reads its ray with six dword loads 12 bytes apart from its neighbours': a wave's 768 bytes per array are six whole
// 128-byte lines either way, fetched once per ray in front of a traversal of dozens of dependent node fetches, so the rays
// are not staged through LDS with wide loads.  UNMEASURED, like the staged form.
// Two kernels of one name, told apart by their parameters, for the reason nearest_k_device_kernel has two: the ones launched
// without filters hold no filter code.  The filtered one is launched as <accel, ANY = true, EXTRAS = true> with a t_max alone
// (p3d_trace_any_filtered_device): row i of the skip buffers is read once, before the walk, into ten registers.
struct RayQueryFilteredParams {
  RayQueryParams q;
  FilterParams f;
};
template <int ACCEL, bool ANY, bool EXTRAS>
__global__ void __launch_bounds__(kBlock) ray_query_kernel(const RayQueryParams P) {
  const NoFilterSource filters{};
#include "ray_query_body.inc"
}
template <int ACCEL, bool ANY, bool EXTRAS>
__global__ void __launch_bounds__(kBlock) ray_query_kernel(const RayQueryFilteredParams PF) {
  const RayQueryParams& P = PF.q;
  const FilterParams& filters = PF.f;
#include "ray_query_body.inc"
}

}  // namespace p3d
