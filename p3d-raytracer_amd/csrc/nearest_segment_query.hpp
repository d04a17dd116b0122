// nearest_segment_query.hpp — nearest surfaces to a segment over device buffers (p3d_nearest_segment_k_device): one kernel body,
// nearest_segment_k_device_kernel, and one policy of the culled walk, bvh_nearest_segment_k.  For every segment a b the (at
// most) k objects with the smallest (d2, object) under the limit, in that order; how far each is, where on the segment and
// where on the object.  The per-object arithmetic and the key of a node are host/nearest_segment_rule.hpp's, shared with
// p3d_host_scene_nearest_segment_k, whose bits the kernel must give; the candidate list, its admission, the gate and the cull
// are the point query's (host/nearest_rule.hpp, nearest_query.hpp: LdsNearestList, NearestKSearch), unchanged.
#pragma once

#include "nearest_query.hpp"  // LdsNearestList, NearestKSearch, nearest_k_lds_bytes
#include "nearest_segment_rule.hpp"

namespace p3d {

// One lane's segment, as the kernel holds it
struct QuerySegment {
  float a[3], b[3];
};

__device__ __forceinline__ float nearest_segment_node_d2(const NodeRec& n, const QuerySegment& g) {
  const float lo[3] = {n.lo.x, n.lo.y, n.lo.z}, hi[3] = {n.hi.x, n.hi.y, n.hi.z};
  return segment_box_d2(g.a, g.b, lo, hi);
}

// As nearest_k_offer: an object the lane's filter names is not offered, and without filters the test is not compiled.  Of the
// rule only d2 is used here: s, x and q are dead and the compiler drops what only they need.  The rows are made at the end,
// by the rule once more at the listed slot
template <class Filter>
__device__ __forceinline__ void nearest_segment_k_offer(const Geom& g, uint32_t slot, const QuerySegment& seg, NearestKSearch& s, const Filter& f) {
  if constexpr (Filter::kFilters) {
    if (filter_skips(f, (int32_t)geom_object(g))) return;
  }
  const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
  float param, x[3], q[3];
  const float d2 = segment_nearest(geom_type(g), v, seg.a, seg.b, param, x, q);
  const int32_t object = (int32_t)geom_object(g);
  if (nearest_k_admits(d2, object, s.gate)) nearest_k_insert(s.list, s.count, s.k, s.gate, d2, object, slot);
}

// P3D_ACCEL_NONE: every object, planes included - the loop of p3d_host_scene_nearest_segment_k
template <class Filter>
__device__ void brute_nearest_segment_k(const DevScene& sc, const QuerySegment& seg, NearestKSearch& s, const Filter& f) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) nearest_segment_k_offer(load_geom(sc.ogeom, i), i, seg, s, f);
}

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp) under NearestKWalk's policy with another key: a box is keyed, ordered and
// stacked by segment_box_d2, a lower bound of the d2 of anything inside it (the rule header has the argument); the nearer
// child first, the left one on a tie; the cull is nearest_culls against s.gate.d2, a positive test with the point query's
// slack, and a popped entry meets it again; a leaf offers each unskipped object once.  (d2, object) is a total order and every
// object sits in one leaf, so the order of the visits does not show in the list; a filter changes what a leaf offers and
// nothing else.
template <class Filter>
struct NearestSegmentKWalk {
  const QuerySegment& seg;
  NearestKSearch& s;
  const Filter& f;
  __device__ __forceinline__ bool key(const NodeRec& n, float& order, float& stacked) const {
    order = stacked = nearest_segment_node_d2(n, seg);
    return !nearest_culls(order, s.gate.d2);
  }
  __device__ __forceinline__ bool culled(float d2) const { return nearest_culls(d2, s.gate.d2); }
  __device__ __forceinline__ bool left_first(float l_d2, float r_d2) const { return !(r_d2 < l_d2); }
  __device__ __forceinline__ bool leaf(const DevScene& sc, uint32_t first, uint32_t end) {
    for (uint32_t g = first; g < end; ++g) nearest_segment_k_offer(load_geom(sc.bgeom, g), g, seg, s, f);
    return false;
  }
};
template <class Filter>
__device__ void bvh_nearest_segment_k(const DevScene& sc, Stack& st, const QuerySegment& seg, NearestKSearch& s, const Filter& f) {
  Counters<false> ct;
  NearestSegmentKWalk<Filter> walk{seg, s, f};
  bvh_culled_walk(sc, st, walk, ct);
}

struct NearestSegmentParams {
  DevScene sc;
  uint32_t n, k;          // 1 <= k <= P3D_NEAREST_K_MAX
  const float* a;         // n x 3
  const float* b;         // n x 3
  const float* max_dist;  // n, or null: no limit
  int32_t* count;         // n
  int32_t* object;        // n x k, required
  float* dist;            // n x k; optional, like param (n x k) and on_segment, closest and normal (n x k x 3)
  float* param;
  float* on_segment;
  float* closest;
  float* normal;
  QueryStack stack;
};
struct NearestSegmentFilteredParams {
  NearestSegmentParams q;
  FilterParams f;
};

// One segment per lane on an empty stack; the dynamic LDS holds the stack window and, behind it, the lists of the call's k
// (nearest_k_lds_bytes), as in nearest_k_device_kernel; the gate stays in registers.  Row i k + j, j < count: the j-th listed
// object, sqrtf(d2), and s, x, q of the rule once more at the listed slot, get_normal of the object at q, not turned.  Rows
// j >= count: -1, FLT_MAX, zeros.
// Two kernels of one name, told apart by their parameters, for the reason nearest_k_device_kernel has two: the one launched
// without filters holds no filter code.  The body is text (nearest_segment_body.inc) for the reason nearest_k_body.inc is.
// The rule is several times the point rule (five candidates for a triangle, two square roots and a division for a sphere):
// a leaf costs more here, a node the same.  The row stores are a lane's own, k rows apart, as there: UNMEASURED alike.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) nearest_segment_k_device_kernel(const NearestSegmentParams P) {
  const NoFilterSource filters{};
#include "nearest_segment_body.inc"
}
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) nearest_segment_k_device_kernel(const NearestSegmentFilteredParams PF) {
  const NearestSegmentParams& P = PF.q;
  const FilterParams& filters = PF.f;
#include "nearest_segment_body.inc"
}

}  // namespace p3d
