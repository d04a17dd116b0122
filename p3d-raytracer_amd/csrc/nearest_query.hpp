// nearest_query.hpp — nearest-surface queries over device buffers (p3d_nearest_device, p3d_nearest_k_device): one kernel,
// nearest_k_device_kernel, and one policy of the culled walk, bvh_nearest_k.  For every point the (at most) k objects with the smallest
// (d2, object) under the limit, in that order, how far each is and where on it; p3d_nearest_device is k = 1 without a count.
// The arithmetic, the candidate list, its admission and the bound a node is culled against are host/nearest_rule.hpp's,
// shared with p3d_host_scene_nearest and p3d_host_scene_nearest_k, whose bits the kernel must give.  Not a ray traversal:
// children are ordered by the distance of their boxes from the point, and the search radius shrinks as candidates are found.
// Of device_core.hpp the node and geometry records are used.
#pragma once

#include "nearest_rule.hpp"
#include "queries.hpp"  // QueryStack, bvh_culled_walk, store_f3, query_list_base

namespace p3d {

// The candidate list of one lane.  A list indexed by a runtime position cannot live in registers (it would go to scratch
// memory), so it lives in LDS behind the stack window, strided by lane like the stack: dword f of entry e of a lane at
// [(3 e + f) * kBlock + lane] - a wave's access to one entry's field touches 64 consecutive dwords, no bank conflicts.  An
// entry is d2, the object and the slot of its geometry (an object index under P3D_ACCEL_NONE, a leaf slot under
// P3D_ACCEL_BVH): 12 bytes, 768 k bytes per wave.  The closest point is not kept: it is computed again from the slot at the
// end (nearest_point is evaluated as written in both translation units, so these are the bits the host has).
struct LdsNearestList {
  lds_u32* base;  // &list[lane]
  __device__ __forceinline__ float d2(uint32_t e) const { return __uint_as_float(base[(3 * e) * kBlock]); }
  __device__ __forceinline__ int32_t object(uint32_t e) const { return (int32_t)base[(3 * e + 1) * kBlock]; }
  __device__ __forceinline__ uint32_t slot(uint32_t e) const { return base[(3 * e + 2) * kBlock]; }
  __device__ __forceinline__ void move(uint32_t to, uint32_t from) {
    for (uint32_t f = 0; f < 3; ++f) base[(3 * to + f) * kBlock] = base[(3 * from + f) * kBlock];
  }
  __device__ __forceinline__ void set(uint32_t e, float d2, int32_t object, uint32_t slot) {
    base[(3 * e) * kBlock] = __float_as_uint(d2);
    base[(3 * e + 1) * kBlock] = (uint32_t)object;
    base[(3 * e + 2) * kBlock] = slot;
  }
};
// LDS of one workgroup's lists, in bytes
__host__ __device__ constexpr uint32_t nearest_k_lds_bytes(uint32_t k) { return k * kBlock * 12u; }

// The state of one point's search.  The gate (what a candidate must beat, what a node is culled against) stays in registers:
// LDS is touched only when a candidate is admitted.
struct NearestKSearch {
  LdsNearestList list;
  NearestKGate gate;
  uint32_t count, k;
};

__device__ __forceinline__ float nearest_node_d2(const NodeRec& n, const float p[3]) {
  const float lo[3] = {n.lo.x, n.lo.y, n.lo.z}, hi[3] = {n.hi.x, n.hi.y, n.hi.z};
  return nearest_box_d2(p, lo, hi);
}

// An object the lane's filter names is not offered: the rule is not evaluated for it (filter_rule.hpp).  NoFilter: the test is
// not compiled at all (if constexpr: a test that folds to false still left other instructions in the sweep's kernels)
template <class Filter>
__device__ __forceinline__ void nearest_k_offer(const Geom& g, uint32_t slot, const float p[3], NearestKSearch& s, const Filter& f) {
  if constexpr (Filter::kFilters) {
    if (filter_skips(f, (int32_t)geom_object(g))) return;
  }
  const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
  float q[3];
  const float d2 = nearest_point(geom_type(g), v, p, q);
  const int32_t object = (int32_t)geom_object(g);
  if (nearest_k_admits(d2, object, s.gate)) nearest_k_insert(s.list, s.count, s.k, s.gate, d2, object, slot);
}

// P3D_ACCEL_NONE: every object, planes included - the loop of p3d_host_scene_nearest_k
template <class Filter>
__device__ void brute_nearest_k(const DevScene& sc, const float p[3], NearestKSearch& s, const Filter& f) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) nearest_k_offer(load_geom(sc.ogeom, i), i, p, s, f);
}

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp), not a ray traversal: a box is keyed, ordered and stacked by its d2 from the
// point, the nearer child first (the left one on a tie).
//   - the cull is nearest_culls, a positive test with slack: a NaN box drops nothing (odd_boxes scenes stay correct).  It is
//     taken against s.gate.d2: the squared radius while the list is not full, the k-th entry's d2 once it is.  Until k
//     candidates are in, nothing inside the radius is dropped, so a search is wider than a k = 1 search by what it takes to
//     fill the list;
//   - a popped entry meets the cull again: the radius has shrunk since it was pushed;
//   - a leaf offers each of its objects to the list; (d2, object) is a total order and every object sits in one leaf, so the
//     order of the visits does not show in the list;
//   - a filter changes what a leaf offers and nothing else: the boxes, the cull and its slack are those of the whole scene.  A
//     skipped object tightens no bound, so a filtered search is as wide as the unfiltered search of the scene without it.
template <class Filter>
struct NearestKWalk {
  const float* p;
  NearestKSearch& s;
  const Filter& f;
  __device__ __forceinline__ bool key(const NodeRec& n, float& order, float& stacked) const {
    order = stacked = nearest_node_d2(n, p);
    return !nearest_culls(order, s.gate.d2);
  }
  __device__ __forceinline__ bool culled(float d2) const { return nearest_culls(d2, s.gate.d2); }
  __device__ __forceinline__ bool left_first(float l_d2, float r_d2) const { return !(r_d2 < l_d2); }
  __device__ __forceinline__ bool leaf(const DevScene& sc, uint32_t first, uint32_t end) {
    for (uint32_t g = first; g < end; ++g) nearest_k_offer(load_geom(sc.bgeom, g), g, p, s, f);
    return false;
  }
};
template <class Filter>
__device__ void bvh_nearest_k(const DevScene& sc, Stack& st, const float p[3], NearestKSearch& s, const Filter& f) {
  Counters<false> ct;
  NearestKWalk<Filter> walk{p, s, f};
  bvh_culled_walk(sc, st, walk, ct);
}

struct NearestKParams {
  DevScene sc;
  uint32_t n, k;          // 1 <= k <= P3D_NEAREST_K_MAX
  const float* point;     // n x 3
  const float* max_dist;  // n, or null: no limit
  int32_t* count;         // n, or null: not written (p3d_nearest_device)
  int32_t* object;        // n x k, required
  float* dist;            // n x k; optional, like closest and normal (n x k x 3)
  float* closest;
  float* normal;
  QueryStack stack;
};
// p3d_nearest_k_filtered_device: the same, and where the lanes' filters are
struct NearestKFilteredParams {
  NearestKParams q;
  FilterParams f;
};

// One point per lane on an empty stack; the dynamic LDS holds the stack window and, behind it, the lists of
// the call's k (not of P3D_NEAREST_K_MAX: LDS per workgroup decides how many waves a CU holds).  Row i k + j, j < count: the
// j-th listed object, sqrtf(d2), the closest point (the rule once more at the listed slot) and get_normal of the object
// there, not turned.  Rows j >= count: -1, FLT_MAX, zeros.
// k is a runtime argument.  k as a template parameter over a few sizes would unroll the insertion and fix the LDS offsets; it
// was not tried: UNMEASURED.
// A lane writes its k rows itself: neighbouring lanes are k rows apart, so the stores of one row index are 4 k (object, dist)
// or 12 k (closest, normal) bytes apart and not coalesced.  UNMEASURED; the alternatives are to write row-major through LDS
// (the lists are already there) or to give the outputs the layout (k, n).
// A lane reads its point with three dword loads 12 bytes apart from its neighbours' (ray_query_kernel: whole 128-byte lines
// either way, in front of dozens of dependent node fetches).  UNMEASURED, like the staged form.
// Two kernels of one name, told apart by their parameters: the one p3d_nearest_device and p3d_nearest_k_device launch, which
// knows no filters, and the one of p3d_nearest_k_filtered_device.  A filter costs registers (ten words, and the compares in
// every leaf), which is why the unfiltered calls do not go through the filtered kernel with an empty filter (DESIGN.md
// "Filtered queries" has the compiler's numbers).  The list in LDS next to the candidate lists, read in the leaf, is the
// alternative: not tried, UNMEASURED.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) nearest_k_device_kernel(const NearestKParams P) {
  const NoFilterSource filters{};
#include "nearest_k_body.inc"
}
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) nearest_k_device_kernel(const NearestKFilteredParams PF) {
  const NearestKParams& P = PF.q;
  const FilterParams& filters = PF.f;
#include "nearest_k_body.inc"
}

}  // namespace p3d
