// overlap_query.hpp — the objects that touch a box, over device buffers (p3d_overlap_box_device): one kernel body,
// overlap_box_device_kernel, and one policy of the culled walk, bvh_overlap_box.  For every closed axis-aligned box lo .. hi
// the number of objects it overlaps and the (at most) k lowest object indices among them, ascending.  The per-object predicate
// and the test of a node's box are host/overlap_rule.hpp's, shared with p3d_host_scene_overlap_box, whose bits the kernel
// must give.  The list is this file's own: k sorted object indices per lane in LDS, 4 bytes an entry (LdsNearestList with a
// constant key would carry a key and a slot nobody reads: 12 bytes an entry and two more moves per shifted entry).
#pragma once

#include "overlap_rule.hpp"
#include "queries.hpp"  // QueryStack, bvh_culled_walk, query_list_base, FilterParams, NoFilterSource

namespace p3d {

// One lane's box, as the kernel holds it
struct QueryBox {
  float lo[3], hi[3];
};

// LDS of one workgroup's lists, in bytes: none for k == 0
__host__ __device__ constexpr uint32_t overlap_lds_bytes(uint32_t k) { return k * kBlock * 4u; }

// The state of one box's search.  The list lives in LDS behind the stack window, strided by lane like the stack: entry e of a
// lane at [e * kBlock + lane], ascending.  The gate stays in registers: what an object must be below to enter - INT32_MAX
// while the list has room (every index is below it), its last entry once it is full, and -1 for k == 0: nothing enters, no
// list is touched, none exists.  LDS is touched only when an object is admitted.
struct OverlapSearch {
  lds_u32* list;  // &list[lane]
  uint32_t count, k, total, flags;
  int32_t gate;
};

// Puts an ADMITTED object where it belongs: the larger entries move one place down, the last one of a full list out
__device__ __forceinline__ void overlap_insert(OverlapSearch& s, int32_t object) {
  uint32_t e = s.count < s.k ? s.count++ : s.k - 1;
  for (; e > 0 && object < (int32_t)s.list[(e - 1) * kBlock]; --e) s.list[e * kBlock] = s.list[(e - 1) * kBlock];
  s.list[e * kBlock] = (uint32_t)object;
  if (s.count == s.k) s.gate = (int32_t)s.list[(s.k - 1) * kBlock];
}

// An object the lane's filter names is neither counted nor listed: the rule is not evaluated for it.  NoFilter: the test is
// not compiled at all (nearest_k_offer has the reason)
template <class Filter>
__device__ __forceinline__ void overlap_offer(const Geom& g, const QueryBox& q, OverlapSearch& s, const Filter& f) {
  const int32_t object = (int32_t)geom_object(g);
  if constexpr (Filter::kFilters) {
    if (filter_skips(f, object)) return;
  }
  const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
  if (overlap_box(geom_type(g), v, q.lo, q.hi, s.flags)) {
    ++s.total;
    if (object < s.gate) overlap_insert(s, object);
  }
}

// P3D_ACCEL_NONE: every object, planes included - the loop of p3d_host_scene_overlap_box
template <class Filter>
__device__ void brute_overlap_box(const DevScene& sc, const QueryBox& q, OverlapSearch& s, const Filter& f) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) overlap_offer(load_geom(sc.ogeom, i), q, s, f);
}

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp) with the simplest policy it has had.  A node is alive unless its box and the
// query box are apart on some axis: comparisons only, no arithmetic and NO SLACK - a true overlap_box implies, by its first
// stage, that the query box overlaps the object's stored box by these same comparisons, and every ancestor's box is a union of
// such boxes by min / max (DESIGN.md "Overlap queries").  The bound never moves: culled() is a constant false, the pop loop
// folds to one pop, and the float of a stack entry is a dead zero.  All hits are counted, so nothing orders the children: the
// left one first.  A leaf offers each unskipped object once; every object sits in one leaf and (object) is a total order, so
// the order of the visits does not show in the list.
template <class Filter>
struct OverlapWalk {
  const QueryBox& q;
  OverlapSearch& s;
  const Filter& f;
  __device__ __forceinline__ bool key(const NodeRec& n, float& order, float& stacked) const {
    const float lo[3] = {n.lo.x, n.lo.y, n.lo.z}, hi[3] = {n.hi.x, n.hi.y, n.hi.z};
    order = stacked = 0.0f;
    return !overlap_boxes_apart(q.lo, q.hi, lo, hi);
  }
  __device__ __forceinline__ bool culled(float) const { return false; }
  __device__ __forceinline__ bool left_first(float, float) const { return true; }
  __device__ __forceinline__ bool leaf(const DevScene& sc, uint32_t first, uint32_t end) {
    for (uint32_t g = first; g < end; ++g) overlap_offer(load_geom(sc.bgeom, g), q, s, f);
    return false;
  }
};
template <class Filter>
__device__ void bvh_overlap_box(const DevScene& sc, Stack& st, const QueryBox& q, OverlapSearch& s, const Filter& f) {
  Counters<false> ct;
  OverlapWalk<Filter> walk{q, s, f};
  bvh_culled_walk(sc, st, walk, ct);
}

struct OverlapParams {
  DevScene sc;
  uint32_t n, k, flags;  // 0 <= k <= P3D_NEAREST_K_MAX; flags: 0 or P3D_OVERLAP_SOLID
  const float* lo;       // n x 3
  const float* hi;       // n x 3
  int32_t* total;        // n, required
  int32_t* object;       // n x k, required with k >= 1; k == 0: neither read nor written
  QueryStack stack;
};
struct OverlapFilteredParams {
  OverlapParams q;
  FilterParams f;
};

// One box per lane on an empty stack; the dynamic LDS holds the stack window and, behind it, the lists of the call's k
// (overlap_lds_bytes; none for k == 0).  Row i k + j, j < min(total, k): the j-th lowest overlapping object; the rows behind: -1.
// A lane writes its k rows itself, at the end, and reads its box with dword loads: the choices of nearest_k_device_kernel,
// UNMEASURED here as there.
// Two kernels of one name, told apart by their parameters, for the reason nearest_k_device_kernel has two: the one launched
// without filters holds no filter code.  The body is text (overlap_body.inc) for the reason nearest_k_body.inc is.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) overlap_box_device_kernel(const OverlapParams P) {
  const NoFilterSource filters{};
#include "overlap_body.inc"
}
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) overlap_box_device_kernel(const OverlapFilteredParams PF) {
  const OverlapParams& P = PF.q;
  const FilterParams& filters = PF.f;
#include "overlap_body.inc"
}

}  // namespace p3d
