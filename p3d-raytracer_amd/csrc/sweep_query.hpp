// sweep_query.hpp — sphere sweeps over device buffers (p3d_sweep_sphere_device): one kernel, sweep_sphere_device_kernel, and
// one policy of the culled walk, bvh_sweep.  For every moving ball the object it touches first, when, where its centre is
// then and where on the object it touches.  The arithmetic, the key of a node, the cull and the order of two contacts are
// host/sweep_rule.hpp's, shared with p3d_host_scene_sweep_sphere, whose bits the kernel must give.  A ray traversal, but of
// boxes grown by the ball: children are ordered by the ray's entry into them, and the bound shrinks as contacts are found.
// Of device_core.hpp the node and geometry records are used.
#pragma once

#include "queries.hpp"  // QueryStack, bvh_culled_walk, store_f3
#include "sweep_rule.hpp"

namespace p3d {

// The state of one ball's search, all of it in registers: one answer needs no list.  slot: where the best object's geometry
// lives (an object index under P3D_ACCEL_NONE, a leaf slot under P3D_ACCEL_BVH), for the outputs at the end
struct SweepBest {
  float t;         // the best T so far; the limit before there is one: what a node is culled against
  int32_t object;  // kSweepNoObject: none yet
  uint32_t slot;
};

// An object the lane's filter names is not offered: the rule is not evaluated for it (filter_rule.hpp).  NoFilter: the test is
// not compiled at all (if constexpr: a test that folds to false still left other instructions in these kernels)
template <class Filter>
__device__ __forceinline__ void sweep_offer(const Geom& g, uint32_t slot, const SweepRay& s, SweepBest& best, const Filter& f) {
  if constexpr (Filter::kFilters) {
    if (filter_skips(f, (int32_t)geom_object(g))) return;
  }
  const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
  const int32_t object = (int32_t)geom_object(g);
  float t;
  if (sweep_contact(geom_type(g), v, s, t) && sweep_wins(t, object, best.t, best.object)) {
    best.t = t; best.object = object; best.slot = slot;
  }
}

// P3D_ACCEL_NONE: every object, planes included - the loop of p3d_host_scene_sweep_sphere
template <class Filter>
__device__ void brute_sweep(const DevScene& sc, const SweepRay& s, SweepBest& best, const Filter& f) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) sweep_offer(load_geom(sc.ogeom, i), i, s, best, f);
}

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp).  A box is keyed, ordered and stacked by the parameter at which the ray
// enters it once it is grown by the ball (sweep_box_entry: 0 with the origin inside), the nearer child first (the left one
// on a tie).
//   - the grown box contains the Minkowski sum of box and ball, so a ball that misses it touches nothing inside: conservative;
//   - the cull is sweep_culls, a positive test with slack, against best.t: the limit (FLT_MAX without one) until a contact is
//     found, its T from then on.  An entry beyond the best T and one beyond t_max are this one comparison;
//   - a popped entry meets the cull again: the bound has shrunk since it was pushed;
//   - a leaf offers each of its objects and never ends the lane: (T, object) is a total order and every object sits in one
//     leaf, so the order of the visits does not show in the answer;
//   - a filter changes what a leaf offers and nothing else: a skipped object is no contact and shrinks no bound.
template <class Filter>
struct SweepWalk {
  const SweepRay& s;
  const SweepSlabs& slabs;
  SweepBest& best;
  const Filter& f;
  __device__ __forceinline__ bool key(const NodeRec& n, float& order, float& stacked) const {
    const float lo[3] = {n.lo.x, n.lo.y, n.lo.z}, hi[3] = {n.hi.x, n.hi.y, n.hi.z};
    float entry;
    const bool in = sweep_box_entry(s, slabs, lo, hi, entry);
    order = stacked = entry;
    return in && !sweep_culls(entry, best.t);
  }
  __device__ __forceinline__ bool culled(float entry) const { return sweep_culls(entry, best.t); }
  __device__ __forceinline__ bool left_first(float l, float r) const { return !(r < l); }
  __device__ __forceinline__ bool leaf(const DevScene& sc, uint32_t first, uint32_t end) {
    for (uint32_t g = first; g < end; ++g) sweep_offer(load_geom(sc.bgeom, g), g, s, best, f);
    return false;
  }
};
template <class Filter>
__device__ void bvh_sweep(const DevScene& sc, Stack& st, const SweepRay& s, SweepBest& best, const Filter& f) {
  Counters<false> ct;
  SweepSlabs slabs;
  sweep_slabs(s, slabs);
  SweepWalk<Filter> walk{s, slabs, best, f};
  bvh_culled_walk(sc, st, walk, ct);
}

struct SweepParams {
  DevScene sc;
  uint32_t n;
  const float* origin;     // n x 3
  const float* direction;  // n x 3, as given
  const float* radius;     // n
  const float* t_max;      // n, or null: no limit
  int32_t* object;         // n, required
  float* t;                // n; optional, like centre, contact and normal (n x 3)
  float* centre;
  float* contact;
  float* normal;
  QueryStack stack;
};
// p3d_sweep_sphere_filtered_device: the same, and where the lanes' filters are
struct SweepFilteredParams {
  SweepParams q;
  FilterParams f;
};

// One ball per lane on an empty stack; the dynamic LDS holds the stack window only.  Found: the object, T, c(T), the closest
// point of the object at c(T) (nearest_point once more at the kept slot: evaluated as written in both translation units, so
// these are the bits the host has) and get_normal of the object there, not turned.  Not found: -1, FLT_MAX, zeros.
// The triangle rule is long (a face, three edges, three vertices, each with its own square root): the kernel's registers, not
// its LDS, set how many waves a CU holds (DESIGN.md "Sphere sweeps" has the compiler's numbers).  Splitting the walk from the
// primitive tests (collect leaf slots, test them in a second phase) was not tried: UNMEASURED.
// A lane reads its ray with dword loads 12 bytes apart from its neighbours' (ray_query_kernel: whole 128-byte lines either
// way, in front of dozens of dependent node fetches).  UNMEASURED, like the staged form.
// Two kernels of one name, told apart by their parameters: the one p3d_sweep_sphere_device launches, which knows no filters,
// and the one of p3d_sweep_sphere_filtered_device, which holds ten more words per lane through the walk (DESIGN.md "Filtered
// queries" has what that costs in registers).  The list in LDS, read in the leaf, is the alternative: not tried, UNMEASURED.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) sweep_sphere_device_kernel(const SweepParams P) {
  const NoFilterSource filters{};
#include "sweep_body.inc"
}
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) sweep_sphere_device_kernel(const SweepFilteredParams PF) {
  const SweepParams& P = PF.q;
  const FilterParams& filters = PF.f;
#include "sweep_body.inc"
}

}  // namespace p3d
