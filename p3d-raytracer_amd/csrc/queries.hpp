// queries.hpp — batched per-object queries against a scene, for the unit-level parity of the host classes
// (object_query_kernel), and what the traversing query kernels share: QueryStack, the stack their parameters embed,
// bvh_culled_walk, the one stack traversal with a cull, the output helpers store_f3 and query_list_base, and the two sources
// of a lane's filter, FilterParams and NoFilterSource.
#pragma once

#include "device_core.hpp"
#include "filter_rule.hpp"

namespace p3d {

// Object::intercepts / Object::getNormal / Scene::GetSkyboxColor for batches (host-class forwarding, unit parity)
struct ObjectQueryParams {
  DevScene sc;
  uint32_t object, n;
  const float* a;   // origins | points | directions
  float* b;         // directions (in/out) | normals | rgb
  uint8_t* hit;
  float* t;
};
template <int WHAT>  // 0 intercepts, 1 normal, 2 skybox colour
__global__ void __launch_bounds__(kBlock) object_query_kernel(const ObjectQueryParams P) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= P.n) return;
  Counters<false> ct;
  if (WHAT == 0) {
    const Geom g = load_geom(P.sc.ogeom, P.object);
    RayS ray;
    ray_set(ray, f3(P.a[3 * i], P.a[3 * i + 1], P.a[3 * i + 2]), f3(P.b[3 * i], P.b[3 * i + 1], P.b[3 * i + 2]));
    float t = 0.0f;
    const bool h = intercepts(g, ray, t, ct);
    P.hit[i] = h ? 1 : 0;
    if (h) P.t[i] = t;
    P.b[3 * i] = ray.d.x; P.b[3 * i + 1] = ray.d.y; P.b[3 * i + 2] = ray.d.z;
  } else if (WHAT == 1) {
    const Geom g = load_geom(P.sc.ogeom, P.object);
    const F3 nrm = get_normal(g, P.sc.normals, f3(P.a[3 * i], P.a[3 * i + 1], P.a[3 * i + 2]));
    P.b[3 * i] = nrm.x; P.b[3 * i + 1] = nrm.y; P.b[3 * i + 2] = nrm.z;
  } else {
    const F3 c = skybox_color(P.sc, f3(P.a[3 * i], P.a[3 * i + 1], P.a[3 * i + 2]));
    P.b[3 * i] = c.x; P.b[3 * i + 1] = c.y; P.b[3 * i + 2] = c.z;
  }
}

// The spilling stack of a query kernel that traverses the tree (ray_query.hpp, hit_list_query.hpp, nearest_query.hpp), one
// lane per query: a stack_cap-entry LDS window per lane at the start of the dynamic LDS and, for a tree deeper than the
// window, the lane's column of the scene's spill area.  The host fills it in one place (capi_query.hpp bind_query_stack).
struct QueryStack {
  uint2* spill;
  uint32_t spill_stride;
  int32_t stack_cap;
};
// Lane threadIdx.x's empty stack for query i
__device__ __forceinline__ void query_stack_bind(Stack& st, float4* smem, const QueryStack& q, uint32_t i) {
  stack_bind(st, smem, 0, threadIdx.x, q.stack_cap, q.spill, q.spill_stride, i);
}
// Lane threadIdx.x's column of the candidate lists that lie behind the stack window in the dynamic LDS (nearest_query.hpp
// LdsNearestList)
__device__ __forceinline__ lds_u32* query_list_base(float4* smem, const QueryStack& q) {
  return (lds_u32*)(reinterpret_cast<uint32_t*>(smem + stack_lds_f4(kStackWindow, (uint32_t)q.stack_cap))) + threadIdx.x;
}
// Row `row` of an n x 3 output.  3 * row is taken in the caller's index type: a kernel keeps the address arithmetic it had
template <class Index>
__device__ __forceinline__ void store_f3(float* base, Index row, F3 v) {
  base[3 * row] = v.x; base[3 * row + 1] = v.y; base[3 * row + 2] = v.z;
}

// Where a query kernel's lanes get their filters from (host/filter_rule.hpp): the template argument that tells a filtered
// instantiation from the unfiltered one.  FilterParams: the skip buffers of a *_filtered_device call, row i read once, before
// the walk, into ten registers.  NoFilterSource: nothing is read and filter_skips is a constant false, so the instantiation is
// instruction for instruction the kernel that knows no filters.
struct FilterParams {
  const int32_t* skip;   // n x n_skip, or null
  const int32_t* range;  // n x 2, or null
  uint32_t n_skip;
  __device__ __forceinline__ QueryFilter load(uint32_t i, uint32_t n_objs) const { return filter_load(skip, n_skip, range, i, n_objs); }
};
struct NoFilterSource {
  __device__ __forceinline__ NoFilter load(uint32_t, uint32_t) const { return NoFilter{}; }
};

// The stack traversal over sc.nodes / sc.bgeom of the queries that cull (DESIGN.md "One culled walk"): the segment any-hit
// (ray_query.hpp), the hit list (hit_list_query.hpp) and the k nearest surfaces (nearest_query.hpp).  The walk owns the state
// word, the stepping, the two-child fetch (64 contiguous bytes), "first child now, the other on the stack" and the pop; a
// policy `p`, passed by reference and inlined, says what differs:
//   p.key(node, order, stacked)  whether the node is alive (its box passes the cull), the float that orders it against its
//                                sibling and the float that goes on the stack with it;
//   p.culled(stacked)            whether a popped entry is dead by now (the bound may have shrunk since the push).  A policy
//                                whose bound never moves returns a constant false and the pop loop folds to one pop;
//   p.left_first(l, r)           which of two live children is visited first, from their order floats;
//   p.leaf(sc, first, end)       visits the leaf slots [first, end); true: this lane is finished, the walk returns true for it.
// Every cull is a positive test, so a NaN culls nothing.
// The state of a lane is ONE word as in bvh_closest / bvh_any: the descriptor of the node it stands on, or one of the two end
// states, kDescDone (nothing left; the walk returns false) and kDescHit (a leaf said so; true).  Both have the leaf bit.
// The stack is the caller's and empty on entry; a lane pushes at most one entry per step down, so the stack is never deeper
// than the tree: the bound the host sizes the spill area with (capi_query.hpp bind_query_stack).  It is empty again on exit
// unless a leaf finished the lane, whose entries nobody reads: the query kernel is the only caller and ends there.
// A ray's policy evaluates slab_fast_path once, when it is made: the tests run on copies of the ray, which never changes.
// The steps are taken by wave vote as in bvh_closest (VOTE), not as nested loops: these scenes are traversed from global
// memory, where bvh_closest measured the vote ahead, and neighbouring lanes hold unrelated rays or points (no pixel coherence),
// so descents differ in length and the nested form would let the longest hold up every lane that stands on a leaf.
// UNMEASURED for all three policies; the nested-loop form is the alternative.
template <class Policy, class CT>
__device__ __forceinline__ bool bvh_culled_walk(const DevScene& sc, Stack& st, Policy& p, CT& ct) {
  constexpr int SPILL = kStackWindow;
  float order, stacked;
  const NodeRec root = load_node(sc.nodes, 0);
  ct.add(kNodeTests);
  if (!p.key(root, order, stacked)) return false;
  uint32_t desc = __float_as_uint(root.lo.w);
  auto next_entry = [&]() {
    desc = kDescDone;
    bool more = st.sp > 0;
    while (more) {
      const uint2 e = pop<SPILL>(st);
      const bool take = !p.culled(__uint_as_float(e.y));
      if (take) desc = e.x;
      more = !take && st.sp > 0;
    }
  };
  while (true) {
    const bool on_inner = !(desc & kDescLeaf), on_leaf = !on_inner && desc < kDescHit;
    const unsigned long long m_inner = __ballot(on_inner), m_leaf = __ballot(on_leaf);
    if ((m_inner | m_leaf) == 0) break;
    const bool descend = m_leaf == 0 || __popcll(m_inner) * P3D_VOTE_DEN >= __popcll(m_leaf) * P3D_VOTE_NUM;  // wave-uniform
    if (descend && on_inner) {
      const uint32_t index = desc_index(desc);
      const NodeRec l = load_node(sc.nodes, index), r = load_node(sc.nodes, index + 1);
      float l_order, r_order, l_stacked, r_stacked;
      ct.add(kNodeTests, 2);
      const bool l_in = p.key(l, l_order, l_stacked), r_in = p.key(r, r_order, r_stacked);
      const uint32_t ld = __float_as_uint(l.lo.w), rd = __float_as_uint(r.lo.w);
      if (l_in && r_in) {
        if (p.left_first(l_order, r_order)) { desc = ld; push<SPILL>(st, rd, r_stacked, ct); }
        else                                { desc = rd; push<SPILL>(st, ld, l_stacked, ct); }
      } else if (l_in) { desc = ld; }
      else if (r_in)   { desc = rd; }
      else next_entry();
    }
    if (!descend && on_leaf) {
      const uint32_t first = desc_index(desc);
      if (p.leaf(sc, first, first + desc_count(desc))) desc = kDescHit;
      else next_entry();
    }
  }
  return desc == kDescHit;
}

}  // namespace p3d
