// nearest_query.hpp — nearest-surface queries over device buffers (p3d_nearest_device): nearest_device_kernel.  Which object's
// surface is nearest to a point, how far, and where on it: the arithmetic is host/nearest_rule.hpp's, shared with
// p3d_host_scene_nearest, whose bits the kernel must give.  Not a ray traversal: children are ordered by the distance of their
// boxes from the point, and the search radius shrinks with every candidate found.  Nothing of device_core.hpp is changed: the
// node and geometry records, the stack and its push / pop are used as they are.
#pragma once

#include "device_core.hpp"
#include "nearest_rule.hpp"

namespace p3d {

// The state of one point's search: the best candidate so far.  `slot` is where its geometry lives (an object index under
// P3D_ACCEL_NONE, a leaf slot under P3D_ACCEL_BVH): it is fetched again for the normal instead of being carried in twelve
// registers through the traversal.
struct NearestBest {
  float d2;
  int32_t object;
  uint32_t slot;
  float q[3];
};

__device__ __forceinline__ void nearest_try(const Geom& g, uint32_t slot, const float p[3], NearestBest& b) {
  const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
  float q[3];
  const float d2 = nearest_point(geom_type(g), v, p, q);
  const int32_t object = (int32_t)geom_object(g);
  if (nearest_wins(d2, object, b.d2, b.object)) {
    b.d2 = d2; b.object = object; b.slot = slot;
    b.q[0] = q[0]; b.q[1] = q[1]; b.q[2] = q[2];
  }
}

__device__ __forceinline__ float nearest_node_d2(const NodeRec& n, const float p[3]) {
  const float lo[3] = {n.lo.x, n.lo.y, n.lo.z}, hi[3] = {n.hi.x, n.hi.y, n.hi.z};
  return nearest_box_d2(p, lo, hi);
}

// P3D_ACCEL_NONE: every object, planes included - the loop of p3d_host_scene_nearest
__device__ void brute_nearest(const DevScene& sc, const float p[3], NearestBest& b) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) nearest_try(load_geom(sc.ogeom, i), i, p, b);
}

// P3D_ACCEL_BVH: a stack traversal over sc.nodes / sc.bgeom.  The float of a stack entry is the child's box d2.
//   - an inner node fetches both children (64 contiguous bytes), visits the nearer one first and pushes the farther one if
//     the cull lets it live;
//   - a popped entry meets the cull again: the radius has shrunk since it was pushed;
//   - a leaf runs the rule on its objects; (d2, object) is a total order, so the order of the visits does not show in the answer;
//   - the cull is nearest_culls, a positive test with slack: a NaN box drops nothing (odd_boxes scenes stay correct).
// A lane pushes at most one entry per step down, so the stack is never deeper than the tree: the bound the host sizes the
// spill area with.  The stack is empty on entry and on exit.
// The steps are taken by wave vote as in bvh_segment_any, not as nested loops: neighbouring lanes hold unrelated points here
// (no pixel coherence), so descents differ in length from lane to lane and the nested form would let the longest hold up every
// lane that stands on a leaf; these scenes are traversed from global memory, where bvh_closest measured the vote ahead.
// UNMEASURED for this traversal; the nested-loop form is the alternative.
__device__ void bvh_nearest(const DevScene& sc, Stack& st, const float p[3], NearestBest& b) {
  constexpr int SPILL = kStackWindow;
  Counters<false> ct;
  const NodeRec root = load_node(sc.nodes, 0);
  if (nearest_culls(nearest_node_d2(root, p), b.d2)) return;
  uint32_t desc = __float_as_uint(root.lo.w);  // a descriptor, or kDescDone
  auto next_entry = [&]() {
    desc = kDescDone;
    bool more = st.sp > 0;
    while (more) {
      const uint2 e = pop<SPILL>(st);
      const bool take = !nearest_culls(__uint_as_float(e.y), b.d2);
      if (take) desc = e.x;
      more = !take && st.sp > 0;
    }
  };
  while (true) {
    const bool on_inner = !(desc & kDescLeaf), on_leaf = !on_inner && desc != kDescDone;
    const unsigned long long m_inner = __ballot(on_inner), m_leaf = __ballot(on_leaf);
    if ((m_inner | m_leaf) == 0) break;
    const bool descend = m_leaf == 0 || __popcll(m_inner) * P3D_VOTE_DEN >= __popcll(m_leaf) * P3D_VOTE_NUM;  // wave-uniform
    if (descend && on_inner) {
      const uint32_t index = desc_index(desc);
      const NodeRec l = load_node(sc.nodes, index), r = load_node(sc.nodes, index + 1);
      const float l_d2 = nearest_node_d2(l, p), r_d2 = nearest_node_d2(r, p);
      const bool l_in = !nearest_culls(l_d2, b.d2), r_in = !nearest_culls(r_d2, b.d2);
      const uint32_t ld = __float_as_uint(l.lo.w), rd = __float_as_uint(r.lo.w);
      if (l_in && r_in) {
        if (r_d2 < l_d2) { desc = rd; push<SPILL>(st, ld, l_d2, ct); }
        else             { desc = ld; push<SPILL>(st, rd, r_d2, ct); }
      } else if (l_in) { desc = ld; }
      else if (r_in)   { desc = rd; }
      else next_entry();
    }
    if (!descend && on_leaf) {
      const uint32_t first = desc_index(desc), end = first + desc_count(desc);
      for (uint32_t s = first; s < end; ++s) nearest_try(load_geom(sc.bgeom, s), s, p, b);
      next_entry();
    }
  }
}

struct NearestParams {
  DevScene sc;
  uint32_t n;
  const float* point;     // n x 3
  const float* max_dist;  // n, or null: no limit
  int32_t* object;        // required
  float* dist;            // optional, like closest and normal
  float* closest;
  float* normal;
  uint2* spill;
  uint32_t spill_stride;
  int32_t stack_cap;
};

// One point per lane on an empty stack bound as in trace_device_kernel.  object = -1, dist = FLT_MAX, closest = normal = 0
// where nothing lies within the limit.  normal: get_normal of the found object at the closest point, not turned.
// A lane reads its point with three dword loads 12 bytes apart from its neighbours' (trace_device_kernel: whole 128-byte
// lines either way, in front of dozens of dependent node fetches).  UNMEASURED, like the staged form.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) nearest_device_kernel(const NearestParams P) {
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  stack_bind(st, smem, 0, threadIdx.x, P.stack_cap, P.spill, P.spill_stride, i);
  if (i >= P.n) return;
  const float p[3] = {P.point[3 * i], P.point[3 * i + 1], P.point[3 * i + 2]};
  NearestBest b;
  b.object = -1; b.slot = 0; b.q[0] = b.q[1] = b.q[2] = 0.0f;
  const bool open = nearest_radius(P.max_dist != nullptr, P.max_dist ? P.max_dist[i] : 0.0f, b.d2);
  if (open && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_nearest(P.sc, st, p, b);
    else brute_nearest(P.sc, p, b);
  }
  const bool found = b.object >= 0;
  P.object[i] = b.object;
  if (P.dist) P.dist[i] = found ? sqrtf(b.d2) : FLT_MAX;
  const F3 q = found ? f3(b.q[0], b.q[1], b.q[2]) : f3(0, 0, 0);
  if (P.closest) {
    P.closest[3 * i] = q.x; P.closest[3 * i + 1] = q.y; P.closest[3 * i + 2] = q.z;
  }
  if (P.normal) {
    F3 nrm = f3(0, 0, 0);
    if (found) nrm = get_normal(load_geom(ACCEL == P3D_ACCEL_BVH ? P.sc.bgeom : P.sc.ogeom, b.slot), P.sc.normals, q);
    P.normal[3 * i] = nrm.x; P.normal[3 * i + 1] = nrm.y; P.normal[3 * i + 2] = nrm.z;
  }
}

}  // namespace p3d
