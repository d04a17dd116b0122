// hit_list_query.hpp — the hits along a ray in order, over device buffers (p3d_trace_hits_device): one kernel,
// trace_hits_kernel, and one traversal, bvh_segment_hits.  For every ray the (at most) k objects with the smallest
// (t, object) among those its segment hits, in that order, and the number of all of them: the ray-side twin of
// nearest_k_device_kernel.  The per-object predicate is ray_query.hpp's segment test (a fresh copy of the ray per test), the
// candidate list, its admission and its LDS storage are the nearest-k query's (host/nearest_rule.hpp NearestKGate and
// nearest_k_insert, nearest_query.hpp LdsNearestList) with t in the place of d2: `d2` is the name of the list's KEY there.
// Of device_core.hpp the node and geometry records, the slab test, the stack and its push / pop are used.
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
// the gate is (limit, -1) and admission is t < limit once more; a NaN t passes neither comparison
template <class CT>
__device__ __forceinline__ void hit_list_offer(const Geom& g, uint32_t slot, const RayS& ray, HitListSearch& s, CT& ct) {
  RayS r = ray;
  float t;
  if (intercepts(g, r, t, ct) && t < s.limit) {
    ++s.total;
    const int32_t object = (int32_t)geom_object(g);
    if (nearest_k_admits(t, object, s.gate)) nearest_k_insert(s.list, s.count, s.k, s.gate, t, object, slot);
  }
}

// P3D_ACCEL_NONE: every object, planes included
template <class CT>
__device__ void brute_segment_hits(const DevScene& sc, const RayS& ray, HitListSearch& s, CT& ct) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) hit_list_offer(load_geom(sc.ogeom, i), i, ray, s, ct);
}

// P3D_ACCEL_BVH: bvh_segment_any's traversal - its records, slab test, push / pop and wave-vote stepping - that never stops at
// a hit.  What differs:
//   - a leaf offers each of its objects to the list; (t, object) is a total order and every object sits in one leaf, so the
//     order of the visits does not show in the answer;
//   - a child is skipped if the ray misses its box or its slab interval begins behind s.bound() (a positive test: a NaN t0
//     or bound culls nothing).  The bound only shrinks when total is not wanted and the list is full;
//   - the float of a stack entry is the child's t0, and a popped entry meets the cull again: the bound may have shrunk since
//     the push;
//   - the nearer child (by the slab test's t, as everywhere) goes first.
// A lane pushes at most one entry per step down, so the stack is never deeper than the tree: the bound the host sizes the
// spill area with.  The stack is empty on entry and on exit.
// The steps are taken by wave vote as in bvh_segment_any; UNMEASURED for this traversal, the nested-loop form is the
// alternative.
template <class CT>
__device__ void bvh_segment_hits(const DevScene& sc, Stack& st, const RayS& ray, HitListSearch& s, CT& ct) {
  constexpr int SPILL = kStackWindow;
  // (the ray never changes here - the tests run on copies - so one answer holds for the whole traversal)
  const bool fin = slab_fast_path<true>(sc, ray);
  float tmp, t0;
  const NodeRec root = load_node(sc.nodes, 0);
  ct.add(kNodeTests);
  if (!aabb_intercepts(xyz(root.lo), xyz(root.hi), ray, tmp, fin, &t0) || t0 > s.bound()) return;
  uint32_t desc = __float_as_uint(root.lo.w);  // a descriptor, or kDescDone
  auto next_entry = [&]() {
    desc = kDescDone;
    bool more = st.sp > 0;
    while (more) {
      const uint2 e = pop<SPILL>(st);
      const bool take = !(__uint_as_float(e.y) > s.bound());
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
      float l_t, r_t, l_t0, r_t0;
      ct.add(kNodeTests, 2);
      const float bound = s.bound();
      const bool l_hit = aabb_intercepts(xyz(l.lo), xyz(l.hi), ray, l_t, fin, &l_t0) && !(l_t0 > bound);
      const bool r_hit = aabb_intercepts(xyz(r.lo), xyz(r.hi), ray, r_t, fin, &r_t0) && !(r_t0 > bound);
      const uint32_t ld = __float_as_uint(l.lo.w), rd = __float_as_uint(r.lo.w);
      if (l_hit && r_hit) {
        if (l_t < r_t) { desc = ld; push<SPILL>(st, rd, r_t0, ct); }
        else           { desc = rd; push<SPILL>(st, ld, l_t0, ct); }
      } else if (l_hit) { desc = ld; }
      else if (r_hit)   { desc = rd; }
      else next_entry();
    }
    if (!descend && on_leaf) {
      const uint32_t first = desc_index(desc), end = first + desc_count(desc);
      for (uint32_t g = first; g < end; ++g) hit_list_offer(load_geom(sc.bgeom, g), g, ray, s, ct);
      next_entry();
    }
  }
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
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) trace_hits_kernel(const TraceHitsParams P) {
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  HitListSearch s;
  s.list.base = (lds_u32*)(reinterpret_cast<uint32_t*>(smem + stack_lds_f4(kStackWindow, (uint32_t)P.stack.stack_cap))) + threadIdx.x;
  s.k = P.k; s.want_total = P.total != nullptr;
  if (i >= P.n) return;
  Counters<false> ct;
  RayS ray;
  ray_set(ray, f3(P.origin[3 * i], P.origin[3 * i + 1], P.origin[3 * i + 2]),
          f3(P.direction[3 * i], P.direction[3 * i + 1], P.direction[3 * i + 2]));
  if (hit_list_open(P.t_max, i, s) && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_segment_hits(P.sc, st, ray, s, ct);
    else brute_segment_hits(P.sc, ray, s, ct);
  }
  if (P.total) P.total[i] = (int32_t)s.total;
  if (P.k == 0) return;
  P.count[i] = (int32_t)s.count;
  const float4* geom = ACCEL == P3D_ACCEL_BVH ? P.sc.bgeom : P.sc.ogeom;
  for (uint32_t e = 0; e < P.k; ++e) {
    const size_t row = (size_t)i * P.k + e;
    int32_t object = -1;
    float t = FLT_MAX;
    F3 hp = f3(0, 0, 0), nrm = f3(0, 0, 0);
    if (e < s.count) {
      object = s.list.object(e);
      t = s.list.d2(e);
      if (P.hit_point || P.normal) {
        const Geom g = load_geom(geom, s.list.slot(e));
        RayS r = ray;
        float again;
        intercepts(g, r, again, ct);  // (for the ray it leaves behind: a sphere has normalised it, Q8)
        hp = r.o + r.d * t;
        if (P.normal) nrm = get_normal(g, P.sc.normals, hp);
      }
    }
    P.object[row] = object;
    if (P.t) P.t[row] = t;
    if (P.hit_point) {
      P.hit_point[3 * row] = hp.x; P.hit_point[3 * row + 1] = hp.y; P.hit_point[3 * row + 2] = hp.z;
    }
    if (P.normal) {
      P.normal[3 * row] = nrm.x; P.normal[3 * row + 1] = nrm.y; P.normal[3 * row + 2] = nrm.z;
    }
  }
}

}  // namespace p3d
