// ray_query.hpp — the batched ray queries, from host arrays (p3d_trace_closest, p3d_trace_any) and over device buffers
// (p3d_trace_closest_device, p3d_trace_any_device): ray_query_kernel, one body for both, and bvh_segment_any, the any-hit
// with a distance limit.  The unlimited paths call device_core.hpp's closest_hit / any_hit (bvh.cpp:198-340,
// grid.cpp:71-208, main.cpp:116-124,208-216), the segment query has a traversal of its own.
#pragma once

#include "queries.hpp"  // QueryStack

namespace p3d {

// The segment query (DESIGN.md "Segment occlusion"):
//   occluded = some object j has intercepts(object j, a fresh copy of the ray, t) true and t < t_max.
// Every primitive is tested on a copy of the caller's ray, so a sphere test's re-normalisation (Q8) never reaches a later
// test and the answer does not depend on the order of the visits.  A NaN t (A10) and a NaN t_max keep nothing.
template <class CT>
__device__ __forceinline__ bool segment_test(const Geom& g, const RayS& ray, float t_max, CT& ct) {
  RayS r = ray;
  float t;
  return intercepts(g, r, t, ct) && t < t_max;
}

// P3D_ACCEL_NONE: every object
template <class CT>
__device__ bool brute_segment_any(const DevScene& sc, const RayS& ray, float t_max, CT& ct) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) {
    const Geom g = load_geom(sc.ogeom, i);
    if (segment_test(g, ray, t_max, ct)) return true;
  }
  return false;
}

// P3D_ACCEL_BVH: a stack traversal over sc.nodes / sc.bgeom with the records, the slab test and the stack of device_core.hpp.
// What differs from bvh_any, the reference's feeler:
//   - a child whose box the ray misses, or whose slab interval begins behind t_max, is not visited (t0 of aabb_intercepts, the
//     ray as given, as bvh_closest prunes with it; a negative or NaN t0 culls nothing: never less conservative than the
//     closest-hit traversal);
//   - a primitive counts only with t < t_max;
//   - a dead end pops the next entry: no restart from the bottom-most entry (Q1), so nothing the ray can reach is skipped.
// The nearer child is visited first.  The stack is the caller's, empty on entry; a hit leaves its entries behind, which
// nobody reads: the query kernel is the only caller and ends there.
// The steps are taken by wave vote as in bvh_closest (VOTE): these scenes are traversed from global memory.  That choice
// is UNMEASURED for this traversal; the nested-loop form is the alternative.
template <class CT>
__device__ bool bvh_segment_any(const DevScene& sc, Stack& st, const RayS& ray, float t_max, CT& ct) {
  constexpr int SPILL = kStackWindow;
  // (the ray never changes here - the tests run on copies - so one answer holds for the whole traversal; lanes only leave)
  const bool fin = slab_fast_path<true>(sc, ray);
  float tmp, t0;
  const NodeRec root = load_node(sc.nodes, 0);
  ct.add(kNodeTests);
  if (!aabb_intercepts(xyz(root.lo), xyz(root.hi), ray, tmp, fin, &t0) || t0 > t_max) return false;
  // state word as in bvh_any: a descriptor, kDescDone or kDescHit
  uint32_t desc = __float_as_uint(root.lo.w);
  auto next_entry = [&]() { desc = st.sp > 0 ? pop<SPILL>(st).x : kDescDone; };
  while (true) {
    const bool on_inner = !(desc & kDescLeaf), on_leaf = !on_inner && desc < kDescHit;
    const unsigned long long m_inner = __ballot(on_inner), m_leaf = __ballot(on_leaf);
    if ((m_inner | m_leaf) == 0) break;
    const bool descend = m_leaf == 0 || __popcll(m_inner) * P3D_VOTE_DEN >= __popcll(m_leaf) * P3D_VOTE_NUM;  // wave-uniform
    if (descend && on_inner) {
      const uint32_t index = desc_index(desc);
      const NodeRec l = load_node(sc.nodes, index), r = load_node(sc.nodes, index + 1);
      float l_t, r_t, l_t0, r_t0;
      ct.add(kNodeTests, 2);
      const bool l_hit = aabb_intercepts(xyz(l.lo), xyz(l.hi), ray, l_t, fin, &l_t0) && !(l_t0 > t_max);
      const bool r_hit = aabb_intercepts(xyz(r.lo), xyz(r.hi), ray, r_t, fin, &r_t0) && !(r_t0 > t_max);
      const uint32_t ld = __float_as_uint(l.lo.w), rd = __float_as_uint(r.lo.w);
      if (l_hit && r_hit) {
        if (l_t < r_t) { desc = ld; push<SPILL>(st, rd, r_t, ct); }
        else           { desc = rd; push<SPILL>(st, ld, l_t, ct); }
      } else if (l_hit) { desc = ld; }
      else if (r_hit)   { desc = rd; }
      else next_entry();
    }
    if (!descend && on_leaf) {
      uint32_t s = desc_index(desc);
      const uint32_t end = s + desc_count(desc);
      bool occluded = false, more = s < end;
      while (more) {
        const Geom g = load_geom(sc.bgeom, s);
        occluded = segment_test(g, ray, t_max, ct);
        ++s;
        more = !occluded && s < end;
      }
      if (occluded) desc = kDescHit;
      else next_entry();
    }
  }
  return desc == kDescHit;
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
template <int ACCEL, bool ANY, bool EXTRAS>
__global__ void __launch_bounds__(kBlock) ray_query_kernel(const RayQueryParams P) {
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  if (i >= P.n) return;
  Counters<false> ct;
  RayS ray;
  ray_set(ray, f3(P.origin[3 * i], P.origin[3 * i + 1], P.origin[3 * i + 2]),
          f3(P.direction[3 * i], P.direction[3 * i + 1], P.direction[3 * i + 2]));
  const float* t_max = EXTRAS ? P.t_max : nullptr;
  if (ANY) {
    bool occluded;
    if (!t_max) occluded = any_hit<ACCEL, true, true>(P.sc, st, ray, ct);
    else if (ACCEL == P3D_ACCEL_BVH) occluded = bvh_segment_any(P.sc, st, ray, t_max[i], ct);
    else occluded = brute_segment_any(P.sc, ray, t_max[i], ct);
    P.occluded[i] = occluded ? 1 : 0;
  } else {
    F3 hp = f3(0, 0, 0);
    Geom g;
    float t = FLT_MAX;
    int obj = closest_hit<ACCEL, true, true>(P.sc, st, ray, hp, g, ct, nullptr, &t);
    if (t_max && obj >= 0 && !(t < t_max[i])) obj = -1;
    P.hit_id[i] = obj;
    if (P.t) P.t[i] = obj < 0 ? FLT_MAX : t;
    if (obj < 0) hp = f3(0, 0, 0);
    if (P.hit_point) {
      P.hit_point[3 * i] = hp.x; P.hit_point[3 * i + 1] = hp.y; P.hit_point[3 * i + 2] = hp.z;
    }
    if (EXTRAS && P.normal) {
      const F3 nrm = obj < 0 ? f3(0, 0, 0) : get_normal(g, P.sc.normals, hp);
      P.normal[3 * i] = nrm.x; P.normal[3 * i + 1] = nrm.y; P.normal[3 * i + 2] = nrm.z;
    }
  }
}

}  // namespace p3d
