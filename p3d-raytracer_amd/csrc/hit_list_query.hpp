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

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp) with bvh_segment_any's key of a box, never stopped by a hit.  What differs:
//   - a leaf offers each of its objects to the list; (t, object) is a total order and every object sits in one leaf, so the
//     order of the visits does not show in the answer;
//   - the cull is taken against s.bound(), not a constant.  The bound only shrinks when total is not wanted and the list is full;
//   - so the float of a stack entry is the child's t0, and a popped entry meets the cull again.
template <class CT>
struct SegmentHitsWalk {
  const RayS& ray;
  HitListSearch& s;
  bool fin;  // slab_fast_path of the ray
  CT& ct;
  __device__ __forceinline__ bool key(const NodeRec& n, float& order, float& stacked) const {
    return segment_box(n, ray, fin, s.bound(), order, stacked);
  }
  __device__ __forceinline__ bool culled(float t0) const { return t0 > s.bound(); }
  __device__ __forceinline__ bool left_first(float l_t, float r_t) const { return l_t < r_t; }
  __device__ __forceinline__ bool leaf(const DevScene& sc, uint32_t first, uint32_t end) {
    for (uint32_t g = first; g < end; ++g) hit_list_offer(load_geom(sc.bgeom, g), g, ray, s, ct);
    return false;
  }
};
template <class CT>
__device__ void bvh_segment_hits(const DevScene& sc, Stack& st, const RayS& ray, HitListSearch& s, CT& ct) {
  SegmentHitsWalk<CT> walk{ray, s, slab_fast_path<true>(sc, ray), ct};
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
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) trace_hits_kernel(const TraceHitsParams P) {
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  HitListSearch s;
  s.list.base = query_list_base(smem, P.stack);
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
    if (P.hit_point) store_f3(P.hit_point, row, hp);
    if (P.normal) store_f3(P.normal, row, nrm);
  }
}

}  // namespace p3d
