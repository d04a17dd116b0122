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

__device__ __forceinline__ void sweep_offer(const Geom& g, uint32_t slot, const SweepRay& s, SweepBest& best) {
  const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
  const int32_t object = (int32_t)geom_object(g);
  float t;
  if (sweep_contact(geom_type(g), v, s, t) && sweep_wins(t, object, best.t, best.object)) {
    best.t = t; best.object = object; best.slot = slot;
  }
}

// P3D_ACCEL_NONE: every object, planes included - the loop of p3d_host_scene_sweep_sphere
__device__ void brute_sweep(const DevScene& sc, const SweepRay& s, SweepBest& best) {
  for (uint32_t i = 0; i < sc.n_objs; ++i) sweep_offer(load_geom(sc.ogeom, i), i, s, best);
}

// P3D_ACCEL_BVH: bvh_culled_walk (queries.hpp).  A box is keyed, ordered and stacked by the parameter at which the ray
// enters it once it is grown by the ball (sweep_box_entry: 0 with the origin inside), the nearer child first (the left one
// on a tie).
//   - the grown box contains the Minkowski sum of box and ball, so a ball that misses it touches nothing inside: conservative;
//   - the cull is sweep_culls, a positive test with slack, against best.t: the limit (FLT_MAX without one) until a contact is
//     found, its T from then on.  An entry beyond the best T and one beyond t_max are this one comparison;
//   - a popped entry meets the cull again: the bound has shrunk since it was pushed;
//   - a leaf offers each of its objects and never ends the lane: (T, object) is a total order and every object sits in one
//     leaf, so the order of the visits does not show in the answer.
struct SweepWalk {
  const SweepRay& s;
  const SweepSlabs& slabs;
  SweepBest& best;
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
    for (uint32_t g = first; g < end; ++g) sweep_offer(load_geom(sc.bgeom, g), g, s, best);
    return false;
  }
};
__device__ void bvh_sweep(const DevScene& sc, Stack& st, const SweepRay& s, SweepBest& best) {
  Counters<false> ct;
  SweepSlabs slabs;
  sweep_slabs(s, slabs);
  SweepWalk walk{s, slabs, best};
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

// One ball per lane on an empty stack; the dynamic LDS holds the stack window only.  Found: the object, T, c(T), the closest
// point of the object at c(T) (nearest_point once more at the kept slot: evaluated as written in both translation units, so
// these are the bits the host has) and get_normal of the object there, not turned.  Not found: -1, FLT_MAX, zeros.
// The triangle rule is long (a face, three edges, three vertices, each with its own square root): the kernel's registers, not
// its LDS, set how many waves a CU holds (DESIGN.md "Sphere sweeps" has the compiler's numbers).  Splitting the walk from the
// primitive tests (collect leaf slots, test them in a second phase) was not tried: UNMEASURED.
// A lane reads its ray with dword loads 12 bytes apart from its neighbours' (ray_query_kernel: whole 128-byte lines either
// way, in front of dozens of dependent node fetches).  UNMEASURED, like the staged form.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) sweep_sphere_device_kernel(const SweepParams P) {
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, i);
  if (i >= P.n) return;
  const size_t row = i;  // (3 * row in 64 bits)
  const float o[3] = {P.origin[3 * row], P.origin[3 * row + 1], P.origin[3 * row + 2]};
  const float d[3] = {P.direction[3 * row], P.direction[3 * row + 1], P.direction[3 * row + 2]};
  SweepRay s;
  sweep_ray(o, d, P.radius[i], P.t_max != nullptr, P.t_max ? P.t_max[i] : 0.0f, s);
  SweepBest best{s.limit, kSweepNoObject, 0u};
  if (s.ok && P.sc.n_objs > 0) {
    if (ACCEL == P3D_ACCEL_BVH) bvh_sweep(P.sc, st, s, best);
    else brute_sweep(P.sc, s, best);
  }
  const bool found = best.object != kSweepNoObject;
  int32_t object = -1;
  float t = FLT_MAX;
  F3 c = f3(0, 0, 0), q = f3(0, 0, 0), nrm = f3(0, 0, 0);
  if (found) {
    const Geom g = load_geom(ACCEL == P3D_ACCEL_BVH ? P.sc.bgeom : P.sc.ogeom, best.slot);
    const float v[9] = {g.a.x, g.a.y, g.a.z, g.a.w, g.b.x, g.b.y, g.b.z, g.b.w, g.c.x};
    float cc[3], qq[3];
    sweep_centre(s, best.t, cc);
    nearest_point(geom_type(g), v, cc, qq);
    object = best.object;
    t = best.t;
    c = f3(cc[0], cc[1], cc[2]);
    q = f3(qq[0], qq[1], qq[2]);
    if (P.normal) nrm = get_normal(g, P.sc.normals, q);
  }
  P.object[i] = object;
  if (P.t) P.t[i] = t;
  if (P.centre) store_f3(P.centre, row, c);
  if (P.contact) store_f3(P.contact, row, q);
  if (P.normal) store_f3(P.normal, row, nrm);
}

}  // namespace p3d
