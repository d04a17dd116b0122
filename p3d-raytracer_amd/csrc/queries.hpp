// queries.hpp — batched per-object queries against a scene, for the unit-level parity of the host classes
// (object_query_kernel), and QueryStack, the stack every traversing query kernel's parameters embed.
#pragma once

#include "device_core.hpp"

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

// The spilling stack of a query kernel that traverses the tree (ray_query.hpp, nearest_query.hpp), one lane per query: a
// stack_cap-entry LDS window per lane at the start of the dynamic LDS and, for a tree deeper than the window, the lane's
// column of the scene's spill area.  The host fills it in one place (capi_query.hpp bind_query_stack).
struct QueryStack {
  uint2* spill;
  uint32_t spill_stride;
  int32_t stack_cap;
};
// Lane threadIdx.x's empty stack for query i
__device__ __forceinline__ void query_stack_bind(Stack& st, float4* smem, const QueryStack& q, uint32_t i) {
  stack_bind(st, smem, 0, threadIdx.x, q.stack_cap, q.spill, q.spill_stride, i);
}

}  // namespace p3d
