// queries.hpp — batched queries against a scene, for the unit-level parity of the traversal back ends and of the host
// classes: trace_kernel (bvh.cpp:198-340, grid.cpp:71-208, main.cpp:116-124,208-216) and object_query_kernel.
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

struct TraceParams {
  DevScene sc;
  uint32_t n;
  const float* origin;
  const float* direction;
  int32_t* hit_id;
  float* t;
  float* hit_point;
  uint8_t* occluded;
  uint2* spill;
  uint32_t spill_stride;
  int32_t stack_cap;
};

template <int ACCEL, bool ANY>
__global__ void __launch_bounds__(kBlock) trace_kernel(const TraceParams P) {
  extern __shared__ float4 smem[];
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  stack_bind(st, smem, 0, threadIdx.x, P.stack_cap, P.spill, P.spill_stride, i);
  if (i >= P.n) return;
  Counters<false> ct;
  RayS ray;
  ray_set(ray, f3(P.origin[3 * i], P.origin[3 * i + 1], P.origin[3 * i + 2]),
          f3(P.direction[3 * i], P.direction[3 * i + 1], P.direction[3 * i + 2]));
  if (ANY) {
    P.occluded[i] = any_hit<ACCEL, true, true>(P.sc, st, ray, ct) ? 1 : 0;
  } else {
    F3 hp = f3(0, 0, 0);
    Geom g;
    float t = FLT_MAX;
    const int obj = closest_hit<ACCEL, true, true>(P.sc, st, ray, hp, g, ct, nullptr, &t);
    P.hit_id[i] = obj;
    if (P.t) P.t[i] = obj < 0 ? FLT_MAX : t;
    if (obj < 0) hp = f3(0, 0, 0);
    if (P.hit_point) {
      P.hit_point[3 * i] = hp.x; P.hit_point[3 * i + 1] = hp.y; P.hit_point[3 * i + 2] = hp.z;
    }
  }
}

}  // namespace p3d
