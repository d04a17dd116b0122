// features.hpp — per-pixel feature buffers (AOVs) of a tile's primary rays: p3d_render_features (include/p3d.h).
//
// One lane per pixel, one wave per 8x8 tile (the tile map of the render kernels, tile_of_block).  Every lane traces the
// primary rays of samples [0, K) of its pixel - the rays the integrators trace: the same RNG stream per (pixel, sample),
// make_primary, and the closest-hit traversal of the configured accel on an empty stack - and averages what the samples
// that hit something saw.  Scene staging, stack mode and LDS size are the ones plan_frame picks for the frame
// (capi_frame_plan.hpp); the kernel has no shading, so it is short and its registers do not limit occupancy.
#pragma once

#include "kernels.hpp"

namespace p3d {

// Counts nothing, like Counters<false>, but a type of its own: the traversal templates instantiated for this kernel are
// then not the ones the render kernels call, and the compiler's inlining of those (bvh_closest is a plain __device__
// template) stays what it was - every existing kernel keeps its instruction stream.
struct FeatureCounters {
  __device__ __forceinline__ void add(int, uint32_t = 1) {}
  __device__ __forceinline__ void stack_depth(int) {}
  __device__ __forceinline__ void clear() {}
  __device__ __forceinline__ uint32_t get(int) const { return 0; }
};

struct FeatureParams {
  float4* normal_depth;  // [pixel] (n.x, n.y, n.z, t): means over the samples whose primary ray hit
  float4* albedo_cov;    // [pixel] (diff_color, hits / K)
  uint32_t samples;      // K
};

// STACK: the node-stack form of the launch (kStackLds6 / kStackLds8 / kStackWindow, device_core.hpp "Stack")
template <int ACCEL, bool LDS, int STACK>
__global__ void __launch_bounds__(kBlock) feature_kernel(const RenderParams P, const FeatureParams F) {
  extern __shared__ float4 smem[];
  uint32_t tx, ty;
  if (!tile_of_block(P, tx, ty)) return;
  DevScene sc = P.sc;
  stage_scene<LDS, ACCEL != P3D_ACCEL_BVH>(sc, P, smem);  // (the BVH traversal reads the BVH-ordered geometry only)
  const uint32_t lane = threadIdx.x;
  Stack st;
  stack_bind(st, smem, P.lds_scene_f4, lane, P.stack_cap, P.spill, P.level_stride, blockIdx.x * kBlock + lane);
  const int c = (int)(tx * 8 + (lane & 7u)), r = (int)(ty * 8 + (lane >> 3));
  if (c >= P.w || r >= P.h) return;
  const int x = P.x0 + c, y = P.y0 + r;  // (no stripes: the host refuses them)
  const int SPP = P.spp_sqrt ? (int)P.spp_sqrt : 1;  // (antialiasing = 0: one sample, SPP unused)
  FeatureCounters ct;
  F3 nsum = f3(0, 0, 0), asum = f3(0, 0, 0);
  float tsum = 0.0f;
  uint32_t hits = 0;
  for (uint32_t s = 0; s < F.samples; ++s) {
    Rng rng;
    if (P.antialiasing) rng.seed_stream(P.seed, (uint32_t)(y * sc.cam.res_x + x), s);
    F3 o, d;
    make_primary(P, sc.cam, x, y, (int)s / SPP, (int)s % SPP, rng, o, d);
    RayS ray;
    ray_set(ray, o, d);
    stack_clear(st);
    F3 Pn;
    Geom g;
    float t = 0.0f;
    const int obj = closest_hit<ACCEL, STACK, !LDS, true>(sc, st, ray, Pn, g, ct, nullptr, &t);
    if (obj < 0) continue;
    const F3 norm = get_normal(g, sc.normals, Pn);                  // main.cpp:366
    const F3 norml = (dot(norm, ray.d) < 0) ? norm : norm * -1.0f;  // main.cpp:368
    nsum = nsum + norml;
    asum = asum + xyz(sc.mats[4 * geom_material(g)]);
    tsum += t;
    ++hits;
  }
  float4 nd = make_float4(0, 0, 0, 0), ac = make_float4(0, 0, 0, 0);
  if (hits) {
    const float fh = (float)hits;
    nd = make_float4(nsum.x / fh, nsum.y / fh, nsum.z / fh, tsum / fh);
    ac = make_float4(asum.x / fh, asum.y / fh, asum.z / fh, fh / (float)F.samples);
  }
  const size_t k = (size_t)r * (size_t)P.w + (size_t)c;
  F.normal_depth[k] = nd;
  F.albedo_cov[k] = ac;
}

}  // namespace p3d
