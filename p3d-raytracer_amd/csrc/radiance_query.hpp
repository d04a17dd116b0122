// radiance_query.hpp — what a ray sees, for rays in device memory (p3d_trace_radiance_device), and the rays of a camera
// (p3d_camera_rays_device).  radiance_query_kernel is rayTracing (main.cpp:92-309) for a ray that is nobody's pixel: the
// chain loop and the bottom-up fold of whitted_sample.inc spelled around whitted_level.inc, as wf_level_kernel spells one
// level of it, on the stack of the ray queries (queries.hpp QueryStack).  camera_rays_kernel is camera.h:65-82 for the pixel
// centres of a tile.  Uses the stripe rows of handoff_kernels.hpp (through kernels.hpp) and the level body.
#pragma once

#include "kernels.hpp"
#include "queries.hpp"  // QueryStack, query_stack_bind, store_f3

namespace p3d {

// One record {local colour, child weight} per level and lane, in dynamic LDS behind the stack window, the lane the fastest
// index: level l of lane t at [l * kBlock + t], 16 bytes each.  A wave's ds_write_b128 / ds_read_b128 of one level touches
// 1 KB of consecutive bytes (every 8-lane group of the store 32 banks, every 16-lane group of the load 64: no bank conflict),
// once per level each.  A record array indexed by a runtime level cannot live in registers; in LDS it needs no global
// scratch, so the call allocates nothing.  P3D_RADIANCE_MAX_DEPTH levels: 16 KB next to the 8 KB window.
typedef float __attribute__((ext_vector_type(4))) RadianceRecord;
typedef __attribute__((address_space(3))) RadianceRecord LdsRadianceRecord;
__host__ __device__ constexpr uint32_t radiance_lds_bytes(uint32_t max_depth) { return max_depth * kBlock * 16u; }

// What whitted_level.inc reads of its `P`.  The options a caller's ray does not have are constants: the level body's
// branches on them fold away (no debug view, no soft shadows, no zero-weight reflection rays put aside).
struct RadianceQueryParams {
  DevScene sc;
  uint32_t n;
  const float* origin;     // n x 3
  const float* direction;  // n x 3, used as given
  int32_t max_depth;       // 0 .. P3D_RADIANCE_MAX_DEPTH
  uint32_t skybox;         // a miss is the cubemap's texel (the host: only with a cubemap)
  float* rgb;              // n x 3
  int32_t* hit_id;         // n, or null
  QueryStack stack;
  static constexpr uint32_t debug_view = P3D_DEBUG_NONE, soft_shadows = 0, level_stride = 0;
  static constexpr float light_side = 0.0f;
  static constexpr float4* deferred = nullptr;
};

// One ray per lane.  The ray starts as a primary ray starts: depth = max_depth, ior_1 = 1, outside every object, on an empty
// hit_stack that its chain, feelers included, carries on (Q2) - a pixel of a P3D_STACK_PER_PIXEL frame without
// anti-aliasing, whose bits this gives for that pixel's ray: the same level body in the same per-lane order.  The scene is
// read from global memory (L2), whatever its size; the BVH loops step by wave vote as in the other queries.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock) radiance_query_kernel(const RadianceQueryParams P) {
  constexpr int SPILL = kStackWindow, LIT = 0;
  constexpr bool STATS = false, AA = false, GHOST = false, COLD = false, VOTE = true;
  extern __shared__ float4 smem[];
  const DevScene& sc = P.sc;
  const uint32_t gid = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, gid);
  if (gid >= P.n) return;
  LdsRadianceRecord* records =
      (LdsRadianceRecord*)(reinterpret_cast<RadianceRecord*>(smem + stack_lds_f4(kStackWindow, (uint32_t)P.stack.stack_cap))) + threadIdx.x;
  Counters<STATS> ct;
  RayS ray;
  const size_t row = gid;  // (3 * row in 64 bits: n x 12 bytes may pass 4 GB)
  ray_set(ray, f3(P.origin[3 * row], P.origin[3 * row + 1], P.origin[3 * row + 2]),
          f3(P.direction[3 * row], P.direction[3 * row + 1], P.direction[3 * row + 2]));

  // what the level body names and a query does not have: one sample, no ghost chain, no hand-off records
  const int si = 0, sj = 0, SPP = 1;
  const bool ghost = false;
  int n_deferred = 0, first_hit = -1;
  Rng rng;
  rng.state = 0; rng.inc = 1;
  bool unit_touched = false;
  uint32_t unit_ch0[kCh0Counters] = {0, 0, 0, 0, 0};
  const Handoff H{};
  const uint32_t unit = 0;
  ColdState<COLD> cold;
#ifdef P3D_PT_PROFILE
  RegionProf prof; prof.init();  // (instrumented build: the level body marks its regions; only the megakernel reports them)
#endif

  int depth = P.max_depth;
  float ior_1 = 1.0f;
  bool inside = false;
  int level = 0;
  F3 chain_result = f3(0, 0, 0);
#define P3D_FIRST_HIT(obj) first_hit = (obj)
  while (true) {  // the reflect / refract chain of main.cpp:92-309 (whitted_sample.inc)
#include "whitted_level.inc"
    if (chain_ended) break;
    records[level * kBlock] = RadianceRecord{col.x, col.y, col.z, weight};
    ++level;
    --depth;
    ray_set(ray, child_o, child_d);
    ior_1 = child_ior;
    inside = child_inside;
  }
#undef P3D_FIRST_HIT
  (void)n_deferred; (void)unit_touched; (void)unit_ch0; (void)H; (void)unit;
  // fold the chain bottom-up with the per-level clamp (main.cpp:305-307, Q4)
  F3 result = chain_result;
  while (level > 0) {
    --level;
    const RadianceRecord rec = records[level * kBlock];
    result = clamp01(f3(rec.x, rec.y, rec.z) + result * rec.w);
  }
  store_f3(P.rgb, row, result);
  if (P.hit_id) P.hit_id[gid] = first_hit;
}

struct CameraRaysParams {
  DevCamera cam;
  int32_t x0, y0, w, h, stripe_h, stripe_stride;  // the tile, stripe_h >= 1
  float* origin;     // w*h x 3
  float* direction;  // w*h x 3
};

// primary_ray(cam, x + 0.5, y + 0.5) of every pixel of the tile, spelt as the frame kernels spell it (main.cpp:805-808), in
// the row order of the tile's frame
__global__ void __launch_bounds__(256) camera_rays_kernel(const CameraRaysParams C) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint32_t)C.w * (uint32_t)C.h) return;
  const int r = (int)(i / (uint32_t)C.w), c = (int)(i - (uint32_t)r * (uint32_t)C.w);
  const int x = C.x0 + c, y = stripe_row<int>(C.y0, r, C.stripe_h, C.stripe_stride);
  F3 o, d;
  primary_ray(C.cam, (float)(x + 0.5), (float)(y + 0.5), o, d);
  store_f3(C.origin, (size_t)i, o);
  store_f3(C.direction, (size_t)i, d);
}

}  // namespace p3d
