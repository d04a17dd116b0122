// path_query.hpp — path-traced radiance for rays in device memory (p3d_trace_path_device), and the sample rays of a camera
// (p3d_camera_sample_rays_device).  path_query_kernel is Radiance (main.cpp:313-516) for a ray that is nobody's pixel: the
// persistent bounce loop of pt_body.inc in its one-lane-per-pixel shape spelled around pt_bounce.inc, the one spelling of a
// bounce, on the stack of the ray queries (queries.hpp QueryStack).  camera_sample_rays_kernel is make_primary
// (main.cpp:758-787) for one sample of every pixel of a tile, with the RNG state the sample's path goes on from.
#pragma once

#include "pt_kernel.hpp"       // det_sincos, kPIf, P3D_PT_WAVES: what pt_bounce.inc names
#include "queries.hpp"         // QueryStack, query_stack_bind, store_f3
#include "radiance_query.hpp"  // RadianceRecord, LdsRadianceRecord: one 16-byte LDS access

// Bytes of dynamic LDS a launch of path_query_kernel asks for and does not use: an experiment build (make variant) runs the
// kernel at a lower occupancy with it (profiles/tools/trace_path_probe.py).  0 in the product library.
#ifndef P3D_PATH_QUERY_LDS_PAD
#define P3D_PATH_QUERY_LDS_PAD 0
#endif

namespace p3d {

// The two pending dielectric branches of a lane (main.cpp:512-513: only the first two bounces fork), 3 x 16 bytes each, in
// dynamic LDS behind the stack window with the lane as the fastest index: float4 q of entry e of lane t at
// [(e * 3 + q) * kBlock + t].  pt_bounce.inc writes them as pend.base[(e * 3 + q) * pend.stride] = float4, which the frame
// kernels resolve to their global scratch; here the same expression is one ds_write_b128 through an address-space-3
// pointer (a float4 of HIP is a class: it is assigned through the vector type of the radiance records).  No scratch, so the
// call allocates nothing.  6 KB per wave next to the 8 KB window.
struct LdsPending {
  struct Slot {
    LdsRadianceRecord* p;
    __device__ __forceinline__ void operator=(const float4& v) const { *p = RadianceRecord{v.x, v.y, v.z, v.w}; }
    __device__ __forceinline__ float4 load() const { const RadianceRecord r = *p; return make_float4(r.x, r.y, r.z, r.w); }
  };
  struct Base {
    LdsRadianceRecord* p;
    __device__ __forceinline__ Slot operator[](size_t i) const { return Slot{p + (uint32_t)i}; }
  };
  Base base;
  static constexpr uint32_t stride = kBlock;
  int n;
};
constexpr uint32_t kPathPending = 2;  // entries per lane
__host__ __device__ constexpr uint32_t path_lds_bytes() { return kPathPending * 3u * kBlock * 16u + (uint32_t)(P3D_PATH_QUERY_LDS_PAD); }

// {state, inc} of one ray's stream: one 16-byte access, at the 8-byte alignment of a uint64 array
typedef unsigned long long __attribute__((ext_vector_type(2), aligned(8))) RngWords;

// What pt_bounce.inc reads of its `P`.  A caller's ray has no debug view: the branch on it folds away.
struct PathQueryParams {
  DevScene sc;
  uint32_t n;
  const float* origin;     // n x 3
  const float* direction;  // n x 3, used as given
  int32_t max_depth;
  uint32_t skybox;         // a miss is the cubemap's texel (the host: only with a cubemap)
  uint32_t accumulate;     // the sum starts from what rgb holds
  uint32_t sample_begin, samples;  // samples >= 1, sample_begin + samples <= 2^32
  uint64_t seed;
  RngWords* rng;           // n x {state, inc}, in/out, or null: sample s of ray i draws from seed_stream(seed, i, s)
  float* rgb;              // n x 3
  int32_t* hit_id;         // n, or null
  QueryStack stack;
  static constexpr uint32_t debug_view = P3D_DEBUG_NONE;
};

// One ray per lane.  Every sample starts as a sample of a pixel starts - on a cleared stack, T = 1, L = 0, depth = max_depth -
// from the same ray, and the lane adds its samples up in sample order: a pixel of a path-traced frame whose primary rays
// and RNG states the caller brought along (camera_sample_rays_kernel gives them), in that frame's bits.  A lane whose path
// ended pops its pending branch or starts its next sample in the same trip, so a wave lasts as long as its longest lane's
// sample SET.  The scene is read from global memory (L2), whatever its size; the BVH loops step by wave vote as in the
// other queries.  The path tracer asks closest-hit queries only, which leave the stack empty: its worst case is one
// traversal's.
template <int ACCEL>
__global__ void __launch_bounds__(kBlock, P3D_PT_WAVES) path_query_kernel(const PathQueryParams P) {
  constexpr int SUB = 1, PT_STACK = kStackWindow;
  constexpr bool LDS = false, STATS = false;
  extern __shared__ float4 smem[];
  const DevScene& sc = P.sc;
  const uint32_t gid = blockIdx.x * kBlock + threadIdx.x;
  Stack st;
  query_stack_bind(st, smem, P.stack, gid);
  if (gid >= P.n) return;
  LdsPending pend;
  pend.base.p = (LdsRadianceRecord*)(reinterpret_cast<RadianceRecord*>(smem + stack_lds_f4(kStackWindow, (uint32_t)P.stack.stack_cap))) + threadIdx.x;
  pend.n = 0;
  Counters<STATS> ct;
  const size_t row = gid;  // (3 * row in 64 bits: n x 12 bytes may pass 4 GB)
  const F3 ray_o = f3(P.origin[3 * row], P.origin[3 * row + 1], P.origin[3 * row + 2]);
  const F3 ray_d = f3(P.direction[3 * row], P.direction[3 * row + 1], P.direction[3 * row + 2]);
  const int MAXD = P.max_depth;

  // what the bounce names and a query does not have: the sample ring of the four-lanes-per-pixel kernels
  struct { int first_hit[1]; } shared;
  const uint32_t px = 0;
#ifdef P3D_PT_PROFILE
  RegionProf prof; prof.init();  // (instrumented build: the bounce marks its regions; only the frame kernels report them)
#endif

  F3 color = f3(0, 0, 0);  // the sum of the samples, spelt as the frame spells it (main.cpp:792)
  if (P.accumulate) color = f3(P.rgb[3 * row], P.rgb[3 * row + 1], P.rgb[3 * row + 2]);
  int first_hit = -1;
  uint32_t s = P.sample_begin, left = P.samples;  // next sample to start; samples not yet started
  Rng rng;
  rng.state = 0; rng.inc = 1;
  if (P.rng) {
    const RngWords v = P.rng[gid];
    rng.state = v.x; rng.inc = v.y;
  }
  bool alive = false, in_sample = false, first_ray = false;
  RayS ray;
  F3 T = f3(1, 1, 1), L = f3(0, 0, 0);
  int depth = 0;
  while (true) {
    if (!alive) {
      if (pend.n > 0) {  // resume the deferred reflection branch of a dielectric hit
        --pend.n;
        const float4 q0 = pend.base[(size_t)(pend.n * 3 + 0) * pend.stride].load(), q1 = pend.base[(size_t)(pend.n * 3 + 1) * pend.stride].load(),
                     q2 = pend.base[(size_t)(pend.n * 3 + 2) * pend.stride].load();
        ray_set(ray, f3(q0.x, q0.y, q0.z), f3(q0.w, q1.x, q1.y));
        T = f3(q1.z, q1.w, q2.x);
        depth = __float_as_int(q2.y);
        alive = true;
      } else {
        if (in_sample) {
          color = color + L;
          in_sample = false;
        }
        if (left == 0) break;
        if (!P.rng) rng.seed_stream(P.seed, gid, s);  // the frame's rule with the ray in the pixel's place
        stack_clear(st);
        ray_set(ray, ray_o, ray_d);
        T = f3(1, 1, 1);
        L = f3(0, 0, 0);
        depth = MAXD;
        first_ray = (left == P.samples);  // the ray is the same in every sample: the call's first one names the hit
        ++s;
        --left;
        alive = true;
        in_sample = true;
      }
    }
#include "pt_bounce.inc"
  }
  (void)shared; (void)px;
  if (P.rng) P.rng[gid] = RngWords{rng.state, rng.inc};
  store_f3(P.rgb, row, color);
  if (P.hit_id) P.hit_id[gid] = first_hit;
}

struct CameraSampleRaysParams {
  DevCamera cam;
  int32_t x0, y0, w, h, stripe_h, stripe_stride;  // the tile, stripe_h >= 1
  uint32_t spp_sqrt, antialiasing, depth_of_field, sample_disk, sample_mode;  // of the p3d_config
  uint32_t sample;  // < spp_sqrt^2
  uint64_t seed;
  float* origin;     // w*h x 3
  float* direction;  // w*h x 3
  RngWords* rng;     // w*h x {state, inc} after the sample's draws, or null
};

// Sample `sample` of every pixel of the tile as the frame loop casts it (main.cpp:758-787): the pixel's stream of that
// sample, seeded as the frame kernels seed it, and make_primary with the options of the config - the fields of a
// RenderParams make_primary reads, nothing else of it is touched.  In the row order of the tile's frame.
__global__ void __launch_bounds__(256) camera_sample_rays_kernel(const CameraSampleRaysParams C) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= (uint32_t)C.w * (uint32_t)C.h) return;
  const int r = (int)(i / (uint32_t)C.w), c = (int)(i - (uint32_t)r * (uint32_t)C.w);
  const int x = C.x0 + c, y = stripe_row<int>(C.y0, r, C.stripe_h, C.stripe_stride);
  RenderParams R;
  R.spp_sqrt = C.spp_sqrt; R.antialiasing = C.antialiasing; R.depth_of_field = C.depth_of_field;
  R.sample_disk = C.sample_disk; R.sample_mode = C.sample_mode;
  const int SPP = (int)C.spp_sqrt;
  const int si = (int)C.sample / SPP, sj = (int)C.sample - si * SPP;
  Rng rng;
  rng.seed_stream(C.seed, (uint32_t)(y * C.cam.res_x + x), C.sample);
  F3 o, d;
  make_primary(R, C.cam, x, y, si, sj, rng, o, d);
  store_f3(C.origin, (size_t)i, o);
  store_f3(C.direction, (size_t)i, d);
  if (C.rng) C.rng[i] = RngWords{rng.state, rng.inc};
}

}  // namespace p3d
