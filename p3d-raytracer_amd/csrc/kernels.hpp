// kernels.hpp — what every render kernel shares (launch parameters, scene staging, tile schedule, pixel samples, the
// four-lanes-per-pixel ring) and the Whitted megakernel (gfx950).
//
//   whitted_kernel : primary ray -> closest hit -> Blinn-Phong with shadow feelers ->
//                    reflect / refract chain with per-level clamp      (main.cpp:92-309 + 753-820)
//   elsewhere      : pt_kernel.hpp (path tracer), handoff_kernels.hpp (hit_stack hand-off), wavefront.hpp (one launch
//                    per chain level), queries.hpp (batched queries)
//
// One workgroup = one wavefront = an 8x8 pixel block.  See device_core.hpp for the
// traversal conventions and DESIGN.md for the kernel-by-kernel roofline discussion.
#pragma once

#include "device_core.hpp"
#include "handoff.hpp"
#include "p3d.h"

// Minimum waves per SIMD the register allocator must leave room for (2nd __launch_bounds__ argument): whitted_waves() below
// says which instantiation gets which.
#ifndef P3D_WHITTED_WAVES
#define P3D_WHITTED_WAVES 2
#endif
#ifndef P3D_LIST_WAVES
#define P3D_LIST_WAVES 4
#endif
#ifndef P3D_WHITTED_GLOBAL_WAVES
#define P3D_WHITTED_GLOBAL_WAVES 6
#endif
#ifndef P3D_WHITTED_LDS_WAVES
#define P3D_WHITTED_LDS_WAVES 5
#endif

namespace p3d {

#ifdef P3D_TIMELINE  // debug builds only (build/variants): per-workgroup start/end clock + HW id
__device__ unsigned long long* g_timeline = nullptr;
#define P3D_TL_BEGIN() const unsigned long long tl_t0 = wall_clock64();
#define P3D_TL_END()                                                                                  \
  if (g_timeline && threadIdx.x == 0) {                                                               \
    g_timeline[3 * (size_t)blockIdx.x] = tl_t0;                                                       \
    g_timeline[3 * (size_t)blockIdx.x + 1] = wall_clock64();                                          \
    g_timeline[3 * (size_t)blockIdx.x + 2] =                                                          \
        ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | __builtin_amdgcn_s_getreg(63492); \
  }
#else
#define P3D_TL_BEGIN()
#define P3D_TL_END()
#endif

#ifdef P3D_ENTRY_CLOCK  // debug builds only (profiles/tools/entry_clock.py): per-workgroup ticks from the first instruction of
// whitted_kernel to the end of scene staging (kind 2) or to the LIT == 3 exit (kind 1), and to the end of the workgroup.
// Round 0 (LIT == 3) records behind g_entry_half workgroups, so that one frame keeps pass 1 and round 0 apart; the work-list
// launches (LIT == 2) record nothing.
__device__ unsigned long long* g_entry_clock = nullptr;
__device__ unsigned int g_entry_half = 0;
#define P3D_EC_SLOT(LIT) (3 * ((size_t)((LIT) == 3 ? g_entry_half : 0u) + blockIdx.x))
#define P3D_EC_BEGIN() const unsigned long long ec_t0 = wall_clock64();
#define P3D_EC_MARK(LIT, kind)                                          \
  if ((LIT) != 2 && g_entry_clock && threadIdx.x == 0) {                \
    g_entry_clock[P3D_EC_SLOT(LIT)] = wall_clock64() - ec_t0;           \
    g_entry_clock[P3D_EC_SLOT(LIT) + 2] = (kind);                       \
  }
#define P3D_EC_END(LIT) \
  if ((LIT) != 2 && g_entry_clock && threadIdx.x == 0) g_entry_clock[P3D_EC_SLOT(LIT) + 1] = wall_clock64() - ec_t0;
#else
#define P3D_EC_BEGIN()
#define P3D_EC_MARK(LIT, kind)
#define P3D_EC_END(LIT)
#endif

#ifdef P3D_PT_PROFILE  // debug builds only: wave-time, entries and active lanes per region of a kernel's loop
__device__ unsigned long long* g_pt_prof = nullptr;
constexpr int kProfRegions = 12;
// The clock belongs to the wave, not to a lane: whichever lanes reach a marker, the time since the previous marker
// (reached by any lanes) was spent executing the region that marker opened — divergent paths run one after the other.
struct RegionProfShared { unsigned long long acc[kProfRegions], lanes[kProfRegions], iters[kProfRegions], last; int cur; };
struct RegionProf {
  volatile RegionProfShared* s;
  __device__ void init() {
    __shared__ RegionProfShared sh;  // one wave per workgroup
    s = &sh;
    if (__ffsll((unsigned long long)__ballot(1)) - 1 == (int)(threadIdx.x & 63)) {
      for (int i = 0; i < kProfRegions; ++i) s->acc[i] = s->lanes[i] = s->iters[i] = 0;
      s->cur = 0; s->last = __builtin_readcyclecounter();
    }
  }
  __device__ void enter(int r) {
    __builtin_amdgcn_s_waitcnt(0);  // outstanding loads belong to the region that issued them
    const unsigned long long now = __builtin_readcyclecounter(), m = __ballot(1);
    if (__ffsll(m) - 1 == (int)(threadIdx.x & 63)) {
      s->acc[s->cur] += now - s->last; s->last = now; s->cur = r;
      s->lanes[r] += __popcll(m); s->iters[r] += 1;
    }
    __builtin_amdgcn_s_waitcnt(0);
  }
  __device__ void flush() {
    if (g_pt_prof && __ffsll((unsigned long long)__ballot(1)) - 1 == (int)(threadIdx.x & 63))
      for (int i = 0; i < kProfRegions; ++i) {
        atomicAdd(&g_pt_prof[3 * i], s->acc[i]); atomicAdd(&g_pt_prof[3 * i + 1], s->lanes[i]); atomicAdd(&g_pt_prof[3 * i + 2], s->iters[i]);
      }
  }
};
#define PT_REGION(r) prof.enter(r);
#else
#define PT_REGION(r)
#endif

struct RenderParams {
  DevScene sc;
  const float4* blob;   // all float4 scene arrays, contiguous (for the LDS staging copy)
  uint32_t blob_f4;     // float4s of blob staged in LDS (= lds_scene_f4 when the scene is staged): the arrays a kernel of this
                        // launch reads in its loops, without the alignment pad in front and - Whitted over the BVH, which only
                        // reads the BVH-ordered copy - without the object-order geometry at the end
  uint32_t stage_lo;    // first staged float4 of blob
  // byte offsets (in float4) of the arrays inside blob, same order as DevScene
  uint32_t off_nodes, off_bgeom, off_ogeom, off_normals, off_mats, off_lights;
  // options (p3d_config)
  int32_t max_depth;
  uint32_t spp_sqrt, antialiasing, depth_of_field, sample_disk, soft_shadows, sample_mode;
  float light_side, gamma;
  uint32_t skybox;  // miss = cubemap texel (only set when the scene has a cubemap)
  uint32_t debug_view;  // P3D_DEBUG_* (constants.h:18,33)
  uint64_t seed;
  // tile
  int32_t x0, y0, w, h, stripe_h, stripe_stride;
  uint32_t tiles_x, tiles_y, xcd_chunk;
  uint32_t tile_w_shift, tile_h_shift;  // one-lane-per-pixel kernels: a wave renders a (1 << w) x (1 << h) pixel tile: 8x8, 8x4 or 4x4 (host: tile_shape)
  // outputs (device memory, any may be null)
  float* rgb;
  int32_t* hit_id;
  uint8_t* rgb8;
  // scratch
  float4* levels;          // Whitted per-level records {local colour, child weight}, [level][thread]
  uint32_t level_stride;   // threads in this launch
  unsigned long long* stats;  // kNumStats counters
  uint2* spill;               // backing array of the node stack (entries that sank out of the LDS window), [entry][thread]
  int32_t stack_cap;          // node-stack entries per lane held in LDS (spilling stack: the window, a power of two)
  uint32_t lds_scene_f4;      // float4s reserved for the staged scene (0 when not staged)
  // Cost-ordered tile schedule (DESIGN.md "Tile schedule"); both null: frame order, nothing recorded.
  //   sched: see sched_build_kernel.   tile_cost[t]: wall-clock ticks the workgroup of tile t was resident.
  const uint32_t* sched;
  uint32_t* tile_cost;
  uint32_t stack_spills;  // LDS-staged scene with the spilling stack (host-side kernel choice)
  // P3D_STACK_LITERAL (handoff.hpp)
  Handoff hand;
  int32_t row0;            // first tile row of this launch (units are numbered over the whole tile)
  uint32_t tile_blocks;    // workgroups that render tiles; the ones behind them render halo chains (pass 1, check)
  float4* deferred;        // zero-weight reflection rays put aside, 2 x float4 each, [2 * entry][thread]
  uint32_t* status;        // device-detected errors of this scene (kHoErr* bits), never cleared by a kernel
  uint32_t debug_trip_bound;  // tests only: trip bound of the four-lanes-per-pixel sample loops (0 = the real bound)
  // Per-level ("wavefront") launches of the Whitted chain, scenes traversed from L2 (wf_level_kernel)
  uint32_t wf_level;       // chain level this launch renders
  uint32_t wf_seg_cap;     // entries per queue segment
  float4* wf_ray_in;       // [kWfSegments][wf_seg_cap][2]: rays this level traces, written by the level above
  float4* wf_ray_out;
  const uint32_t* wf_n_in; // [kWfSegments] counters, one per 128-byte line
  uint32_t* wf_n_out;
  float4* wf_final;        // [units] {colour the chain ended with, number of level records below it}
  uint32_t level_stride2;  // units: stride of the level records of the per-level launches
  // binning of the child rays by origin cell and direction octant between two levels (wf_scan_kernel, wf_scatter_kernel)
  uint32_t* wf_key_out;    // [kWfSegments][wf_seg_cap] bin of every staged ray
  const uint32_t* wf_key_in;
  uint32_t* wf_hist;       // [kWfBins + 1] rays per bin of the level being written; after the scan: first slot of each bin
  const uint32_t* wf_total;  // rays in the sorted queue this launch reads
  float4* wf_sorted;       // [units][2] the queue in bin order
  F3 wf_cell_origin, wf_cell_scale;  // cell = (origin - wf_cell_origin) * wf_cell_scale, clamped to [0, kWfCellsPerAxis)
  // Sample range of this launch (anti-aliased kernels only; p3d_accum, include/p3d.h): samples [sample_begin, sample_end) of
  // every pixel.  A whole frame is [0, SPP^2) with no accumulator.  With sample_begin > 0 a pixel's running sum and first
  // hit start from accum_sum / accum_hit; with accum_sum set the raw sum and first hit are stored there at the end.  (Last in
  // the struct: the kernarg offsets of every field above stay what they were.)
  uint32_t sample_begin, sample_end;
  float* accum_sum;        // [3 * pixel] running sum of the samples so far (before the division by the sample count)
  int32_t* accum_hit;      // [pixel] first hit of global sample 0
};

// LDS map of one workgroup:  [ staged scene (lds_scene_f4 float4) | node stack (cap * 64 * 8 B) | per-pixel sample ring (PT, 4 lanes per pixel) ]
// OBJECTS: the launch stages the object-order geometry too (every kernel but Whitted over the BVH; the host's stage range)
// The copy comes in two halves, so that a kernel can have its first loads on their way while it waits for something that
// does not depend on them (whitted_kernel: its schedule entry): stage_issue() starts the loads of the lane's first
// kStageBatch float4s, stage_scene() stores them and copies what is left, kStageBatch loads of a lane in flight at a time (a
// plain loop of load + store waits for every load on its own).  A load past the staged range reads the range's last float4
// instead and is not stored.  16 registers, at a point where a kernel holds little else.  What it buys is small - every
// wave of a CU reads the same few KB, the round trips are short - and measured in profiles/entry/README.md.
constexpr int kStageBatch = 4;
static_assert(kStageBatch == 4, "StageRegs holds a batch in named members (an indexed array in a struct that lives across the kernel's early exits went to scratch)");
struct StageBatch { float4 a, b, c, d; };
template <bool LDS> struct StageRegs { StageBatch v; };
template <> struct StageRegs<false> {};

__device__ __forceinline__ StageBatch stage_load_batch(const RenderParams& P, uint32_t base) {
  StageBatch v;
  const float4* src = P.blob + P.stage_lo;
  const uint32_t last = P.blob_f4 - 1;  // (callers: blob_f4 != 0)
  const uint32_t i = base + threadIdx.x;
  v.a = src[i < last ? i : last];
  v.b = src[i + kBlock < last ? i + kBlock : last];
  v.c = src[i + 2 * kBlock < last ? i + 2 * kBlock : last];
  v.d = src[i + 3 * kBlock < last ? i + 3 * kBlock : last];
  return v;
}
__device__ __forceinline__ void stage_store_batch(const RenderParams& P, uint32_t base, const StageBatch& v, float4* smem) {
  const uint32_t i = base + threadIdx.x;
  if (i < P.blob_f4) smem[i] = v.a;
  if (i + kBlock < P.blob_f4) smem[i + kBlock] = v.b;
  if (i + 2 * kBlock < P.blob_f4) smem[i + 2 * kBlock] = v.c;
  if (i + 3 * kBlock < P.blob_f4) smem[i + 3 * kBlock] = v.d;
}

template <bool LDS>
__device__ __forceinline__ void stage_issue(const RenderParams& P, StageRegs<LDS>& first) {
  if constexpr (LDS) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    first.v = P.blob_f4 ? stage_load_batch(P, 0) : StageBatch{zero, zero, zero, zero};
  }
}

// the copy is complete: wait for every lane's stores, then the kernel's scene arrays are the staged ones
template <bool OBJECTS>
__device__ __forceinline__ void stage_bind(DevScene& sc, const RenderParams& P, float4* smem) {
  __syncthreads();
  sc.nodes = smem + (P.off_nodes - P.stage_lo);
  sc.bgeom = smem + (P.off_bgeom - P.stage_lo);
  sc.normals = smem + (P.off_normals - P.stage_lo);
  sc.mats = smem + (P.off_mats - P.stage_lo);
  sc.lights = smem + (P.off_lights - P.stage_lo);
  if (OBJECTS) sc.ogeom = smem + (P.off_ogeom - P.stage_lo);  // (otherwise: stays in global memory)
}

template <bool LDS, bool OBJECTS>
__device__ __forceinline__ void stage_scene(DevScene& sc, const RenderParams& P, float4* smem, const StageRegs<LDS>& first) {
  if constexpr (LDS) {
    if (P.blob_f4) stage_store_batch(P, 0, first.v, smem);
    for (uint32_t base = kStageBatch * kBlock; base < P.blob_f4; base += kStageBatch * kBlock)
      stage_store_batch(P, base, stage_load_batch(P, base), smem);
    stage_bind<OBJECTS>(sc, P, smem);
  }
}
template <bool LDS, bool OBJECTS>
__device__ __forceinline__ void stage_scene(DevScene& sc, const RenderParams& P, float4* smem) {
  StageRegs<LDS> first;
  stage_issue<LDS>(P, first);
  stage_scene<LDS, OBJECTS>(sc, P, smem, first);
}
// One float4 at a time, every load waited for on its own: the work-list launches of the hit_stack hand-off only (a few
// waves behind a frame's round 0, nothing to gain; with the batched copy two of their anti-aliased instantiations, which
// the allocator holds to 128 registers, spilled 12 and 16 bytes more).
template <bool LDS, bool OBJECTS>
__device__ __forceinline__ void stage_scene_plain(DevScene& sc, const RenderParams& P, float4* smem) {
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < P.blob_f4; i += kBlock) smem[i] = P.blob[P.stage_lo + i];
    stage_bind<OBJECTS>(sc, P, smem);
  }
}

// XCD-aware block -> tile map.  Workgroups are dealt round-robin over the 8 XCDs, so blocks
// b, b+8, b+16, ... share an L2.  Tiles are grouped into chunks of `xcd_chunk` consecutive
// 8x8 tiles (one tile row of the frame for big scenes) and chunks are dealt to XCDs round-
// robin: each XCD's L2 sees spatially coherent rays (matters for the 8.8 MB scene, which
// does not fit one 4 MiB L2) while expensive and cheap image regions are still spread over
// all XCDs.  xcd_chunk = 1 is the identity map (LDS-staged scenes have no L2 working set).
//
// With a schedule (DESIGN.md "Tile schedule") blockIdx order is "most expensive class first":
// workgroups are dispatched in blockIdx order, so the few long-running tiles start at once and
// the many short ones fill in behind them instead of the other way round.
__device__ __forceinline__ bool tile_of_block(const RenderParams& P, uint32_t& tx, uint32_t& ty) {
  const uint32_t b = blockIdx.x;
  const uint32_t n = P.tiles_x * P.tiles_y;
  uint32_t tile;
  if (P.sched) {
    if (b >= n) return false;
    tile = P.sched[b];
  } else {
    const uint32_t j = b >> 3;
    tile = ((j / P.xcd_chunk) * 8 + (b & 7u)) * P.xcd_chunk + (j % P.xcd_chunk);
    if (tile >= n) return false;
  }
  tx = tile % P.tiles_x;
  ty = tile / P.tiles_x;
  return true;
}

// Cost of a finished tile, for the schedule of the following launches.
__device__ __forceinline__ void record_tile_cost(const RenderParams& P, uint32_t tx, uint32_t ty, unsigned long long t_begin) {
  if (P.tile_cost && threadIdx.x == 0) P.tile_cost[ty * P.tiles_x + tx] = (uint32_t)(wall_clock64() - t_begin);
}

// One workgroup: counting sort of the tiles by cost class, most expensive class first.  Classes
// are quarter octaves of cost / mean cost, from below 1/4 to above 3.4 (order inside a class:
// arrival).  sched[i] = the tile workgroup i renders.
constexpr int kSchedBuildThreads = 1024;
constexpr int kSchedClasses = 16;
__device__ __forceinline__ int sched_class(uint32_t cost, float mean) {
  if (cost == 0) return 0;
  const int c = (int)floorf(log2f((float)cost / mean) * 4.0f) + 8;
  return c < 0 ? 0 : (c >= kSchedClasses ? kSchedClasses - 1 : c);
}

__global__ void __launch_bounds__(kSchedBuildThreads) sched_build_kernel(const uint32_t* cost, uint32_t n, uint32_t* sched) {
  __shared__ unsigned long long total;
  __shared__ uint32_t cursor[kSchedClasses];
  if (threadIdx.x == 0) total = 0;
  if (threadIdx.x < kSchedClasses) cursor[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long mine = 0;
  for (uint32_t t = threadIdx.x; t < n; t += kSchedBuildThreads) mine += cost[t];
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&total, mine);
  __syncthreads();
  const float mean = fmaxf((float)total / (float)n, 1.0f);
  for (uint32_t t = threadIdx.x; t < n; t += kSchedBuildThreads) atomicAdd(&cursor[sched_class(cost[t], mean)], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {  // class sizes -> first slot of each class, most expensive class first
    uint32_t at = 0;
    for (int c = kSchedClasses - 1; c >= 0; --c) {
      const uint32_t size = cursor[c];
      cursor[c] = at;
      at += size;
    }
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < n; t += kSchedBuildThreads) sched[atomicAdd(&cursor[sched_class(cost[t], mean)], 1u)] = t;
}

// One launch instead of a hipMemsetAsync per buffer (each of those is a fill kernel of its own, ~5 us): zeroes up to
// three word ranges at the head of a frame (counters, touched bits, statistics).
struct ClearParams {
  uint32_t* p[3];
  uint32_t n[3];
  const uint32_t* halo_verdict;  // kHoErrHalo or 0 as the last halo_find_kernel launch for this tile left it (the search is
  uint32_t* status;              // memoised per tile; its verdict holds for every frame that uses the memoised chain)
};
__global__ void __launch_bounds__(256) clear_kernel(const ClearParams C) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
  if (i == 0 && C.halo_verdict && *C.halo_verdict) atomicOr(C.status, *C.halo_verdict);
  for (int k = 0; k < 3; ++k)
    for (uint32_t j = i; j < C.n[k]; j += stride) C.p[k][j] = 0;
}

template <bool STATS>
__device__ __forceinline__ void flush_stats(Counters<STATS>&, unsigned long long*) {}
template <>
__device__ __forceinline__ void flush_stats<true>(Counters<true>& ct, unsigned long long* out) {
  for (int s = 0; s < kNumStats; ++s) {
    uint32_t v = ct.c[s];
    if (s == kMaxStack) {
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = __shfl_xor(v, o, 64);
        v = other > v ? other : v;
      }
      if ((threadIdx.x & 63) == 0) atomicMax(&out[s], (unsigned long long)v);
    } else {
      unsigned long long w = v;
      for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
      if ((threadIdx.x & 63) == 0 && w) atomicAdd(&out[s], w);
    }
  }
}

// Pixel sample of main.cpp:758-787: sub-pixel position (jitter / tent), optional lens sample.
__device__ __forceinline__ void make_primary(const RenderParams& P, const DevCamera& cam, int x, int y, int i, int j,
                                             Rng& rng, F3& o, F3& d) {
  const int SPP = (int)P.spp_sqrt;
  float px, py;
  if (!P.antialiasing) {  // main.cpp:805-808
    px = (float)(x + 0.5);
    py = (float)(y + 0.5);
    primary_ray(cam, px, py, o, d);
    return;
  }
  if (P.sample_mode == P3D_SAMPLE_JITTER) {  // main.cpp:763-766
    px = x + (i + rng.rand_float()) / SPP;
    py = y + (j + rng.rand_float()) / SPP;
  } else {  // tent, main.cpp:767-773
    const double r1 = 2 * rng.erand48(), dx = r1 < 1 ? sqrt(r1) - 1 : 1 - sqrt(2 - r1);
    const double r2 = 2 * rng.erand48(), dy = r2 < 1 ? sqrt(r2) - 1 : 1 - sqrt(2 - r2);
    px = (float)(x + (0.5 + dx) / SPP);
    py = (float)(y + (0.5 + dy) / SPP);
  }
  if (P.depth_of_field) {  // main.cpp:776-784
    float lx, ly;
    if (P.sample_disk) {  // sampler.cpp:5-11; argument order as g++ evaluates it: y first
      do {
        const float b = rng.rand_float();
        const float a = rng.rand_float();
        lx = a * 2 - 1.0f;
        ly = b * 2 - 1.0f;
      } while (lx * lx + ly * ly + 0.0f * 0.0f >= 1.0f);
    } else {
      lx = (i + rng.rand_float()) / SPP;
      ly = (j + rng.rand_float()) / SPP;
    }
    primary_ray_lens(cam, lx, ly, px, py, o, d);
  } else {
    primary_ray(cam, px, py, o, d);
  }
}

// Four lanes per pixel (SUB = 4 of pt_kernel and of the anti-aliased whitted_kernel; a wave renders a 4x4-pixel tile).  The samples of a pixel are
// independent (own RNG stream each) but main.cpp:792-800 adds them up in sample order, and float
// addition does not commute: the four lanes take the pixel's samples in order from a shared
// counter, post each finished sample's radiance to a small ring in LDS, and lane 0 of the pixel
// adds the ring entries to the pixel colour strictly in sample order.  Same samples, same sum,
// four times more and four times shorter workgroups (DESIGN.md "Tile schedule": the path
// tracer's frame ends with a tail as long as its last tiles).
constexpr int kPtRing = 16;  // finished samples a pixel can hold before the oldest one is added
struct PtPixelShared {       // [..][pixel]: the 16 pixels of the tile are the fastest index (LDS banks)
  uint32_t next_start[16];   // next sample index to hand out (runs past the last sample: one ticket per finished lane)
  uint32_t next_add[16];     // next sample index to add to the pixel colour
  int32_t first_hit[16];
  float colour[3][16];             // the pixel's running sum (kept here, not in lane 0's registers)
  uint32_t tag[kPtRing][16];       // sample index + 1 of the radiance in that ring slot
  float radiance[kPtRing][3][16];
};

typedef __attribute__((address_space(3))) volatile PtPixelShared LdsPtPixelShared;
__device__ __forceinline__ void ring_init(LdsPtPixelShared& shared, uint32_t px, uint32_t sample_begin) {
  shared.next_start[px] = sample_begin;
  shared.next_add[px] = sample_begin;
  shared.first_hit[px] = -1;
  shared.colour[0][px] = 0.0f; shared.colour[1][px] = 0.0f; shared.colour[2][px] = 0.0f;
  for (int k = 0; k < kPtRing; ++k) shared.tag[k][px] = 0;
}
// post finished sample s; its ring slot is free (guaranteed when the sample was handed out)
__device__ __forceinline__ void ring_post(LdsPtPixelShared& shared, uint32_t px, int s, F3 radiance) {
  const int k = s % kPtRing;
  shared.radiance[k][0][px] = radiance.x; shared.radiance[k][1][px] = radiance.y; shared.radiance[k][2][px] = radiance.z;
  shared.tag[k][px] = (uint32_t)s + 1;
}

}  // namespace p3d

#include "handoff_kernels.hpp"  // uses the above; whitted_kernel uses its steps

namespace p3d {

// ---------------------------------------------------------------------------
// Whitted megakernel
// ---------------------------------------------------------------------------
//
// SUB = 4 (anti-aliased launches with at least four samples per pixel over a scene traversed from L2): four lanes per pixel, as in the path
// tracer — the samples of a pixel are handed out by ticket, finished samples wait in a ring in LDS and lane 0 of
// the pixel adds them in sample order (main.cpp:792-800 sums in that order).  An 8x8 tile of 4 x 4 = 16 chained
// samples per lane was the longest thing in such a frame; now a wave has a 4x4 tile and a quarter of the samples.
//
// LIT (P3D_STACK_LITERAL, handoff.hpp): 0 = the stack is emptied at every primary sample (one launch, nothing kept);
// 1 = pass 1: the pixel starts on an empty stack, the samples of the pixel hand the stack on, and the pixel's leftover,
// its touched flag and its first closest hit are recorded; 2 = the lanes take units from a work list, seed the stack
// with the predecessor's leftover, re-trace the first closest hit if the list entry asks for it, and render the unit again
// if that hit changed; 3 = round 0 of the hand-off over the TILES, check and repair in one launch (LDS-staged scenes): every lane
// whose unit starts on a non-empty leftover re-traces its first closest hit on it (what handoff_check_kernel does) and, if that
// hit changed, renders the unit again in the same wave (what the first work-list launch did with 64 unrelated pixels per
// wave: the units to repair of one tile are neighbours and walk the scene together - round 3, one box: the list launch
// cost the frames-in-flight loop of the bench workload 0.023 of its 0.126 ms per frame, profiles/r04/experiments).
// GHOSTS: the scene has a material that is transmissive AND reflective, i.e. LITERAL frames trace zero-weight reflection rays
// (whitted_sample.inc); without one the machinery is compiled out (pass 1 over the bench scene: 107 -> 96 VGPRs, five waves
// per SIMD like the per-pixel kernel).
constexpr int whitted_waves(bool AA, bool LDS, int LIT, bool GHOSTS) {
  // The work-list launches of the hit_stack hand-off (LIT == 2) are short lists of unrelated deep pixels: every wave waits on
  // its own dependent chain, so what counts is how many waves are resident at once, not registers per wave.
  if (LIT >= 2) return P3D_LIST_WAVES;
  if (AA) return P3D_WHITTED_WAVES;
  // The no-AA instantiations that traverse the scene from L2 wait on memory, not on the VALU, and trade registers for waves.
  // 100k triangles 1024x1024 / 2048x2048 with 16 / 12 / 12 / 10 / 8 LDS stack entries: 4 waves (111 VGPRs) 8.44 / 22.9 ms,
  // 5 (96) 7.69 / 20.7, 6 (80 VGPRs, 46 spilled dwords) 7.26 / 19.4, 7 (72) 7.40 / 18.7, 8 (64) 7.37 / 18.7.
  if (!LDS) return P3D_WHITTED_GLOBAL_WAVES;
  // One sample per pixel over an LDS-staged scene: 96 VGPRs = five waves per SIMD.  The per-pixel kernel needs exactly that; the
  // literal pass 1 needs 99 without the zero-weight-reflection machinery (GHOSTS = false) and is held to 96 without a spilled
  // dword (with it: 107, and holding it to 96 spills 12 dwords - profiles/r03/experiments §13).
  return (LIT == 1 && GHOSTS) ? P3D_WHITTED_WAVES : P3D_WHITTED_LDS_WAVES;
}
template <int ACCEL, bool LDS, bool STATS, bool AA, bool SPILL = !LDS, int SUB = 1, int LIT = 0, bool GHOSTS = true>
__global__ void __launch_bounds__(kBlock, whitted_waves(AA, LDS, LIT, GHOSTS)) whitted_kernel(const RenderParams P) {
  static_assert(SUB == 1 || AA, "four lanes per pixel need more than one sample per pixel");
  static_assert(LIT == 0 || (ACCEL == P3D_ACCEL_BVH && SUB == 1), "only the BVH has a stack to hand on; one lane per pixel");
  constexpr bool REDO = LIT >= 2;               // launches that render units again, seeded with their predecessor's leftover
  constexpr bool GHOST = LIT != 0 && GHOSTS;    // zero-weight reflection rays are put aside and traced (whitted_sample.inc)
  extern __shared__ float4 smem[];
  P3D_EC_BEGIN()
  // The staged bytes depend on neither the tile nor the schedule entry: the launches whose waves all stage (LIT < 2) start the
  // copy's first loads before anything else, the others behind the exit most of their waves take.
  constexpr bool STAGE_FIRST = LIT < 2, STAGE_PLAIN = LIT == 2;
  StageRegs<LDS && !STAGE_PLAIN> staged;
  if (STAGE_FIRST) stage_issue<LDS && !STAGE_PLAIN>(P, staged);
  uint32_t tx = 0, ty = 0;
  const bool halo_block = (LIT == 1 || LIT == 3) && blockIdx.x >= P.tile_blocks;
  if (LIT != 2 && !halo_block && !tile_of_block(P, tx, ty)) return;
  // LIT == 2: nothing on the list for this workgroup: leave before the scene is staged
  if (LIT == 2 && (size_t)blockIdx.x * P.hand.lanes >= list_count(P.hand.n_in, P.hand.list_cap)) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t tws = SUB == 4 ? 2u : P.tile_w_shift, ths = SUB == 4 ? 2u : P.tile_h_shift;  // tile = (1 << tws) x (1 << ths) pixels
  // LIT == 3: which lanes have anything to re-trace is known before the scene is staged, and most waves leave here.  The
  // predecessor's record is read from meta0, pass 1's copy: a predecessor repaired by another wave of THIS launch changes
  // its meta word while this wave may still be reading it (Jacobi: everybody starts from pass 1's leftovers).
  uint32_t t_unit = 0, t_pred = 0, t_slot_count = 0;
  bool t_need = false;
  if (LIT == 3) {
    const bool act = unit_of_lane(P, halo_block, tx, ty, tws, ths, lane, t_unit);
    if (act && handoff_touched(P.hand, t_unit)) {  // (twin: handoff_check_kernel, which reads meta)
      const int pred = handoff_pred(P.hand, t_unit);
      if (pred >= 0) {
        const uint32_t pm = P.hand.meta0[pred];
        t_need = (pm & 0xffffu) != 0;  // otherwise the predecessor left nothing: pass 1's empty stack was right
        t_pred = (uint32_t)pred;
        t_slot_count = pm & 0x1ffffu;
      }
    }
    if (__ballot(t_need) == 0) {
      P3D_EC_MARK(LIT, 1)
      P3D_EC_END(LIT)
      return;
    }
  }
  P3D_TL_BEGIN()
  const unsigned long long t_begin = (LIT < 2 && P.tile_cost) ? wall_clock64() : 0;
  DevScene sc = P.sc;
  if constexpr (STAGE_PLAIN) {
    stage_scene_plain<LDS, ACCEL != P3D_ACCEL_BVH>(sc, P, smem);
  } else {
    if (!STAGE_FIRST) stage_issue<LDS>(P, staged);
    stage_scene<LDS, ACCEL != P3D_ACCEL_BVH>(sc, P, smem, staged);
  }
  P3D_EC_MARK(LIT, 2)

  const uint32_t px = SUB == 4 ? lane >> 2 : lane;  // pixel of the tile this lane works for
  const uint32_t sub = SUB == 4 ? lane & 3u : 0u;
  Counters<STATS> ct;
  if (STATS) reinterpret_cast<Counters<true>&>(ct).clear();
  Stack st;
  stack_bind(st, smem, P.lds_scene_f4, lane, P.stack_cap, P.spill, P.level_stride, blockIdx.x * kBlock + lane);
  const uint32_t gid = blockIdx.x * kBlock + lane;
  // cold shading state behind the node stack (device_core.hpp ColdState): only the kernels that trade registers for waves
  constexpr bool COLD = !LDS && !AA;
  constexpr bool VOTE = !LDS;  // BVH loops by majority vote (device_core.hpp): scenes traversed from global memory only
  ColdState<COLD> cold;
  cold.bind(smem, P.lds_scene_f4 + stack_lds_f4(SPILL, P.stack_cap), lane);
  // per-pixel sample hand-out state behind the node stack (only allocated for SUB == 4); explicit LDS address space
  LdsPtPixelShared& shared = *(LdsPtPixelShared*)(smem + P.lds_scene_f4 + stack_lds_f4(SPILL, P.stack_cap));
  if (SUB == 4 && sub == 0) ring_init(shared, px, P.sample_begin);

  const Handoff& H = P.hand;
  uint4* list_in = H.list_in;
  uint4* list_out = H.list_out;
  uint32_t* n_in_p = H.n_in;
  uint32_t* n_out_p = H.n_out;
  for (uint32_t round = 0;; ++round) {  // LIT == 2 in one persistent workgroup: a trip per round; otherwise one trip
    uint32_t n_in = 0;
    if (LIT == 2) {
      n_in = list_count(n_in_p, H.list_cap);
      if (n_in == 0) break;
      if (H.round_base + round >= H.max_rounds) {  // work left after the last round allowed: the frame is not the serial one
        if (lane == 0) atomicOr(P.status, kHoErrNoFixedPoint);
        break;
      }
      if (H.count && blockIdx.x == 0 && lane == 0) {  // rounds that found work: round 1 as a flag (the tile launch's own re-checks raise it too)
        if (H.round_base + round == 1) atomicOr(&H.counters[kHoRound1], 1u);
        else atomicAdd(&H.counters[kHoRounds], 1u);
      }
    }
    for (uint32_t chunk = blockIdx.x;; chunk += gridDim.x) {  // LIT == 2: 64 list entries per trip
      bool active;
      UnitPlace up = no_place();
      uint32_t unit = 0, pred = 0, pred_slot_count = 0, flags = 0;
      if (LIT == 2) {
        if ((size_t)chunk * H.lanes >= n_in) break;
        const uint32_t i = chunk * H.lanes + lane;
        active = lane < H.lanes && i < n_in;
        if (active) {
          const uint4 e = list_entry(list_in, i);
          unit = e.x; pred = e.y; pred_slot_count = e.z; flags = e.w;
        }
      } else if (LIT == 3) {  // the tile's lanes that start on a non-empty leftover: check first, like a list entry with flag 1
        active = t_need;
        unit = t_unit; pred = t_pred; pred_slot_count = t_slot_count; flags = 1u;
      } else if (halo_block) {
        active = halo_unit_of_lane(P, lane, unit);
        up.halo = true;
        if (active) up = place_of_unit(P, unit);
      } else {
        active = tile_pixel(P, tx, ty, tws, ths, px, up.c, up.r);
        up.valid = active;
        up.x = P.x0 + up.c;
        up.y = image_row(P, up.r);
        if (LIT == 1) unit = unit_of_pixel(P, up.c, up.r);
      }
      if (REDO && active) {
        up = place_of_unit(P, unit);
        active = up.valid;
      }

      bool unit_touched = false;
      uint32_t unit_ch0[kCh0Counters] = {0, 0, 0, 0, 0};
      if (STATS && LIT != 0) ct.clear();  // LITERAL: counters per unit (store_unit_counters), not per lane
      if (REDO && active) {  // seed with the predecessor's leftover; re-trace the first closest hit if asked to
        seed_stack<SPILL>(st, H, pred, pred_slot_count, ct);
        if (flags & 1u) {  // (twin: first_hit_unchanged; calling it here spills more SGPRs in three LIT == 2 instantiations)
          if (H.count) atomicAdd(&H.counters[kHoChecked], 1u);
          const float4 now = first_closest_hit<SPILL, !LDS>(P, sc, st, up.x, up.y, AA ? H.first_sample[unit] : 0u, ct);
          if (same_first(now, H.first[unit])) {  // nothing this unit computes can differ
            active = false;
            replace_ch0_counters<STATS>(H, unit, ct, P.stats);
          } else {
            seed_stack<SPILL>(st, H, pred, pred_slot_count, ct);
          }
          if (STATS) ct.clear();
        }
        if (active && H.count) {
          atomicAdd(&H.counters[kHoRedone], 1u);
          if (LIT == 3) atomicOr(&H.counters[kHoRound0], 1u);  // (the tile launch is a round of its own if it repaired anything)
        }
      }
      if (LIT == 1) stack_clear(st);
      uint32_t leave_n = 0, leave_slot = 0;  // LIT != 0: entries this lane's unit leaves, stored after the lanes have come together again
      bool leave_succ = false;

      if (active) {
        const int c = up.c, r = up.r, x = up.x, y = up.y;
        const int SPP = AA ? (int)P.spp_sqrt : 1;
        if (sub == 0 && !(LIT != 0 && up.halo)) ct.add(kPixels);

        F3 color = f3(0, 0, 0);
        int first_hit = -1;
        Rng rng;
        rng.state = 0; rng.inc = 1;
#ifdef P3D_PT_PROFILE
        RegionProf prof; prof.init();
#endif
        // one sample per pixel: the hit ID goes to memory when it is known instead of riding through the whole chain in a register
        constexpr bool EARLY_HIT = !AA && !LDS;  // (kernels that trade registers for waves; over an LDS-staged scene the extra store only costs)
        if (EARLY_HIT && P.hit_id && !(LIT != 0 && up.halo)) P.hit_id[(size_t)r * P.w + c] = -1;  // a primary ray that is never traced (none: every sample is) would leave -1
#define P3D_FIRST_HIT(obj)                                                                                   \
  do {                                                                                                       \
    if (EARLY_HIT) { if (P.hit_id && !(LIT != 0 && up.halo)) P.hit_id[(size_t)r * P.w + c] = (obj); }        \
    else first_hit = (obj);                                                                                  \
  } while (0)
        // a later pass of an accumulated frame goes on from the running sum and first hit the passes before it left
        if (AA && LIT == 0 && P.sample_begin > 0 && (SUB == 1 || sub == 0)) {
          const size_t k = (size_t)r * P.w + c;
          color = f3(P.accum_sum[3 * k], P.accum_sum[3 * k + 1], P.accum_sum[3 * k + 2]);
          first_hit = P.accum_hit[k];
          if (SUB == 4) {
            shared.colour[0][px] = color.x; shared.colour[1][px] = color.y; shared.colour[2][px] = color.z;
            shared.first_hit[px] = first_hit;
          }
        }
        if (SUB == 1 && !AA) {
          for (int si = 0; si < SPP; ++si) {
            for (int sj = 0; sj < SPP; ++sj) {
#include "whitted_sample.inc"
              color = color + result;
            }
          }
        } else if (SUB == 1) {  // samples [sample_begin, sample_end) in sample order
          int si = (int)P.sample_begin / SPP, sj = (int)P.sample_begin - si * SPP;
          for (int s = (int)P.sample_begin; s < (int)P.sample_end; ++s) {
#include "whitted_sample.inc"
            color = color + result;
            if (++sj == SPP) { sj = 0; ++si; }
          }
        } else {
          // Lanes of one wave wait for each other here (full ring, lane 0 waiting for the last samples of its pixel),
          // so the loop is wave-uniform — a ballot every lane takes part in decides its end, a waiting lane sits out
          // the rest of the trip — exactly as in pt_kernel (where a per-lane `continue` got split off as an inner loop).
          const uint32_t s_end = P.sample_end;  // one past the last sample of this launch
          const unsigned long long trips_max = P.debug_trip_bound ? (unsigned long long)P.debug_trip_bound : (unsigned long long)(s_end - P.sample_begin) * 2ull + 1024ull;
          uint32_t trips_left = trips_max > 0xffffffffull ? 0xffffffffu : (uint32_t)trips_max;
          const uint32_t spp_magic = (uint32_t)((0x100000000ull + (unsigned)SPP - 1) / (unsigned)SPP);
          bool done = false, holding = false;
          int s = 0;
          while (true) {
            if (trips_left-- == 0) {  // backstop: the pixel would be written with samples missing -> the call fails
              if (!done) atomicOr(P.status, kHoErrTrips);
              done = true;
            }
            if (__ballot(!done) == 0) break;
            if (done) continue;
            if (sub == 0) {  // add finished samples to the pixel colour, strictly in sample order
              uint32_t na = shared.next_add[px];
              if (na < s_end && shared.tag[na % kPtRing][px] == na + 1) {
                F3 sum = f3(shared.colour[0][px], shared.colour[1][px], shared.colour[2][px]);
                do {
                  const int k = (int)(na % kPtRing);
                  sum = sum + f3(shared.radiance[k][0][px], shared.radiance[k][1][px], shared.radiance[k][2][px]);
                  ++na;
                } while (na < s_end && shared.tag[na % kPtRing][px] == na + 1);
                shared.colour[0][px] = sum.x; shared.colour[1][px] = sum.y; shared.colour[2][px] = sum.z;
                shared.next_add[px] = na;
              }
            }
            if (!holding) {
              s = (int)__hip_atomic_fetch_add(&shared.next_start[px], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
              holding = true;
            }
            if ((uint32_t)s >= s_end) {  // nothing left to start: finished, except lane 0 while samples remain to be added
              done = sub != 0 || shared.next_add[px] >= s_end;
              continue;
            }
            if ((uint32_t)s >= shared.next_add[px] + kPtRing) continue;  // wait for room in the ring
            holding = false;
            const int si = (int)__umulhi((uint32_t)s, spp_magic);  // s / SPP (exact: s * SPP < 2^32, SPP >= 2)
            const int sj = s - si * SPP;
#include "whitted_sample.inc"
            if (s == 0) shared.first_hit[px] = first_hit;
            ring_post(shared, px, s, result);
          }
          if (sub == 0) {
            color = f3(shared.colour[0][px], shared.colour[1][px], shared.colour[2][px]);
            first_hit = shared.first_hit[px];
          }
        }
#undef P3D_FIRST_HIT
        if (AA && LIT == 0 && P.accum_sum && (SUB == 1 || sub == 0)) {  // the running sum and first hit for the next pass
          const size_t k = (size_t)r * P.w + c;
          P.accum_sum[3 * k] = color.x; P.accum_sum[3 * k + 1] = color.y; P.accum_sum[3 * k + 2] = color.z;
          P.accum_hit[k] = first_hit;
        }
        if (AA) color = color / (float)P.sample_end;  // main.cpp:800 (sample_end = SPP * SPP on a frame's last pass)
#ifdef P3D_PT_PROFILE
        PT_REGION(8)
        prof.flush();
#endif

        if ((SUB == 1 || sub == 0) && !(LIT != 0 && up.halo)) {  // SUB == 4: lane 0 of the pixel holds its colour
          const size_t k = (size_t)r * P.w + c;
          if (P.rgb) {
            P.rgb[3 * k] = color.x; P.rgb[3 * k + 1] = color.y; P.rgb[3 * k + 2] = color.z;
          }
          if (!EARLY_HIT && P.hit_id) P.hit_id[k] = first_hit;
          if (P.rgb8) store_rgb8(P.rgb8 + 3 * k, color, P.gamma);
        }

#ifndef P3D_ABL_NO_RECORDS  // (timing ablation only: pass 1 keeps no records, the frame is the per-pixel one)
        if (LIT == 1) {  // what this unit leaves behind (slot 0), whether it touched the stack, its first closest hit
          uint32_t meta = 0;
          if (unit_touched) {
            uint32_t n = (uint32_t)st.sp;
            if (n > H.cap) { atomicOr(P.status, kHoErrLeftoverCap); n = H.cap; }
            leave_n = n;
            meta = n | kMetaTouched;
            atomicOr(&H.touched[unit >> 5], 1u << (unit & 31u));
          }
          H.meta[unit] = meta;
          H.meta0[unit] = meta;  // pass 1's record, never changed by a repair (what the tile launch of round 0 reads of its predecessors)
        }
#endif
        if (LIT != 0 && STATS) {
          if (up.halo) ct.clear();  // a halo pixel is rendered for its leftover, it is not a pixel of this tile
          store_unit_counters<STATS>(H, unit, ct, unit_ch0, P.stats);
        }
        if (REDO) {  // a changed leftover goes to the unit's other slot and sends the successor to the next round
          const uint32_t meta = H.meta[unit];
          const uint32_t cur = (meta >> 16) & 1u, cnt = meta & 0xffffu;
          uint32_t n = (uint32_t)st.sp;
          if (n > H.cap) { atomicOr(P.status, kHoErrLeftoverCap); n = H.cap; }
          bool same = n == cnt;
          const uint32_t old_at = (same && n) ? leftover_at(H, cur, unit) : 0u;
          for (uint32_t e = 0; same && e < n; ++e) {
            const uint2 a = H.entries[old_at + e], b = stack_read<SPILL>(st, (int)e);
            same = a.x == b.x && a.y == b.y;
          }
          if (!same) {
            leave_n = n;
            leave_slot = cur ^ 1u;
            leave_succ = true;
            H.meta[unit] = n | (leave_slot << 16) | kMetaTouched;
          }
        }
      }
#ifdef P3D_ABL_NO_RECORDS
      if (REDO) {
#else
      if (LIT != 0) {  // every lane: room in the leftover pool (one atomic per wave), then the entries
#endif
        const uint32_t at = leftover_alloc(H, leave_n, leave_slot, unit, P.status, LIT == 1 && !LDS);
        if (at != kNoUnit) {
          for (uint32_t e = 0; e < leave_n; ++e) H.entries[at + e] = stack_read<SPILL>(st, (int)e);
        } else if (leave_n) {  // pool full: the call fails (status); the records must still not point anywhere
          leave_n = 0;
          H.meta[unit] = (leave_slot << 16) | kMetaTouched;
        }
        if (REDO && leave_succ) {
          const int succ = handoff_succ(H, unit);
          if (succ >= 0) handoff_append(list_out, n_out_p, H.list_cap, P.status, make_uint4((uint32_t)succ, unit, (leave_slot << 16) | leave_n, 1u));
        }
      }
      if (LIT != 2) break;
    }
    if (LIT != 2 || !H.persistent) break;
    // next round of the persistent workgroup: what was written becomes the work list; the one just done is emptied
    __threadfence();
    if (lane == 0) __hip_atomic_store(n_in_p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    uint4* tl = list_in; list_in = list_out; list_out = tl;
    uint32_t* tn = n_in_p; n_in_p = n_out_p; n_out_p = tn;
  }
  if (STATS && LIT == 0) flush_stats<STATS>(ct, P.stats);  // LITERAL: ucount_reduce_kernel
  if (LIT < 2 && !halo_block) record_tile_cost(P, tx, ty, t_begin);
  P3D_TL_END()
  P3D_EC_END(LIT)
}

}  // namespace p3d
