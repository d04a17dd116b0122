// handoff_kernels.hpp — the device side of the hit_stack hand-off (handoff.hpp has the records and the scans): where a unit
// lies in the image, the steps of the check (part 1; whitted_kernel's LIT modes are made of the same steps) and the kernels
// that only search or check (part 2).  Included by kernels.hpp between what every render kernel shares (RenderParams,
// stage_scene, tile_of_block, make_primary), which this file uses, and whitted_kernel, which uses part 1.

namespace p3d {

// ---------------------------------------------------------------------------
// Part 1: units and the steps of the check
// ---------------------------------------------------------------------------
// Where a unit of the hand-off (handoff.hpp) lies in the image: tile pixels and, in front of every row, the halo slots.
struct UnitPlace {
  int c, r, x, y;  // tile column / tile row (output index), image pixel
  bool halo;       // a frame pixel rendered only for what it leaves on the stack: no output
  bool valid;
};
__device__ __forceinline__ UnitPlace no_place() { return UnitPlace{0, 0, 0, 0, false, false}; }
// tile row -> image row; rows come in stripes of `sh` with `ss` stripes from one to the next (multi-GPU frames)
template <class T>
__device__ __forceinline__ T stripe_row(T y0, int r, int sh, int ss) { return y0 + (T)(r / sh) * sh * ss + (r % sh); }
__device__ __forceinline__ int image_row(const RenderParams& P, int r) {
  return stripe_row<int>(P.y0, r, P.stripe_h > 0 ? P.stripe_h : 1, P.stripe_h > 0 ? P.stripe_stride : 1);
}
__device__ __forceinline__ UnitPlace place_of_unit(const RenderParams& P, uint32_t unit) {
  const Handoff& H = P.hand;
  UnitPlace u;
  const uint32_t row = unit / H.row_units, j = unit - row * H.row_units;
  u.r = (int)row - P.row0;
  u.halo = j < H.halo;
  u.valid = true;
  if (u.halo) {
    const uint32_t fp = H.halo_pix[row * H.halo + j];
    u.valid = fp != kNoUnit;
    u.c = 0;
    u.x = (int)(fp % (uint32_t)P.sc.cam.res_x);
    u.y = (int)(fp / (uint32_t)P.sc.cam.res_x);
  } else {
    u.c = (int)(j - H.halo);
    u.x = P.x0 + u.c;
    u.y = image_row(P, u.r);
  }
  return u;
}
// pass 1 / check: the unit of a lane of a halo workgroup (8 chains of kHaloChain slots per wave)
__device__ __forceinline__ bool halo_unit_of_lane(const RenderParams& P, uint32_t lane, uint32_t& unit) {
  const Handoff& H = P.hand;
  const uint32_t slot = (blockIdx.x - P.tile_blocks) * kBlock + lane;
  const uint32_t row = slot / kHaloChain, j = slot % kHaloChain;
  if (H.halo == 0 || row >= H.rows || !H.row_chain[row]) return false;
  unit = row * H.row_units + j;
  return H.halo_pix[row * H.halo + j] != kNoUnit;
}
// pixel `px` of tile (tx, ty), a (1 << tws) x (1 << ths) block: its column and row in the launch; false: outside
__device__ __forceinline__ bool tile_pixel(const RenderParams& P, uint32_t tx, uint32_t ty, uint32_t tws, uint32_t ths, uint32_t px, int& c, int& r) {
  c = (int)((tx << tws) + (px & ((1u << tws) - 1u)));
  r = (int)((ty << ths) + (px >> tws));
  return px < (1u << (tws + ths)) && c < P.w && r < P.h;
}
__device__ __forceinline__ uint32_t unit_of_pixel(const RenderParams& P, int c, int r) {
  return (uint32_t)(P.row0 + r) * P.hand.row_units + P.hand.halo + (uint32_t)c;
}
// the unit of a lane of a launch over the tiles: a pixel of the workgroup's tile, or a halo slot in the workgroups behind them
__device__ __forceinline__ bool unit_of_lane(const RenderParams& P, bool halo_block, uint32_t tx, uint32_t ty, uint32_t tws, uint32_t ths,
                                             uint32_t lane, uint32_t& unit) {
  if (halo_block) return halo_unit_of_lane(P, lane, unit);
  int c, r;
  const bool in = tile_pixel(P, tx, ty, tws, ths, lane, c, r);
  unit = unit_of_pixel(P, c, r);
  return in;
}
// a list counter as the launch finds it, held to the list's capacity (an overflow was reported by whoever appended)
__device__ __forceinline__ uint32_t list_count(const uint32_t* n, uint32_t cap) {
  const uint32_t v = __hip_atomic_load(n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return v > cap ? cap : v;
}
// work-list entry {unit, predecessor, slot << 16 | entries, flags}: written by an earlier trip of a persistent workgroup, so not from a cache
__device__ __forceinline__ uint4 list_entry(const uint4* list, uint32_t i) {
  const uint32_t* e = reinterpret_cast<const uint32_t*>(list + i);
  return make_uint4(__hip_atomic_load(e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(e + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                    __hip_atomic_load(e + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), __hip_atomic_load(e + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

template <bool SPILL, class CT>
__device__ __forceinline__ void seed_stack(Stack& st, const Handoff& H, uint32_t pred, uint32_t slot_count, CT& ct) {
  stack_clear(st);
  const uint32_t n = slot_count & 0xffffu, slot = slot_count >> 16;
  const uint32_t at = n ? leftover_at(H, slot, pred) : 0u;
  for (uint32_t e = 0; e < n; ++e) {
    const uint2 v = H.entries[at + e];
    push<SPILL>(st, v.x, __uint_as_float(v.y), ct);
  }
}
// collect_stats under P3D_STACK_LITERAL (handoff.hpp: ucount / uch0).  The deepest stack goes straight to the global
// maximum: it is taken over everything that was traced, speculative passes included.
template <bool STATS>
__device__ __forceinline__ void store_unit_counters(const Handoff& H, uint32_t unit, const Counters<STATS>& ct, const uint32_t* ch0,
                                                    unsigned long long* stats) {
  if (!STATS) return;
  for (int s = 0; s < kNumStats; ++s)
    if (s != kMaxStack) H.ucount[(size_t)s * H.n_units + unit] = ct.get(s);
  for (int k = 0; k < kCh0Counters; ++k) H.uch0[(size_t)k * H.n_units + unit] = ch0[k];
  atomicMax(&stats[kMaxStack], (unsigned long long)ct.get(kMaxStack));
}
// a unit whose first closest hit was re-traced on a new leftover and came out the same: only that query's tests change
template <bool STATS>
__device__ __forceinline__ void replace_ch0_counters(const Handoff& H, uint32_t unit, const Counters<STATS>& cc, unsigned long long* stats) {
  if (!STATS) return;
  for (int k = 0; k < kCh0Counters; ++k) {
    const size_t at = (size_t)k * H.n_units + unit;
    const uint32_t now = cc.get(kNodeTests + k);
    H.ucount[(size_t)(kNodeTests + k) * H.n_units + unit] += now - H.uch0[at];
    H.uch0[at] = now;
  }
  atomicMax(&stats[kMaxStack], (unsigned long long)cc.get(kMaxStack));
}
// sum of the unit counters over the pixels of the tile (halo units are not pixels of the tile)
__global__ void __launch_bounds__(256) ucount_reduce_kernel(const Handoff H, uint32_t w, unsigned long long* stats) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t n_pix = w * H.rows;
  for (int s = 0; s < kNumStats; ++s) {
    if (s == kMaxStack) continue;
    unsigned long long v = 0;
    for (uint32_t p = i; p < n_pix; p += gridDim.x * 256) {
      const uint32_t unit = (p / w) * H.row_units + H.halo + (p % w);
      v += H.ucount[(size_t)s * H.n_units + unit];
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(&stats[s], v);
  }
}

__device__ __forceinline__ bool same_first(float4 a, float4 b) {
  return __float_as_uint(a.x) == __float_as_uint(b.x) && __float_as_uint(a.y) == __float_as_uint(b.y) &&
         __float_as_uint(a.z) == __float_as_uint(b.z) && __float_as_uint(a.w) == __float_as_uint(b.w);
}
// The first closest hit of a unit's first touching sample, traced on whatever the stack holds (bvh.cpp:198-276).
template <bool SPILL, bool VOTE, class CT>
__device__ __forceinline__ float4 first_closest_hit(const RenderParams& P, const DevScene& sc, Stack& st, int x, int y, uint32_t sample, CT& ct) {
  Rng rng;
  rng.state = 0; rng.inc = 1;
  const int SPP = P.antialiasing ? (int)P.spp_sqrt : 1;
  const int si = (int)sample / SPP, sj = (int)sample % SPP;
  if (P.antialiasing) rng.seed_stream(P.seed, (uint32_t)(y * sc.cam.res_x + x), sample);
  F3 o, d, Pn;
  make_primary(P, sc.cam, x, y, si, sj, rng, o, d);
  RayS ray;
  ray_set(ray, o, d);
  Geom g;
  const int obj = closest_hit<P3D_ACCEL_BVH, SPILL, VOTE>(sc, st, ray, Pn, g, ct);
  return obj < 0 ? make_float4(0.f, 0.f, 0.f, __int_as_float(-1)) : make_float4(Pn.x, Pn.y, Pn.z, __int_as_float(obj));
}
// The check of one unit whose stack was seeded with its predecessor's leftover: its first closest hit again.  true: the hit is what
// it was, so nothing the unit computes can differ (only that query's tests: the counters are replaced); false: render it again.
template <bool SPILL, bool VOTE, bool STATS>
__device__ __forceinline__ bool first_hit_unchanged(const RenderParams& P, const DevScene& sc, Stack& st, const UnitPlace& up, uint32_t unit, bool aa,
                                                    Counters<STATS>& ct) {
  const Handoff& H = P.hand;
  if (H.count) atomicAdd(&H.counters[kHoChecked], 1u);
  const float4 now = first_closest_hit<SPILL, VOTE>(P, sc, st, up.x, up.y, aa ? H.first_sample[unit] : 0u, ct);
  if (!same_first(now, H.first[unit])) return false;
  replace_ch0_counters<STATS>(H, unit, ct, P.stats);
  return true;
}

// ---------------------------------------------------------------------------
// Part 2: the chain in front of a row, and the launches that only check
// ---------------------------------------------------------------------------
// For every tile row that starts a chain of its own (its predecessor in the FRAME is not the end of the tile row above:
// first row of a stripe, any row of a sub-rectangle, a tile that does not start at the frame's first pixel): the frame
// pixels in front of the row whose leftovers have to be known for the row's first pixel to start on the right stack.
//
// A pixel "touches" the stack if the primary ray of one of its samples gets past the root test (bvh.cpp:203-205).  What
// the row starts on is the leftover of the last touching pixel before it, which depends on ITS predecessor's leftover,
// and so on back to the frame's first pixel - but only through the result of each pixel's first closest hit
// (handoff.hpp).  The chain can therefore be cut at a pixel whose first closest hit provably does not depend on the
// stack it finds.  The stale entries of a found stack are popped AFTER the query's own traversal and the popped
// subtrees are walked with the query's ray (bvh.cpp:256-265); that changes the result only if (a) one of the primitive
// tests it runs returns a hit nearer than the own traversal's, or (b) a sphere test re-normalises the ray's direction
// (scene.cpp:156, ray.h:16-18).  So a pixel is CERTIFIED if, after its own traversal on an empty stack,
//   (a) NO primitive of the scene - all of them are tested, whatever boxes they sit in - is hit nearer than tmin by the
//       ray as the traversal left it, and
//   (b) the scene has no sphere, or normalising that ray's direction once more leaves its bits unchanged (then every
//       further normalisation is the identity).
// Under (a) and (b) no sequence of stale subtree walks can change tmin, the hit or the direction, whatever the stack
// held: the pixel rendered on an empty stack is the pixel of the serial frame, its leftover included.  The kernel walks
// back from the row, takes the touching pixels most recent first, and stops at the first one it can certify (or at the
// frame's first touching pixel, whose stack IS empty); the pixels it collected are rendered in front of the row for
// their leftovers, the oldest on an empty stack, each next one checked against its predecessor's leftover like any
// other unit.  If `max_chain` (<= kHaloChain) pixels are collected without a certificate and an older touching pixel
// exists, the row cannot be started exactly: kHoErrHalo is raised and the call fails (P3D_ERR_CAPACITY) instead of
// returning a frame that is only probably right.
//
// One workgroup per row.  Every thread looks at one pixel of the kHaloFindThreads before the row; candidates are taken
// one at a time: wave 0 runs the own traversal (all lanes the same ray), all threads share the all-primitives test.
constexpr int kHaloFindThreads = 1024;
struct HaloFindShared {
  unsigned long long touched[kHaloFindThreads / kBlock];
  float tmin, dx, dy, dz;
  uint32_t settled, closer;
};
__device__ __forceinline__ bool pixel_first_touching_ray(const RenderParams& P, const NodeRec& root, long long f, RayS& ray) {
  const DevScene& sc = P.sc;
  const int res_x = sc.cam.res_x, SPP = P.antialiasing ? (int)P.spp_sqrt : 1;
  const int x = (int)(f % res_x), y = (int)(f / res_x);
  for (int s = 0; s < SPP * SPP; ++s) {
    Rng rng;
    rng.state = 0; rng.inc = 1;
    if (P.antialiasing) rng.seed_stream(P.seed, (uint32_t)(y * res_x + x), (uint32_t)s);
    F3 o, d;
    make_primary(P, sc.cam, x, y, s / SPP, s % SPP, rng, o, d);
    ray_set(ray, o, d);
    float t;
    if (aabb_intercepts(xyz(root.lo), xyz(root.hi), ray, t, false)) return true;
  }
  return false;
}
// Which rows of a tile start a chain of their own: a function of the tile alone, worked out on the launch stream so
// that two tiles queued on one stream cannot see each other's flags.  Also resets the verdict of the search that follows.
struct RowChainParams {
  uint8_t* chain;
  uint32_t* verdict;
  int32_t rows, x0, y0, w, res_x, sh, ss;
};
__global__ void __launch_bounds__(256) row_chain_kernel(const RowChainParams C) {
  const int r = (int)(blockIdx.x * 256 + threadIdx.x);
  if (r == 0) *C.verdict = 0;
  if (r >= C.rows) return;
  const long long y = stripe_row<long long>(C.y0, r, C.sh, C.ss);
  const bool full_width = C.x0 == 0 && C.w == C.res_x;
  C.chain[r] = r == 0 ? !(C.x0 == 0 && y == 0) : !(full_width && y == stripe_row<long long>(C.y0, r - 1, C.sh, C.ss) + 1);
}

__global__ void __launch_bounds__(kHaloFindThreads) halo_find_kernel(const RenderParams P, uint32_t* halo_pix, uint32_t* verdict, uint32_t max_chain,
                                                                     uint32_t has_spheres, uint32_t window, uint32_t backing_stride) {
  extern __shared__ float4 smem[];  // wave 0's node stack: window * 64 entries
  __shared__ HaloFindShared sh;
  const Handoff& H = P.hand;
  const uint32_t row = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (row >= H.rows || !H.row_chain[row]) return;
  const DevScene& sc = P.sc;
  const long long f0 = (long long)image_row(P, (int)row) * sc.cam.res_x + P.x0;  // the row's first pixel: search below it
  const NodeRec root = load_node(sc.nodes, 0);
  Counters<false> ct;
  uint32_t found = 0;
  bool certified = false, older_exists = false;
  for (long long base = f0; base > 0 && !certified && !older_exists; base -= kHaloFindThreads) {
    const long long f = base - 1 - (long long)tid;  // thread 0 looks at the most recent pixel
    RayS ray;
    const bool touched = f >= 0 && pixel_first_touching_ray(P, root, f, ray);
    const unsigned long long m = __ballot(touched);
    if (lane == 0) sh.touched[wave] = m;
    __syncthreads();
    for (uint32_t w = 0; w < kHaloFindThreads / kBlock && !certified && !older_exists; ++w) {
      unsigned long long mask = sh.touched[w];
      while (mask && !certified && !older_exists) {  // workgroup-uniform
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (found == max_chain) {  // the chain is full and here is a touching pixel it would still need
          older_exists = true;
          break;
        }
        const long long pix = base - 1 - (long long)(w * kBlock + (uint32_t)l);
        if (tid == 0) halo_pix[row * kHaloChain + (kHaloChain - 1 - found)] = (uint32_t)pix;
        ++found;
        // ---- certificate ----
        pixel_first_touching_ray(P, root, pix, ray);  // (every thread: the same ray)
        if (wave == 0) {
          Stack st;
          stack_bind(st, smem, 0, lane, (int)window, P.spill, backing_stride, blockIdx.x * kBlock + lane);
          F3 hp;
          Geom g;
          float tmin = FLT_MAX;
          RayS left;
          bvh_closest<true>(sc, st, ray, hp, g, ct, nullptr, &tmin, &left);
          if (lane == 0) {
            sh.tmin = tmin;
            sh.dx = left.d.x; sh.dy = left.d.y; sh.dz = left.d.z;
            sh.settled = same_bits(normalized(left.d), left.d) ? 1u : 0u;
            sh.closer = 0;
          }
        }
        __syncthreads();
        const float tmin = sh.tmin;
        const bool settled = sh.settled != 0;
        bool closer = false;
        if (settled || !has_spheres) {
          RayS r = ray;
          r.d = f3(sh.dx, sh.dy, sh.dz);
          r.inv = f3(1.0f / r.d.x, 1.0f / r.d.y, 1.0f / r.d.z);
          r.odd_inv = inv_is_odd(r.inv);
          r.settled = settled;  // a settled direction is returned as it is by the sphere test (ray.h:16-18 would give the same bits)
          for (uint32_t i = tid; i < sc.n_objs && !closer; i += kHaloFindThreads) {
            const Geom g = load_geom(sc.ogeom, i);
            float t;
            closer = intercepts(g, r, t, ct) && t < tmin;
          }
        }
        if (closer) sh.closer = 1;  // (benign race: every writer stores the same value)
        __syncthreads();
        certified = (settled || !has_spheres) && sh.closer == 0;
        __syncthreads();
      }
    }
    __syncthreads();
  }
  if (older_exists && !certified && tid == 0) atomicOr(verdict, kHoErrHalo);
  if (tid < kHaloChain - found) halo_pix[row * kHaloChain + tid] = kNoUnit;
}

// The check of round 0 of the hand-off for a whole launch: every unit that touched the stack and whose predecessor left something
// re-traces its first closest hit on that leftover; the units whose hit changed go on the work list of the redo launch.
template <bool LDS, bool SPILL, bool STATS = false>
__global__ void __launch_bounds__(kBlock) handoff_check_kernel(const RenderParams P) {
  extern __shared__ float4 smem[];
  uint32_t tx = 0, ty = 0;
  const bool halo_block = blockIdx.x >= P.tile_blocks;
  if (!halo_block && !tile_of_block(P, tx, ty)) return;
  const uint32_t lane = threadIdx.x;
  const Handoff& H = P.hand;
  uint32_t unit = 0;
  const bool active = unit_of_lane(P, halo_block, tx, ty, P.tile_w_shift, P.tile_h_shift, lane, unit);
  // which lanes have anything to re-trace is known before the scene is staged: most waves leave here
  int pred = -1;  // (twin: the LIT == 3 prologue of whitted_kernel, which reads meta0; as one function: more SGPRs here)
  uint32_t pm = 0;
  if (active && handoff_touched(H, unit)) {
    pred = handoff_pred(H, unit);
    if (pred >= 0) pm = H.meta[pred];
  }
  const bool need = (pm & 0xffffu) != 0;  // otherwise the predecessor left nothing: pass 1's empty stack was right
  if (__ballot(need) == 0) return;
  DevScene sc = P.sc;
  stage_scene<LDS, false>(sc, P, smem);  // (the hand-off exists for the BVH only)
  if (!need) return;
  Counters<STATS> ct;
  ct.clear();
  Stack st;
  stack_bind(st, smem, P.lds_scene_f4, lane, P.stack_cap, P.spill, P.level_stride, blockIdx.x * kBlock + lane);
  const UnitPlace up = place_of_unit(P, unit);
  const uint32_t slot_count = pm & 0x1ffffu;
  seed_stack<SPILL>(st, H, (uint32_t)pred, slot_count, ct);
  if (!first_hit_unchanged<SPILL, !LDS>(P, sc, st, up, unit, P.antialiasing, ct))
    handoff_append(H.list_out, H.n_out, H.list_cap, P.status, make_uint4(unit, (uint32_t)pred, slot_count, 0u));
}

// The same round over the list pass 1 wrote (Handoff::check_list: the units that left something): entry -> the unit that starts on
// that leftover (the next one that touched the stack) -> re-trace its first closest hit on it.  Every lane has work; one launch
// for the whole tile however many launches pass 1 took.
template <bool LDS, bool SPILL, bool STATS = false>
__global__ void __launch_bounds__(kBlock) handoff_check_list_kernel(const RenderParams P) {
  extern __shared__ float4 smem[];
  const Handoff& H = P.hand;
  const uint32_t n = list_count(H.check_n, H.n_units);
  if ((size_t)blockIdx.x * kBlock >= n) return;  // nothing on the list for this workgroup: leave before the scene is staged
  const uint32_t lane = threadIdx.x;
  DevScene sc = P.sc;
  stage_scene<LDS, false>(sc, P, smem);
  Stack st;
  stack_bind(st, smem, P.lds_scene_f4, lane, P.stack_cap, P.spill, P.level_stride, blockIdx.x * kBlock + lane);
  for (uint32_t chunk = blockIdx.x; (size_t)chunk * kBlock < n; chunk += gridDim.x) {
    const uint32_t i = chunk * kBlock + lane;
    if (i >= n) continue;
    const uint32_t pred = H.check_list[i];
    const uint32_t pm = H.meta[pred];
    const int succ = handoff_succ(H, pred);
    if (succ < 0 || (pm & 0xffffu) == 0) continue;  // nobody starts on it (end of a chain) / the pool was full (the call fails)
    const uint32_t unit = (uint32_t)succ;
    Counters<STATS> ct;
    ct.clear();
    const UnitPlace up = place_of_unit(P, unit);
    const uint32_t slot_count = pm & 0x1ffffu;
    seed_stack<SPILL>(st, H, pred, slot_count, ct);
    if (!first_hit_unchanged<SPILL, !LDS>(P, sc, st, up, unit, P.antialiasing, ct))
      handoff_append(H.list_out, H.n_out, H.list_cap, P.status, make_uint4(unit, pred, slot_count, 0u));
  }
}

// Round 1 of the hand-off as a LIGHT launch.  List B holds the successors of the units whose leftover changed in round 0; nearly
// all of them only need their first closest hit re-traced on the new leftover to find that nothing changes.  Until round 4 that was
// done by the work-list instantiation of whitted_kernel (LIT = 2: the whole Whitted chain, 128 VGPRs + scratch), whose few waves had
// to wait for a double-width slot among the other frames' pass-1 waves; this kernel only checks, and passes the rare entry whose hit
// does change (or that asks for no check) on to list C, which the persistent workgroup behind it renders again.
template <bool LDS, bool SPILL, bool STATS = false>
__global__ void __launch_bounds__(kBlock) handoff_check_entries_kernel(const RenderParams P) {
  extern __shared__ float4 smem[];
  const Handoff& H = P.hand;
  const uint32_t n = list_count(H.n_in, H.list_cap);
  if ((size_t)blockIdx.x * H.lanes >= n) return;  // nothing on the list for this workgroup: leave before the scene is staged
  const uint32_t lane = threadIdx.x;
  if (H.round_base >= H.max_rounds) {  // work left after the last round allowed: the frame is not the serial one
    if (lane == 0) atomicOr(P.status, kHoErrNoFixedPoint);
    return;
  }
  if (H.count && blockIdx.x == 0 && lane == 0) atomicOr(&H.counters[kHoRound1], 1u);
  DevScene sc = P.sc;
  stage_scene<LDS, false>(sc, P, smem);
  Stack st;
  stack_bind(st, smem, P.lds_scene_f4, lane, P.stack_cap, P.spill, P.level_stride, blockIdx.x * kBlock + lane);
  for (uint32_t chunk = blockIdx.x; (size_t)chunk * H.lanes < n; chunk += gridDim.x) {
    const uint32_t i = chunk * H.lanes + lane;
    if (lane >= H.lanes || i >= n) continue;
    const uint4 e = list_entry(H.list_in, i);  // {unit, predecessor, its slot and entries, flags}
    const UnitPlace up = place_of_unit(P, e.x);
    if (!up.valid) continue;
    if (e.w & 1u) {
      Counters<STATS> ct;
      ct.clear();
      seed_stack<SPILL>(st, H, e.y, e.z, ct);
      if (first_hit_unchanged<SPILL, !LDS>(P, sc, st, up, e.x, P.antialiasing, ct)) continue;
    }
    handoff_append(H.list_out, H.n_out, H.list_cap, P.status, make_uint4(e.x, e.y, e.z, 0u));  // rendered again by the launch behind this one
  }
}

}  // namespace p3d
