// capi_frame.hpp — the frame launcher: the tile-schedule cache and FrameLaunch, whose steps enqueue what a FramePlan
// (capi_frame_plan.hpp) says with the kernels capi_dispatch.hpp chooses; the frame, adaptive-pass and feature entry points
// each compose the steps they need
#pragma once
#include "capi_dispatch.hpp"

namespace {

constexpr uint32_t kWfHistWords = kWfBins + 32;  // bin counts of one level + the total, padded to a 128-byte multiple
#ifndef P3D_REDO_LANES
#define P3D_REDO_LANES 64
#endif
// List entries per wave of the first work-list launch (the units rendered again: cfg2 9 995 unrelated deep pixels).
// Fewer entries per wave make that launch shorter when the frame is alone on the chip (round 2, profiles/r02/experiments/
// README.md §7: 4 per wave 130 µs, 32 per wave 160 µs), but every one of those waves holds a slot and issues for ~100 µs
// whatever the number of its active lanes, and with other frames in flight that is what counts.  Round 3, final kernels,
// one box, cfg2 with four frames in flight (1 000-step / 20-step loops) and one frame alone:
//    8 per wave  24.7 k / 23.8 k Mrays/s, 0.333 ms      32 per wave  36.9 k / 31.6 k, 0.337 ms
//   16 per wave  32.0 k / 29.5 k,         0.332 ms      64 per wave  38.9 k / 34.0 k, 0.348 ms
// P3D_REDO_LANES in the environment overrides it.
inline uint32_t redo_lanes() { static const uint32_t v = (uint32_t)env_int("P3D_REDO_LANES", P3D_REDO_LANES, 1, 64); return v; }
// list entries per wave of the round-1 launch (successors to re-check; P3D_ROUND1_LANES overrides)
inline uint32_t round1_lanes() { static const uint32_t v = (uint32_t)env_int("P3D_ROUND1_LANES", 64, 1, 64); return v; }
// workgroups of the round-1 work-list launch (P3D_LIST_BLOCKS overrides)
inline uint32_t list_blocks() { static const uint32_t v = (uint32_t)env_int("P3D_LIST_BLOCKS", 256, 1); return v; }
#ifdef P3D_ABLATION  // timing experiments only (profiles/r04/experiments): stages of the literal frame left out, frames WRONG
// P3D_ABL_SKIP: 1 = no check launch, 2 = no redo launch (round 0), 4 = no round 1 launch, 8 = round 1 launched on an empty list
inline uint32_t abl_skip() { static const uint32_t v = (uint32_t)env_int("P3D_ABL_SKIP", 0); return v; }
#else
constexpr uint32_t abl_skip() { return 0; }
#endif
constexpr uint32_t kPoolEntriesPerUnit = 8;  // compact hand-off records: pool entries per unit of the tile
constexpr size_t kSchedCacheEntries = 16;
constexpr uint32_t kSchedMinTiles = 8192;  // LDS-staged scenes: with fewer tiles than ~2 per wave slot nearly all start at once anyway
constexpr uint32_t kSchedMinTilesL2 = 256;  // scenes traversed from L2: a wave lives a millisecond, the order matters from a few hundred tiles

// What one pass of an adaptive frame (p3d_adaptive) needs besides the plan: the list the pass renders and the resolve /
// decide / compact launch behind it.
struct AdaptPass {
  PtAdaptParams k;
  AdaptResolveParams r;
  uint32_t resident;  // workgroups the device holds at once (the grid of pt_adaptive_kernel at most)
};

// Looks up the schedule for the launch described by (cfg, P).  Known key: P.sched is set.  New
// key: P.tile_cost is set so that this launch (in frame order) records the costs, and *fresh
// points at the entry, to be completed by schedule_finish() right after the launch.
int schedule_lookup(p3d_scene* s, const p3d_config* cfg, bool pt, RenderParams& P, hipStream_t st, SchedEntry** fresh) {
  *fresh = nullptr;
  SchedEntry key;
  key.accel = cfg->accel; key.aa = cfg->antialiasing ? 1 : 0; key.spp = cfg->antialiasing ? cfg->spp_sqrt : 1; key.pt = pt ? 1 : 0; key.tiles_x = P.tiles_x; key.tiles_y = P.tiles_y;
  key.max_depth = P.max_depth; key.x0 = P.x0; key.y0 = P.y0; key.w = P.w; key.h = P.h;
  key.stripe_h = P.stripe_h; key.stripe_stride = P.stripe_stride;
  for (SchedEntry& c : s->sched)
    if (c.built && c.same_key(key)) {
      if (c.built_on != st) P3D_HIP(hipStreamWaitEvent(st, c.ready, 0));
      c.last_use = ++s->sched_clock;
      P.sched = (const uint32_t*)c.sched.p;
      return P3D_OK;
    }
  SchedEntry* e = nullptr;
  for (SchedEntry& c : s->sched)
    if (!e && !c.built && c.same_key(key)) e = &c;
  if (e) {  // voided by p3d_scene_refit_device (void_schedules): recorded again in the memory it holds, nothing freed
  } else if (s->sched.size() < kSchedCacheEntries) {
    s->sched.emplace_back();
    e = &s->sched.back();
  } else {  // recycle the least recently used entry once the work queued with it has drained
    e = &s->sched[0];
    for (SchedEntry& c : s->sched)
      if (!c.built || c.last_use < e->last_use) e = &c;
    P3D_HIP(hipDeviceSynchronize());
  }
  e->built = false;
  const uint32_t n = P.tiles_x * P.tiles_y;
  if (int rc = e->cost.ensure((size_t)n * sizeof(uint32_t))) return rc;
  if (int rc = e->sched.ensure((size_t)n * sizeof(uint32_t))) return rc;
  if (!e->ready) P3D_HIP(hipEventCreateWithFlags(&e->ready, hipEventDisableTiming));
  e->accel = key.accel; e->aa = key.aa; e->spp = key.spp; e->pt = key.pt; e->tiles_x = key.tiles_x; e->tiles_y = key.tiles_y; e->max_depth = key.max_depth; e->x0 = key.x0; e->y0 = key.y0;
  e->w = key.w; e->h = key.h; e->stripe_h = key.stripe_h; e->stripe_stride = key.stripe_stride;
  P.tile_cost = (uint32_t*)e->cost.p;
  *fresh = e;
  return P3D_OK;
}

int schedule_finish(p3d_scene* s, SchedEntry* e, uint32_t n_tiles, hipStream_t st) {
  hipLaunchKernelGGL(sched_build_kernel, dim3(1), dim3(kSchedBuildThreads), 0, st, (const uint32_t*)e->cost.p, n_tiles, (uint32_t*)e->sched.p);
  if (hipError_t err = hipGetLastError(); err != hipSuccess)
    return fail(P3D_ERR_NO_DEVICE, std::string("schedule kernel launch: ") + hipGetErrorString(err));
  P3D_HIP(hipEventRecord(e->ready, st));
  e->built = true;
  e->built_on = st;
  e->last_use = ++s->sched_clock;
  return P3D_OK;
}

int finish_stats(p3d_scene* s, hipStream_t st, p3d_stats* stats, bool literal) {
  P3D_HIP(hipEventRecord(s->ev1, st));
  P3D_HIP(hipEventSynchronize(s->ev1));
  float ms = 0;
  P3D_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  unsigned long long h[kNumStats];
  P3D_HIP(hipMemcpy(h, s->d_stats, sizeof(h), hipMemcpyDeviceToHost));
  std::memset(stats, 0, sizeof(*stats));
  stats->kernel_ms = ms;
  if (literal) {
    float a = 0;
    float head = 0;
    P3D_HIP(hipEventElapsedTime(&a, s->ev_p1, s->ev_mid));
    P3D_HIP(hipEventElapsedTime(&head, s->ev0, s->ev_mid));
    stats->pass1_ms = a;
    stats->handoff_ms = ms - head;
  }
  stats->rays_primary = h[kRaysPrimary]; stats->rays_shadow = h[kRaysShadow]; stats->rays_reflect = h[kRaysReflect];
  stats->rays_refract = h[kRaysRefract]; stats->rays_bounce = h[kRaysBounce]; stats->rays_light = h[kRaysLight];
  stats->node_tests = h[kNodeTests]; stats->sphere_tests = h[kSphereTests]; stats->tri_tests = h[kTriTests];
  stats->box_tests = h[kBoxTests]; stats->plane_tests = h[kPlaneTests]; stats->shaded_hits = h[kShadedHits];
  stats->pixels = h[kPixels]; stats->max_stack = h[kMaxStack];
  if (literal) {
    uint32_t c[kHoNumCounters];
    P3D_HIP(hipMemcpy(c, s->ho_counters.p, sizeof(c), hipMemcpyDeviceToHost));
    static const bool print_handoff = getenv("P3D_PRINT_HANDOFF") != nullptr;  // (profiles/tools/ab/lists_probe.py)
    if (print_handoff) std::fprintf(stderr, "handoff: checked %u redone %u rounds %u pool %u lists A %u B %u C %u D %u check_n %u round0 %u round1 %u\n", c[kHoChecked], c[kHoRedone], c[kHoRounds], c[kHoPoolTop], c[kHoListA], c[kHoListB], c[kHoListC], c[kHoListD], c[kHoCheckN], c[kHoRound0], c[kHoRound1]);
    stats->handoff_checked = c[kHoChecked]; stats->handoff_redone = c[kHoRedone]; stats->handoff_rounds = c[kHoRounds] + (c[kHoRound0] ? 1 : 0) + (c[kHoRound1] ? 1 : 0);
  }
  return check_status(s, true);
}

// What every render call checks before it touches the device: the tile lies in the image, the options are known.
int check_frame(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile) {
  if (int rc = check_accel(s, cfg->accel)) return rc;
  const DevCamera& cam = s->dev.cam;
  if (cam.res_x <= 0 || cam.res_y <= 0) return fail(P3D_ERR_INVALID, "scene has no camera");
  const int sh = tile->stripe_h > 0 ? tile->stripe_h : 1, ss = tile->stripe_h > 0 ? tile->stripe_stride : 1;
  if (tile->w <= 0 || tile->h <= 0 || tile->x0 < 0 || tile->y0 < 0 || ss < 1 || tile->x0 + tile->w > cam.res_x)
    return fail(P3D_ERR_INVALID, "tile outside the image");
  {
    const int last = tile->h - 1;
    const long long ylast = (long long)tile->y0 + (long long)(last / sh) * sh * ss + (last % sh);
    if (ylast >= cam.res_y) return fail(P3D_ERR_INVALID, "tile rows outside the image");
  }
  if (cfg->integrator > P3D_PATHTRACE || cfg->sample_mode > P3D_SAMPLE_TENT) return fail(P3D_ERR_INVALID, "bad integrator / sample_mode");
  if (cfg->tile_order > P3D_TILE_ORDER_FRAME) return fail(P3D_ERR_INVALID, "bad tile_order");
  if (cfg->stack_mode > P3D_STACK_PER_PIXEL) return fail(P3D_ERR_INVALID, "bad stack_mode");
  if (cfg->chain_launch > P3D_CHAIN_PER_LEVEL) return fail(P3D_ERR_INVALID, "bad chain_launch");
  if (cfg->debug_view > P3D_DEBUG_DEPTH_MAP) return fail(P3D_ERR_INVALID, "bad debug_view");
  if (cfg->handoff_records > P3D_HANDOFF_DENSE) return fail(P3D_ERR_INVALID, "bad handoff_records");
  if (cfg->max_depth < 0 || cfg->max_depth > 1024) return fail(P3D_ERR_INVALID, "max_depth out of range");
  if (cfg->antialiasing && (cfg->spp_sqrt == 0 || cfg->spp_sqrt > 1024)) return fail(P3D_ERR_INVALID, "spp_sqrt out of range");
  if (cfg->soft_shadows && !cfg->antialiasing)
    ;  // light replication (main.cpp:725-745) is a host-side scene edit: p3d_host_scene_replicate_lights
  if (cfg->accel == P3D_ACCEL_GRID && s->dev.n_objs == 0) return fail(P3D_ERR_UNSUPPORTED, "grid over an empty scene");
  if (cfg->skybox && !s->has_sky) return fail(P3D_ERR_INVALID, "config asks for SKYBOX but no cubemap was supplied (p3d_scene_set_skybox)");
  return P3D_OK;
}

// One render call in flight on the host: the plan, the kernel parameters and what the steps hand each other.  begin()
// plans and prepares; the entry points below enqueue the steps their mode needs; end() closes the call.
struct FrameLaunch {
  p3d_scene* s;
  const p3d_config* cfg;
  const p3d_tile* tile;
  hipStream_t st;
  p3d_stats* stats;
  float* d_rgb = nullptr;       // outputs of the tile; accum_*: the running sums and first hits of p3d_accum / p3d_adaptive
  int32_t* d_hit = nullptr;
  uint8_t* d_rgb8 = nullptr;
  float* accum_sum = nullptr;
  int32_t* accum_hit = nullptr;
  FramePlan plan{};
  RenderParams P{};
  bool want_counts = false;
  // the hit_stack hand-off (setup_handoff)
  uint4* ho_list[4] = {nullptr, nullptr, nullptr, nullptr};
  uint32_t* ho_counters = nullptr;
  size_t touched_bytes = 0;
  uint32_t counter_words = 0, wf_seg_cap = 0, halo_blocks = 0;
  std::vector<const uint32_t*> band_sched;  // the tile schedule pass 1 used for each band: the tile launch of round 0 takes the same order
  bool on_tail = false;

  FrameLaunch(p3d_scene* s_, const p3d_config* cfg_, const p3d_tile* tile_, void* hip_stream, p3d_stats* stats_)
      : s(s_), cfg(cfg_), tile(tile_), st((hipStream_t)hip_stream), stats(stats_) {}

  // Plan (every refusal of the plan comes before device memory is touched), kernel parameters, scratch, hand-off records
  int begin(FrameMode mode, uint32_t sample_begin, uint32_t sample_end, uint32_t resident) {
    P3D_HIP(hipSetDevice(s->device));
    s->last_status = 0;
    if (int rc = wait_for_tail(s, st)) return rc;  // the scene's scratch is in use until the previous frame's tail has run (p3d_scene_set_tail_stream)
    if (int rc = plan_frame(scene_facts(s), cfg, tile, sample_begin, sample_end, mode, resident, plan)) return rc;
    if (plan.per_level && s->root_stale) {  // the ray queue's bins are cut from the root box, which p3d_scene_refit_device left on the device
      P3D_HIP(hipStreamSynchronize(st));    // (the scene's stream rules put that refit in front of this frame on `st`)
      if (int rc = refresh_root_box(s)) return rc;
    }
    want_counts = stats && cfg->collect_stats;
    fill_params(sample_begin, sample_end);
    if (int rc = ensure_scratch()) return rc;
    if (plan.literal || plan.per_level)
      if (int rc = setup_handoff()) return rc;
    return P3D_OK;
  }

  void fill_params(uint32_t sample_begin, uint32_t sample_end) {
    P.sc = s->dev;
    P.blob = s->d_blob; P.blob_f4 = plan.lds_scene ? plan.stage_hi - plan.stage_lo : 0; P.stage_lo = plan.stage_lo;
    P.off_nodes = s->off_nodes; P.off_bgeom = s->off_bgeom; P.off_ogeom = s->off_ogeom;
    P.off_normals = s->off_normals; P.off_mats = s->off_mats; P.off_lights = s->off_lights;
    P.max_depth = cfg->max_depth; P.spp_sqrt = cfg->spp_sqrt; P.antialiasing = cfg->antialiasing;
    P.depth_of_field = cfg->depth_of_field; P.sample_disk = cfg->sample_disk; P.soft_shadows = cfg->soft_shadows;
    P.sample_mode = cfg->sample_mode; P.light_side = cfg->light_side; P.gamma = cfg->gamma; P.seed = cfg->seed;
    P.skybox = cfg->skybox ? 1u : 0u;
    P.debug_view = cfg->debug_view;
    P.stripe_h = tile->stripe_h > 0 ? tile->stripe_h : 0; P.stripe_stride = plan.ss;
    P.stats = s->d_stats;
    P.status = s->d_status;
    P.debug_trip_bound = s->dbg.trip_bound;
    P.stack_cap = (int32_t)plan.cap;
    P.stack_spills = plan.lds_spill ? 1u : 0u;
    P.lds_scene_f4 = P.blob_f4;
    P.sample_begin = sample_begin;
    P.sample_end = sample_end;
    P.tile_w_shift = plan.tpw == 8 ? 3 : 2;
    P.tile_h_shift = plan.tph == 8 ? 3 : 2;
  }

  int ensure_scratch() {
    if (int rc = s->levels.ensure(plan.levels_bytes)) return rc;
    if (int rc = s->spill.ensure(plan.spill_bytes)) return rc;
    if (int rc = s->deferred.ensure(plan.deferred_bytes)) return rc;
    P.levels = (float4*)s->levels.p;
    P.spill = (uint2*)s->spill.p;
    P.deferred = (float4*)s->deferred.p;
    return P3D_OK;
  }

  // ---- P3D_STACK_LITERAL: per-unit records of the hit_stack hand-off (csrc/handoff.hpp) ----
  int setup_handoff() {
    Handoff& H = P.hand;
    const bool literal = plan.literal, per_level = plan.per_level, lds_scene = plan.lds_scene;
    const int sh = plan.sh, ss = plan.ss;
    const uint32_t per = s->bvh_max_depth > 1 ? s->bvh_max_depth - 1 : 1;
    // Rows whose predecessor in the frame is not the end of the tile row above start a chain of their own (halo_find_kernel)
    const bool full_width = tile->x0 == 0 && tile->w == s->dev.cam.res_x;
    std::vector<uint8_t> chain((size_t)tile->h, 0);
    bool any_chain = false;
    if (literal) {
      long long y_prev = -2;
      for (int r = 0; r < tile->h; ++r) {
        const long long y = (long long)tile->y0 + (long long)(r / sh) * sh * ss + (r % sh);
        chain[r] = r == 0 ? !(tile->x0 == 0 && y == 0) : !(full_width && y == y_prev + 1);
        any_chain = any_chain || chain[r];
        y_prev = y;
      }
    }
    H.halo = any_chain ? kHaloChain : 0;
    H.row_units = (uint32_t)tile->w + H.halo;
    H.rows = (uint32_t)tile->h;
    if ((uint64_t)H.rows * H.row_units >= 0xffffffffull) return fail(P3D_ERR_CAPACITY, "tile too large for the hit_stack hand-off");
    H.n_units = H.rows * H.row_units;
    // what a pixel can leave behind: the entries its last shading point's feelers left (Q2), one tree path per light
    H.cap = std::max<uint32_t>(1, std::min<uint32_t>(plan.bound, s->dev.n_lights * per));
    if (H.cap > 0xffffu) return fail(P3D_ERR_CAPACITY, "hit_stack leftover bound exceeds 65535 entries (lights x tree depth)");
    // leftover records: a pool with 8 entries per unit on average and an offset table (compact), or the worst case of
    // every unit (dense: the per-level launches rewrite a unit's record level by level; p3d_config.handoff_records)
    H.dense = (per_level || cfg->handoff_records == P3D_HANDOFF_DENSE) ? 1u : 0u;
    uint64_t pool_entries = H.dense ? (uint64_t)2 * H.cap * H.n_units : s->dbg.leftover_pool ? s->dbg.leftover_pool : std::max<uint64_t>(1u << 16, (uint64_t)kPoolEntriesPerUnit * H.n_units);
    if (!H.dense) pool_entries = std::min<uint64_t>(pool_entries, (uint64_t)2 * H.cap * H.n_units);  // never more than dense would take
    if (pool_entries > 0xffffffffull) return fail(P3D_ERR_CAPACITY, "hit_stack hand-off records exceed 2^32 entries: render the frame in smaller tiles or use P3D_STACK_PER_PIXEL");
    H.pool_cap = (uint32_t)pool_entries;
    if (int rc = s->ho_entries.ensure((size_t)pool_entries * sizeof(uint2))) return rc;
    if (!H.dense)
      if (int rc = s->ho_where.ensure((size_t)2 * H.n_units * sizeof(uint32_t))) return rc;
    if (int rc = s->ho_meta.ensure((size_t)2 * H.n_units * 4)) return rc;  // meta | meta0 (pass 1's copy)
    if (int rc = s->ho_first.ensure((size_t)H.n_units * sizeof(float4))) return rc;
    if (int rc = s->ho_first_sample.ensure(cfg->antialiasing ? (size_t)H.n_units * 4 : 16)) return rc;
    touched_bytes = ((size_t)H.n_units / 32 + 2) * 4;
    if (int rc = s->ho_touched.ensure(touched_bytes)) return rc;
    if (int rc = s->ho_lists.ensure((size_t)4 * H.n_units * sizeof(uint4))) return rc;
    if (!H.dense && !lds_scene)  // the check launch's work list (handoff.hpp Handoff::check_list)
      if (int rc = s->ho_check.ensure((size_t)H.n_units * sizeof(uint32_t))) return rc;
    // hand-off counters in the first 128-byte line, then one line per (chain level, queue segment) of the per-level launches
    // ... and the bin counts of every level's ray queue
    counter_words = 32 + (per_level ? ((uint32_t)cfg->max_depth + 1) * (kWfSegments * kWfCounterStride + kWfHistWords) : 0);
    if (int rc = s->ho_counters.ensure((size_t)counter_words * sizeof(uint32_t))) return rc;
    if (per_level) {
      wf_seg_cap = H.n_units / 4 + 4096;  // a segment takes the rays of every 8th workgroup: twice its fair share
      if (int rc = s->wf_rays.ensure((size_t)kWfSegments * wf_seg_cap * 2 * sizeof(float4))) return rc;
      if (int rc = s->wf_keys.ensure((size_t)kWfSegments * wf_seg_cap * sizeof(uint32_t))) return rc;
      if (int rc = s->wf_sorted.ensure((size_t)H.n_units * 2 * sizeof(float4))) return rc;
      if (int rc = s->wf_final.ensure((size_t)H.n_units * sizeof(float4))) return rc;
    }
    H.entries = (uint2*)s->ho_entries.p;
    H.where = (uint32_t*)s->ho_where.p;
    H.meta = (uint32_t*)s->ho_meta.p;
    H.meta0 = H.meta + H.n_units;
    H.first = (float4*)s->ho_first.p;
    H.first_sample = (uint32_t*)s->ho_first_sample.p;
    H.touched = (uint32_t*)s->ho_touched.p;
    H.row_chain = nullptr;
    H.halo_pix = nullptr;
    if (any_chain) {
      if (int rc = s->ho_row_chain.ensure((size_t)tile->h)) return rc;
      if (int rc = s->ho_halo_pix.ensure((size_t)tile->h * kHaloChain * 4)) return rc;
      H.row_chain = (const uint8_t*)s->ho_row_chain.p;
      H.halo_pix = (const uint32_t*)s->ho_halo_pix.p;
    }
    if (literal && want_counts) {  // per-unit counters: a unit rendered again replaces its first pass (handoff.hpp)
      if (int rc = s->ho_ucount.ensure((size_t)(kNumStats + kCh0Counters) * H.n_units * sizeof(uint32_t))) return rc;
      H.ucount = (uint32_t*)s->ho_ucount.p;
      H.uch0 = H.ucount + (size_t)kNumStats * H.n_units;
    }
    H.list_cap = H.n_units;
    H.count = want_counts ? 1u : 0u;
    H.max_rounds = std::min<uint32_t>(H.n_units + 2, 4096);  // a chain of n units is exact after n rounds at the latest; measured: 2.  Beyond the cap: P3D_ERR_CAPACITY
    if (s->dbg.max_rounds) H.max_rounds = s->dbg.max_rounds;
    for (int i = 0; i < 4; ++i) ho_list[i] = (uint4*)s->ho_lists.p + (size_t)i * H.n_units;
    ho_counters = (uint32_t*)s->ho_counters.p;
    H.counters = ho_counters;
    H.pool_top = ho_counters + kHoPoolTop;
    // (scenes traversed from global memory only: over an LDS-staged scene 64 unrelated pixels per wave diverge for longer than
    // the few neighbouring lanes of a tile's wave take, cfg2 literal loop 37.3 k -> 35.1 k Mrays/s; 100k triangles 15.9 -> 15.5 ms)
    H.check_list = (H.dense || lds_scene) ? nullptr : (uint32_t*)s->ho_check.p;
    H.check_n = ho_counters + kHoCheckN;
    return P3D_OK;
  }

  // LITERAL, tile with chain rows: the chain flags and the pixels in front of every chain row are a function of the tile
  // and of what shapes the primary rays (the scene is fixed; p3d_scene_set_camera clears the key when the camera
  // changes): worked out by two launches on this stream when any of that changes, kept otherwise (the frames of a
  // sequence find them ready).
  int halo_memo() {
    const Handoff& H = P.hand;
    if (!plan.literal || !H.halo) return P3D_OK;
    const DevCamera& cam = s->dev.cam;
    halo_blocks = (H.rows * kHaloChain + kBlock - 1) / kBlock;
    const uint32_t max_chain = s->dbg.halo_chain ? std::min<uint32_t>(s->dbg.halo_chain, kHaloChain) : kHaloChain;
    const std::vector<int64_t> key = {tile->x0, tile->y0, tile->w, tile->h, tile->stripe_h, tile->stripe_stride, cam.res_x, cam.res_y,
                                      cfg->antialiasing ? 1 : 0, cfg->antialiasing ? (int64_t)cfg->spp_sqrt : 1, (int64_t)cfg->seed,
                                      cfg->sample_mode, cfg->depth_of_field, cfg->sample_disk, max_chain, (int64_t)(intptr_t)st};
    if (key == s->ho_chain_key) return P3D_OK;
    RowChainParams C{(uint8_t*)s->ho_row_chain.p, s->d_halo_verdict, tile->h, tile->x0, tile->y0, tile->w, cam.res_x, plan.sh, plan.ss};
    hipLaunchKernelGGL(row_chain_kernel, dim3(((uint32_t)tile->h + 255) / 256), dim3(256), 0, st, C);
    P3D_HIP(hipGetLastError());
    P.x0 = tile->x0; P.y0 = tile->y0; P.row0 = 0; P.w = tile->w; P.h = tile->h;
    const uint32_t find_window = 8;  // LDS entries of the one traversal at a time each workgroup runs; deeper ones in P.spill
    hipLaunchKernelGGL(halo_find_kernel, dim3(H.rows), dim3(kHaloFindThreads), (size_t)find_window * kBlock * sizeof(uint2), st, P,
                       (uint32_t*)s->ho_halo_pix.p, s->d_halo_verdict, max_chain, s->has_spheres ? 1u : 0u, find_window, H.rows * kBlock);
    P3D_HIP(hipGetLastError());
    s->ho_chain_key = key;
    return P3D_OK;
  }

  // One clear launch at the head of the frame: statistics, counters, touched bits
  int clear() {
    const bool literal = plan.literal, per_level = plan.per_level;
    if (!(literal || per_level || stats)) return P3D_OK;
    ClearParams C{};
    if (stats) { C.p[0] = (uint32_t*)s->d_stats; C.n[0] = kNumStats * 2; }
    if (literal || per_level) { C.p[1] = ho_counters; C.n[1] = counter_words; }
    if (literal) { C.p[2] = (uint32_t*)s->ho_touched.p; C.n[2] = (uint32_t)(touched_bytes / 4); }
    if (literal && P.hand.halo) { C.halo_verdict = s->d_halo_verdict; C.status = s->d_status; }
    // (not LITERAL: the clear is there for the counters only and stays outside kernel_ms)
    const uint32_t words = std::max(C.n[0], std::max(C.n[1], C.n[2]));
    hipLaunchKernelGGL(clear_kernel, dim3(std::min<uint32_t>(256, (words + 255) / 256)), dim3(256), 0, st, C);
    P3D_HIP(hipGetLastError());
    if (stats && !literal) P3D_HIP(hipEventRecord(s->ev0, st));
    return P3D_OK;
  }

  // Everything behind pass 1 is a chain of short dependent launches (p3d_scene_set_tail_stream): on a stream of its own it
  // does not hold up the launches the caller enqueues behind this frame on `st` - other scenes' pass 1.  Not with `stats`
  // (the frame is timed as a whole on one stream).
  int to_tail() {
    if (on_tail || !plan.literal || !s->tail_stream || stats || s->tail_stream == st) return P3D_OK;
    P3D_HIP(hipEventRecord(s->ev_tail_go, st));
    P3D_HIP(hipStreamWaitEvent(s->tail_stream, s->ev_tail_go, 0));
    st = s->tail_stream;
    on_tail = true;
    return P3D_OK;
  }

  // Adaptive passes and feature launches: the whole tile in one launch of `blocks` workgroups, in frame order
  void whole_tile(uint32_t blocks) {
    P.x0 = tile->x0; P.y0 = tile->y0; P.w = tile->w; P.h = tile->h; P.row0 = 0;
    P.tiles_x = plan.tiles_x; P.tiles_y = plan.total_bands; P.xcd_chunk = plan.xcd_chunk;
    P.sched = nullptr; P.tile_cost = nullptr;
    P.tile_blocks = blocks;
    P.level_stride = blocks * kBlock;
  }

  // The listed pixels over the whole tile in one launch, then resolve / decide / compact (adaptive.hpp)
  int adaptive_pass(const AdaptPass& ap) {
    whole_tile(plan.adapt_blocks);
    P.rgb = nullptr; P.hit_id = nullptr; P.rgb8 = nullptr;
    P.accum_sum = accum_sum; P.accum_hit = accum_hit;
    hipError_t e = enqueue(adaptive_kernel(cfg->accel, plan, want_counts), plan.adapt_blocks, kBlock, plan.lds_bytes, st, P, ap.k);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(adapt_resolve_kernel, dim3((ap.r.slots + kAdaptResolveThreads - 1) / kAdaptResolveThreads), dim3(kAdaptResolveThreads), 0, st, ap.r);
      e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("adaptive pass launch: ") + hipGetErrorString(e));
    return P3D_OK;
  }

  // The primary rays of every pixel of the tile, one launch (features.hpp)
  int feature_launch(const FeatureParams& F) {
    whole_tile(plan.feat_blocks);
    const size_t feat_lds = (size_t)P.lds_scene_f4 * sizeof(float4) + (size_t)stack_lds_f4(plan.stack_mode, plan.cap) * sizeof(float4);
    const hipError_t e = enqueue(feature_kernel_of(cfg->accel, plan), plan.feat_blocks, kBlock, feat_lds, st, P, F);
    if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("feature launch: ") + hipGetErrorString(e));
    return P3D_OK;
  }

  // The per-level chain: level 0 over the tiles (+ halo chains), then one launch per chain level over the queue the level
  // above wrote, then the fold.  The grid of a queue launch is fixed (the queue length is only known on the device): 24
  // waves per CU, each taking every (grid / 8)-th chunk of 64 entries of its segment.
  hipError_t level_chain(uint32_t blocks) {
    hipError_t e = hipSuccess;
    P.wf_seg_cap = wf_seg_cap;
    P.wf_final = (float4*)s->wf_final.p;
    P.level_stride2 = P.hand.n_units;
    uint32_t* wf_counters = ho_counters + 32;
    uint32_t* wf_hists = wf_counters + (size_t)((uint32_t)cfg->max_depth + 1) * kWfSegments * kWfCounterStride;
    const uint32_t queue_blocks = std::min<uint32_t>(kWfSegments * 768, std::max<uint32_t>(kWfSegments, (plan.max_threads / kBlock) / kWfSegments * kWfSegments));
    P.wf_ray_out = (float4*)s->wf_rays.p; P.wf_ray_in = (float4*)s->wf_rays.p;
    P.wf_key_out = (uint32_t*)s->wf_keys.p; P.wf_key_in = (const uint32_t*)s->wf_keys.p;
    P.wf_sorted = (float4*)s->wf_sorted.p;
    P.wf_cell_origin = F3{s->root_min[0], s->root_min[1], s->root_min[2]};
    auto scale = [&](int a) { const float w = s->root_max[a] - s->root_min[a]; return w > 0 ? (float)kWfCellsPerAxis / w : 0.0f; };
    P.wf_cell_scale = F3{scale(0), scale(1), scale(2)};
    for (int level = 0; level <= cfg->max_depth && e == hipSuccess; ++level) {
      P.wf_level = (uint32_t)level;
      P.wf_n_out = wf_counters + (size_t)level * kWfSegments * kWfCounterStride;
      P.wf_hist = wf_hists + (size_t)level * kWfHistWords;
      P.wf_total = level ? wf_hists + (size_t)(level - 1) * kWfHistWords + kWfBins : nullptr;
      const uint32_t g = level == 0 ? blocks : queue_blocks;
      P.level_stride = g * kBlock;
      // (wf_level_kernel keeps its shading state in registers: no cold area behind its stack window)
      const size_t wf_lds = plan.lds_bytes - (plan.cold_lds ? (size_t)kColdDwords * kBlock * sizeof(float) : 0);
      e = enqueue(level_kernel(want_counts, plan.literal), g, kBlock, wf_lds, st, P);
      if (e == hipSuccess && level < cfg->max_depth) {  // put the child rays in bin order for the next level
        hipLaunchKernelGGL(wf_scan_kernel, dim3(1), dim3(1024), 0, st, P.wf_hist);
        P.wf_n_in = P.wf_n_out;
        hipLaunchKernelGGL(wf_scatter_kernel, dim3(kWfSegments * 128), dim3(256), 0, st, P, (const uint32_t*)(P.wf_hist + kWfBins));
        e = hipGetLastError();
      }
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(wf_fold_kernel, dim3(((uint32_t)tile->w * (uint32_t)tile->h + 255) / 256), dim3(256), 0, st, P);
      e = hipGetLastError();
    }
    P.level_stride = blocks * kBlock;
    return e;
  }

  // One launch of a LITERAL frame with the frame's staging, stack and LDS
  hipError_t literal_launch(LiteralStep step, uint32_t blocks) {
    return enqueue(literal_kernel(step, plan.lds_scene, plan.lds_spill, s->zero_weight_reflections, cfg->antialiasing != 0, want_counts),
                   blocks, kBlock, plan.lds_bytes, st, P);
  }

  // The tile in launches of bands_per_launch tile bands.  pass 0 = the render launches (LITERAL: pass 1 of the hand-off,
  // everything on an empty stack); pass 1 = LITERAL only: the check (or check + repair) launches over the tiles.
  int bands(int pass) {
    Handoff& H = P.hand;
    const bool literal = plan.literal, lds_scene = plan.lds_scene;
    const int sh = plan.sh, ss = plan.ss;
    const uint32_t tp = plan.tph, tiles_x = plan.tiles_x, total_bands = plan.total_bands, bands_per_launch = plan.bands_per_launch;
    for (uint32_t band0 = 0; band0 < total_bands; band0 += bands_per_launch) {
      const uint32_t nb = std::min(bands_per_launch, total_bands - band0);
      const int row0 = (int)(band0 * tp);
      const int rows = std::min<int>((int)(nb * tp), tile->h - row0);
      // a chunk starts at local row row0; stripes make the image row a function of the LOCAL
      // row of the whole tile, so pass the tile origin and offset the outputs instead
      P.x0 = tile->x0; P.w = tile->w;
      P.h = rows;
      P.row0 = row0;
      if (P.stripe_h > 0) {
        if (row0 % sh != 0 && nb != total_bands) return fail(P3D_ERR_UNSUPPORTED, "stripe_h must divide the tile bands when a frame is split into several launches");
        P.y0 = tile->y0 + (row0 / sh) * sh * ss + (row0 % sh);
      } else {
        P.y0 = tile->y0 + row0;
      }
      P.tiles_x = tiles_x; P.tiles_y = nb;
      P.xcd_chunk = plan.xcd_chunk;
      P.sched = nullptr;
      P.tile_cost = nullptr;
      SchedEntry* fresh = nullptr;
      if (pass == 0 && plan.sched_ok && tiles_x * nb >= (lds_scene ? kSchedMinTiles : kSchedMinTilesL2))
        if (int rc = schedule_lookup(s, cfg, plan.pt, P, st, &fresh)) return rc;
      if (pass == 0) band_sched.push_back(fresh ? (const uint32_t*)fresh->sched.p : P.sched);
      if (pass == 1 && plan.repair_tiles) P.sched = band_sched[band0 / bands_per_launch];  // (built on this stream by now: schedule_finish)
      const uint32_t tile_blocks = plan.blocks_for(tiles_x * nb);
      const uint32_t blocks = tile_blocks + (band0 == 0 ? halo_blocks : 0);  // the halo chains ride on the first launch
      P.tile_blocks = tile_blocks;
      P.level_stride = blocks * kBlock;
      const size_t off = (size_t)row0 * tile->w;
      P.rgb = d_rgb ? d_rgb + 3 * off : nullptr;
      P.hit_id = d_hit ? d_hit + off : nullptr;
      P.rgb8 = d_rgb8 ? d_rgb8 + 3 * off : nullptr;
      P.accum_sum = accum_sum ? accum_sum + 3 * off : nullptr;
      P.accum_hit = accum_hit ? accum_hit + off : nullptr;
      hipError_t e = hipSuccess;
      if (plan.per_level && pass == 0) {
        e = level_chain(blocks);
      } else if (literal) {
        if (pass == 1) { H.list_out = ho_list[plan.repair_tiles ? 1 : 0]; H.n_out = ho_counters + kHoListA + (plan.repair_tiles ? 1 : 0); }
        e = literal_launch(pass == 0 ? LiteralStep::Pass1 : (plan.repair_tiles ? LiteralStep::RepairTiles : LiteralStep::CheckTiles), blocks);
      } else {
        e = enqueue(frame_kernel(cfg->accel, plan, cfg->antialiasing != 0, want_counts), blocks, kBlock, plan.lds_bytes, st, P);
      }
      if (e != hipSuccess) {
        if (fresh) fresh->built = false;
        return fail(P3D_ERR_NO_DEVICE, std::string("kernel launch: ") + hipGetErrorString(e));
      }
      if (fresh)
        if (int rc = schedule_finish(s, fresh, tiles_x * nb, st)) return rc;
    }
    return P3D_OK;
  }

  // The rounds behind pass 1, over the whole tile.  Round 0: the units whose first closest hit changes under the predecessor's
  // pass-1 leftover are rendered again - over the tiles, by bands(1) (LDS-staged scenes: it wrote list B directly), or
  // from list A, which the check launch fills (scenes traversed from global memory) - and put the successors of the units whose
  // own leftover changed on list B.  Round 1: a light launch re-traces the first closest hits of list B's units on the new
  // leftovers and passes the rare one that changes on to list C; one persistent workgroup renders list C again and iterates
  // whatever is left after that - almost never anything - to the fixed point (C -> D -> C ...).
  int handoff_rounds() {
    Handoff& H = P.hand;
    const uint32_t max_threads = plan.max_threads;
    P.x0 = tile->x0; P.w = tile->w; P.h = tile->h; P.row0 = 0; P.y0 = tile->y0;
    P.rgb = d_rgb; P.hit_id = d_hit; P.rgb8 = d_rgb8;
    P.sched = nullptr; P.tile_cost = nullptr;
    // workgroups of a work-list launch: far fewer units than pixels are expected (grid-stride loop for the rest)
    // (one workgroup per 64 pixels at most: with few list entries per wave a list of 1 % of the pixels still gets a wave
    // per chunk; workgroups without a chunk leave at once)
    const uint32_t wide = std::max<uint32_t>(1, std::min<uint32_t>(max_threads / kBlock, std::max<uint32_t>(64, H.n_units / kBlock)));
    if (H.check_list && !(abl_skip() & 1u)) {  // the check of round 0 over the units pass 1 announced: writes list A
      H.list_out = ho_list[0]; H.n_out = ho_counters + kHoListA;
      P.level_stride = wide * kBlock;
      P.tile_blocks = wide;
      const hipError_t e = literal_launch(LiteralStep::CheckList, wide);
      if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("hand-off check launch: ") + hipGetErrorString(e));
    }
    for (int round = 0; round < 3; ++round) {
      if ((round == 0 && (abl_skip() & 2u)) || (round > 0 && (abl_skip() & 4u))) continue;
      if (round == 0 && plan.repair_tiles) continue;  // the tile launch of bands(1) was round 0 and wrote list B
      H.list_in = ho_list[round]; H.n_in = ho_counters + kHoListA + round;
      H.list_out = ho_list[round + 1]; H.n_out = ho_counters + kHoListA + round + 1;
      H.persistent = round == 2 ? 1u : 0u;
      // (the persistent workgroup starts with round 1's own repairs, list C, before it goes on to the rounds that follow)
      H.round_base = (uint32_t)(round == 2 ? 1 : round);
      // round 0 renders unrelated deep pixels again; entries per wave: see P3D_REDO_LANES above
      H.lanes = round == 0 ? redo_lanes() : (round == 1 ? round1_lanes() : kBlock);
      // (round >= 1 works through the successors of units whose leftover changed, a few thousand list entries at most: a small
      // grid with a grid-stride loop - 16 384 workgroups that find nothing take 25 us to come and go, a lone frame waits for them)
      // (round 0 over list A - scenes traversed from global memory - rarely has anything on it: 4 096 workgroups and a
      // grid-stride loop instead of one workgroup per 64 pixels that comes only to find the list empty, 16 us for a 2048x2048 frame)
      const uint32_t blocks = round == 2 ? 1u : (round == 1 ? std::min(wide, list_blocks()) : std::min<uint32_t>(wide, 4096u));
      P.level_stride = blocks * kBlock;
      P.tile_blocks = blocks;
      const uint32_t real_cap = H.list_cap;
      if (abl_skip() & 8u) H.list_cap = 0;  // (ablation: the launch happens, every workgroup finds an empty list)
      const hipError_t e = literal_launch(round == 1 ? LiteralStep::CheckEntries : LiteralStep::RepairList, blocks);
      H.list_cap = real_cap;
      if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("hand-off kernel launch: ") + hipGetErrorString(e));
    }
    if (want_counts) {
      hipLaunchKernelGGL(ucount_reduce_kernel, dim3(256), dim3(256), 0, st, H, (uint32_t)tile->w, s->d_stats);
      P3D_HIP(hipGetLastError());
    }
    return P3D_OK;
  }

  int end() {
    if (on_tail) {
      P3D_HIP(hipEventRecord(s->ev_tail_done, st));
      s->tail_pending = true;
    }
    if (stats) return finish_stats(s, st, stats, plan.literal);
    return P3D_OK;
  }
};

// The render path of p3d_render_tile_device (a whole frame: samples [0, SPP^2), no accumulator) and of p3d_accum_render_device
// (samples [sample_begin, sample_end) of an anti-aliased frame whose running sums and first hits live in accum_sum /
// accum_hit).  The sample range only reaches the anti-aliased sample loops; everything else is the same frame.
int render_frame(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, float* d_rgb, int32_t* d_hit, uint8_t* d_rgb8,
                 void* hip_stream, p3d_stats* stats, uint32_t sample_begin, uint32_t sample_end, float* accum_sum, int32_t* accum_hit) {
  if (int rc = check_frame(s, cfg, tile)) return rc;
  FrameLaunch f(s, cfg, tile, hip_stream, stats);
  f.d_rgb = d_rgb; f.d_hit = d_hit; f.d_rgb8 = d_rgb8; f.accum_sum = accum_sum; f.accum_hit = accum_hit;
  if (int rc = f.begin(kFrame, sample_begin, sample_end, 0)) return rc;
  const bool literal = f.plan.literal;
  if (stats && literal) P3D_HIP(hipEventRecord(s->ev0, f.st));  // kernel_ms of a LITERAL frame is the whole frame: halo search (when not memoised) and clear included
  if (int rc = f.halo_memo()) return rc;
  if (int rc = f.clear()) return rc;
  if (stats && literal) P3D_HIP(hipEventRecord(s->ev_p1, f.st));  // pass1_ms: the speculative pass on its own
  if (int rc = f.bands(0)) return rc;
  if (literal) {
    if (stats) P3D_HIP(hipEventRecord(s->ev_mid, f.st));
    if (int rc = f.to_tail()) return rc;
    // (with a check list the check runs over pass 1's list, once for the whole tile: handoff_rounds)
    if (!(abl_skip() & 1u) && !f.P.hand.check_list)
      if (int rc = f.bands(1)) return rc;
    if (int rc = f.handoff_rounds()) return rc;
  }
  return f.end();
}

// One pass of p3d_adaptive_render_device (path tracer only): the listed pixels, then the resolve of the tile behind them
int render_adaptive_pass(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, void* hip_stream, p3d_stats* stats, uint32_t sample_begin,
                         uint32_t sample_end, float* accum_sum, int32_t* accum_hit, const AdaptPass& ap) {
  if (int rc = check_frame(s, cfg, tile)) return rc;
  FrameLaunch f(s, cfg, tile, hip_stream, stats);
  f.accum_sum = accum_sum; f.accum_hit = accum_hit;
  if (int rc = f.begin(kAdaptivePass, sample_begin, sample_end, ap.resident)) return rc;
  if (int rc = f.clear()) return rc;
  if (int rc = f.adaptive_pass(ap)) return rc;
  return f.end();
}

// p3d_render_features_device: the primary rays of samples [0, samples) into the feature buffers, the frame's staging and stack
int render_feature_buffers(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, void* hip_stream, uint32_t samples, const FeatureParams& F) {
  FrameLaunch f(s, cfg, tile, hip_stream, nullptr);
  if (int rc = f.begin(kFeatures, 0, samples, 0)) return rc;
  if (int rc = f.feature_launch(F)) return rc;
  return f.end();
}

// The host-buffer form of a render call: device copies of the outputs asked for in the scene's out_* buffers, the
// device form (always with stats: the call waits for the frame and reports what the device detected), copy back.
template <class Render>
int render_to_host(p3d_scene* s, size_t px, float* rgb, int32_t* hit_id, uint8_t* rgb8, p3d_stats* stats, Render&& render) {
  P3D_HIP(hipSetDevice(s->device));
  if (rgb) if (int rc = s->out_rgb.ensure(px * 3 * sizeof(float))) return rc;
  if (hit_id) if (int rc = s->out_hit.ensure(px * sizeof(int32_t))) return rc;
  if (rgb8) if (int rc = s->out_rgb8.ensure(px * 3)) return rc;
  p3d_stats local;
  if (int rc = render(rgb ? (float*)s->out_rgb.p : nullptr, hit_id ? (int32_t*)s->out_hit.p : nullptr, rgb8 ? (uint8_t*)s->out_rgb8.p : nullptr,
                      stats ? stats : &local))
    return rc;
  if (rgb) P3D_HIP(hipMemcpy(rgb, s->out_rgb.p, px * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (hit_id) P3D_HIP(hipMemcpy(hit_id, s->out_hit.p, px * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (rgb8) P3D_HIP(hipMemcpy(rgb8, s->out_rgb8.p, px * 3, hipMemcpyDeviceToHost));
  return P3D_OK;  // device-detected errors were turned into a return code by finish_stats()
}

// What p3d_accum and p3d_adaptive check before every pass, and stamp at create / reset.  T: p3d_accum or p3d_adaptive;
// `name`: the prefix of the messages
template <class T>
int check_pass(const T* a, uint32_t n, const char* prefix) {
  if (!a->failed && a->cam_gen == a->s->cam_gen && a->geom_gen == a->s->geom_gen && n != 0 && n <= a->total - a->done) return P3D_OK;
  const std::string name = prefix;  // (only a refusal formats anything)
  if (a->failed) return fail(P3D_ERR_INVALID, name + "_render: a previous pass failed; " + name + "_reset starts the frame again");
  if (a->cam_gen != a->s->cam_gen)
    return fail(P3D_ERR_INVALID, name + "_render: the scene's camera changed since the frame began; " + name + "_reset starts it again in the new view");
  if (a->geom_gen != a->s->geom_gen)
    return fail(P3D_ERR_INVALID, name + "_render: the scene's objects moved since the frame began; " + name + "_reset starts it again");
  return fail(P3D_ERR_INVALID, name + "_render: " + std::to_string(n) + " samples asked, " + std::to_string(a->total - a->done) +
                                   " of " + std::to_string(a->total) + " left (n must be at least 1)");
}
template <class T>
void restart_passes(T* a) {
  a->done = 0;
  a->failed = false;
  a->cam_gen = a->s->cam_gen;
  a->geom_gen = a->s->geom_gen;
}

}  // namespace

extern "C" {

int p3d_render_tile_device(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, float* d_rgb, int32_t* d_hit,
                           uint8_t* d_rgb8, void* hip_stream, p3d_stats* stats) {
  if (!s || !cfg || !tile) return fail(P3D_ERR_INVALID, "p3d_render_tile_device: null argument");
  const uint32_t samples = cfg->antialiasing ? cfg->spp_sqrt * cfg->spp_sqrt : 1u;
  return render_frame(s, cfg, tile, d_rgb, d_hit, d_rgb8, hip_stream, stats, 0, samples, nullptr, nullptr);
}

int p3d_scene_set_tail_stream(p3d_scene* s, void* hip_stream) {
  if (!s) return fail(P3D_ERR_INVALID, "p3d_scene_set_tail_stream: null scene");
  P3D_HIP(hipSetDevice(s->device));
  if (s->tail_pending) {  // (a frame may still be running on the old tail stream)
    P3D_HIP(hipEventSynchronize(s->ev_tail_done));
    s->tail_pending = false;
  }
  s->tail_stream = (hipStream_t)hip_stream;
  return P3D_OK;
}

int p3d_scene_join(p3d_scene* s, void* hip_stream, int host_wait) {
  if (!s) return fail(P3D_ERR_INVALID, "p3d_scene_join: null scene");
  if (!s->tail_pending) return P3D_OK;  // nothing of this scene runs anywhere but on the streams the caller gave it
  P3D_HIP(hipSetDevice(s->device));
  if (host_wait) P3D_HIP(hipEventSynchronize(s->ev_tail_done));
  else P3D_HIP(hipStreamWaitEvent((hipStream_t)hip_stream, s->ev_tail_done, 0));
  return P3D_OK;
}

int p3d_scene_status(p3d_scene* s) {
  if (!s) return fail(P3D_ERR_INVALID, "p3d_scene_status: null argument");
  P3D_HIP(hipSetDevice(s->device));
  P3D_HIP(hipDeviceSynchronize());
  if (int rc = refresh_root_box(s)) return rc;
  return check_status(s);
}

int p3d_render_tile(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, float* rgb, int32_t* hit_id, uint8_t* rgb8,
                    p3d_stats* stats) {
  if (!s || !cfg || !tile) return fail(P3D_ERR_INVALID, "p3d_render_tile: null argument");
  if (tile->w <= 0 || tile->h <= 0) return fail(P3D_ERR_INVALID, "empty tile");
  return render_to_host(s, (size_t)tile->w * tile->h, rgb, hit_id, rgb8, stats, [&](float* d_rgb, int32_t* d_hit, uint8_t* d_rgb8, p3d_stats* st) {
    int rc = p3d_render_tile_device(s, cfg, tile, d_rgb, d_hit, d_rgb8, nullptr, st);
    bool retried = false;
    if (rc == P3D_ERR_CAPACITY && cfg->handoff_records == P3D_HANDOFF_COMPACT && (s->last_status & kHoErrLeftoverCap)) {
      p3d_config dense = *cfg;  // the leftover pool was too small for this frame: once more with room for the worst case
      dense.handoff_records = P3D_HANDOFF_DENSE;
      rc = p3d_render_tile_device(s, &dense, tile, d_rgb, d_hit, d_rgb8, nullptr, st);
      retried = true;
    }
    if (stats && rc == P3D_OK) stats->handoff_dense_retry = retried ? 1 : 0;  // the frame was rendered twice (and the dense records allocated)
    return rc;
  });
}

}  // extern "C"
