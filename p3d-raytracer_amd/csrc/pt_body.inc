// pt_body.inc — the body of the path tracer's kernels: included verbatim by pt_kernel (ADAPT = false: one wave per tile
// of the frame) and by pt_adaptive_kernel (ADAPT = true: groups of the pixel list until the list is used up).  A body
// included into each kernel rather than a shared __forceinline__ function: as a function, inlined, the existing
// pt_kernel instantiations did not compile to the instruction streams they had.  Not a header of its own.
// In scope: ACCEL, LDS, STATS, SUB, ADAPT, P (RenderParams), A (PtAdaptParams).
  extern __shared__ float4 smem[];
  constexpr uint32_t PPW = SUB == 4 ? 16 : 64;  // pixels per wave
  uint32_t tx, ty, n_list = 0;
  if constexpr (ADAPT) {
    n_list = *A.count;
    if (blockIdx.x * PPW >= n_list) return;  // (more waves than groups: leave before staging the scene)
  } else {
    if (!tile_of_block(P, tx, ty)) return;
  }
  P3D_TL_BEGIN()
  const unsigned long long t_begin = P.tile_cost ? wall_clock64() : 0;
  DevScene sc = P.sc;
  stage_scene<LDS, true>(sc, P, smem);

  constexpr int PT_STACK = LDS ? kStackLds8 : kStackWindow;  // (device_core.hpp: registers set this kernel's occupancy)
  const uint32_t lane = threadIdx.x;
  constexpr int TP = SUB == 4 ? 4 : 8;                       // tile edge in pixels
  const uint32_t px = SUB == 4 ? lane >> 2 : lane;           // pixel of the tile this lane works for
  const uint32_t sub = SUB == 4 ? lane & 3u : 0u;
  Counters<STATS> ct;
  if (STATS) reinterpret_cast<Counters<true>&>(ct).clear();
  Stack st;
  stack_bind(st, smem, P.lds_scene_f4, lane, P.stack_cap, P.spill, P.level_stride, blockIdx.x * kBlock + lane);
  Pending pend;
  pend.base = P.levels + (blockIdx.x * kBlock + lane);
  pend.stride = P.level_stride;
  pend.n = 0;
  // after the node stack (only allocated for SUB == 4); explicit LDS address space: a generic
  // pointer would compile to flat_load/flat_store, which are not ordered with the ds_* traffic
  LdsPtPixelShared& shared = *(LdsPtPixelShared*)(smem + P.lds_scene_f4 + stack_lds_f4(PT_STACK, P.stack_cap));
  for (;;) {  // ADAPT: one group of the list per trip; otherwise one trip
    uint32_t pix = 0;  // ADAPT: r * w + c of this lane's pixel
    bool listed = false;
    if constexpr (ADAPT) {
      uint32_t g = 0;
      if (lane == 0) g = atomicAdd(A.ticket, 1u);
      g = __shfl(g, 0, 64);
      if (g * PPW >= n_list) break;
      listed = g * PPW + px < n_list;
      if (listed) pix = A.list[g * PPW + px];
    }
    const int c = ADAPT ? (int)(pix % (uint32_t)P.w) : (int)(tx * TP + (px % TP));
    const int r = ADAPT ? (int)(pix / (uint32_t)P.w) : (int)(ty * TP + (px / TP));
    if (SUB == 4 && sub == 0) ring_init(shared, px, P.sample_begin);

    const bool active = ADAPT ? listed : (c < P.w && r < P.h);
    if (active) {
      const int x = P.x0 + c;
      const int y = image_row(P, r);
      const int SPP = (int)P.spp_sqrt;
      const uint32_t s_end = P.sample_end;  // one past the last sample of this launch (a whole frame: SPP * SPP)
      const int MAXD = P.max_depth;
      if (sub == 0) ct.add(kPixels);

      F3 color = f3(0, 0, 0);  // pixel accumulator (main.cpp:792)
      int first_hit = -1;
      int s = (int)P.sample_begin;  // SUB == 1: next sample to start; SUB == 4: the sample this lane is tracing
      int si = s / SPP, sj = s - si * SPP;
      const size_t k_out = (size_t)r * P.w + c;
      float s2 = 0.0f;  // ADAPT: S2 of the pixel (lane 0)
      if (P.sample_begin > 0 && sub == 0) {  // a later pass of an accumulated frame: go on from what the passes before it left
        color = f3(P.accum_sum[3 * k_out], P.accum_sum[3 * k_out + 1], P.accum_sum[3 * k_out + 2]);
        first_hit = P.accum_hit[k_out];
        if constexpr (ADAPT) s2 = A.sum_y2[k_out];
        if (SUB == 4) {
          shared.colour[0][px] = color.x; shared.colour[1][px] = color.y; shared.colour[2][px] = color.z;
          shared.first_hit[px] = first_hit;
        }
      }
      bool alive = false, in_sample = false, first_ray = false;
      Rng rng;
      RayS ray;
      F3 T = f3(1, 1, 1), L = f3(0, 0, 0);
      int depth = 0;

#ifdef P3D_PT_PROFILE
      RegionProf prof; prof.init();
#endif
      // SUB == 4 lets lanes of one wave wait for each other (a full ring, lane 0 waiting for the last
      // samples of its pixel).  A waiting lane must never spin on its own: the loop is therefore
      // wave-uniform — its exit test is a ballot every lane of the wave takes part in, once per trip —
      // and a waiting lane simply sits out the rest of the trip.  (With a per-lane `continue` as the
      // only way round, LLVM split the wait cycle off as an inner loop for the brute-force and grid
      // instantiations and the waiting lanes starved the working ones.)  The trip bound is a backstop:
      // no lane can need more trips than the pixel's whole sample set traced by one lane.
      const unsigned long long trips_max = P.debug_trip_bound ? (unsigned long long)P.debug_trip_bound
                                                              : (unsigned long long)(s_end - P.sample_begin) * (unsigned)(MAXD + 2) * 4ull + 1024ull;
      uint32_t trips_left = trips_max > 0xffffffffull ? 0xffffffffu : (uint32_t)trips_max;
      bool done = false, holding = false;
      const uint32_t spp_magic = (uint32_t)((0x100000000ull + (unsigned)SPP - 1) / (unsigned)SPP);
      while (true) {
        if (SUB == 4) {
          if (trips_left-- == 0) {  // the pixel would be written with samples missing: the call fails (P3D_ERR_CAPACITY)
            if (!done) atomicOr(P.status, kHoErrTrips);
            done = true;
          }
          if (__ballot(!done) == 0) break;
          if (done) continue;
        }
        PT_REGION(0)
        // lane 0 of a pixel adds its finished samples to the pixel colour, strictly in sample order:
        // whenever it is between two of its own samples, and every fourth trip while it traces one
        if (SUB == 4 && sub == 0 && (!alive || (trips_left & 3) == 0)) {
          uint32_t na = shared.next_add[px];
          if (na < s_end && shared.tag[na % kPtRing][px] == na + 1) {
            F3 sum = f3(shared.colour[0][px], shared.colour[1][px], shared.colour[2][px]);
            do {
              const int k = (int)(na % kPtRing);
              const F3 Lk = f3(shared.radiance[k][0][px], shared.radiance[k][1][px], shared.radiance[k][2][px]);
              sum = sum + Lk;
              if constexpr (ADAPT) s2 = s2 + luma_sq(Lk);
              ++na;
            } while (na < s_end && shared.tag[na % kPtRing][px] == na + 1);
            shared.colour[0][px] = sum.x; shared.colour[1][px] = sum.y; shared.colour[2][px] = sum.z;
            shared.next_add[px] = na;
          }
        }
        if (!alive) {
          PT_REGION(1)
          if (pend.n > 0) {  // resume the deferred reflection branch of a dielectric hit
            --pend.n;
            const float4 q0 = pend.base[(size_t)(pend.n * 3 + 0) * pend.stride], q1 = pend.base[(size_t)(pend.n * 3 + 1) * pend.stride],
                         q2 = pend.base[(size_t)(pend.n * 3 + 2) * pend.stride];
            ray_set(ray, f3(q0.x, q0.y, q0.z), f3(q0.w, q1.x, q1.y));
            T = f3(q1.z, q1.w, q2.x);
            depth = __float_as_int(q2.y);
            alive = true;
          } else {
            if (in_sample) {
              if (SUB == 4) {  // post the finished sample; its ring slot is free (guaranteed when it was handed out)
                ring_post(shared, px, s, L);
              } else {
                color = color + L;
                if constexpr (ADAPT) s2 = s2 + luma_sq(L);
              }
              in_sample = false;
            }
            if (SUB == 4) {
              // Take the pixel's next sample (one LDS atomic hands simultaneous takers distinct
              // tickets), then hold it until the ring has room for its radiance: the oldest sample
              // still being traced blocks the adder, and with it the slot kPtRing samples ahead.
              if (!holding) {
                s = (int)__hip_atomic_fetch_add(&shared.next_start[px], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                holding = true;
              }
              if ((uint32_t)s >= s_end) {  // nothing left to start: finished, except lane 0 while samples remain to be added
                done = sub != 0 || shared.next_add[px] >= s_end;
                continue;
              }
              if ((uint32_t)s >= shared.next_add[px] + kPtRing) continue;  // wait for room
              holding = false;
              si = (int)__umulhi((uint32_t)s, spp_magic);  // s / SPP (exact: s * SPP < 2^32)
              sj = s - si * SPP;
            } else if ((uint32_t)s == s_end) {
              break;
            }
            rng.seed_stream(P.seed, (uint32_t)(y * sc.cam.res_x + x), (uint32_t)s);
            stack_clear(st);
            F3 o, d;
            make_primary(P, sc.cam, x, y, si, sj, rng, o, d);
            ray_set(ray, o, d);
            ct.add(kRaysPrimary);
            T = f3(1, 1, 1);
            L = f3(0, 0, 0);
            depth = MAXD;
            first_ray = (s == 0);
            if (SUB == 1) {
              ++s;
              if (++sj == SPP) { sj = 0; ++si; }
            }
            alive = true;
            in_sample = true;
          }
        }
#include "pt_bounce.inc"  // one bounce: the body of Radiance, up to the ray of the next one
      }
      if (SUB == 4 && sub == 0) {
        color = f3(shared.colour[0][px], shared.colour[1][px], shared.colour[2][px]);
        first_hit = shared.first_hit[px];
      }
      if (P.accum_sum && sub == 0) {  // the running sum and first hit for the next pass
        P.accum_sum[3 * k_out] = color.x; P.accum_sum[3 * k_out + 1] = color.y; P.accum_sum[3 * k_out + 2] = color.z;
        P.accum_hit[k_out] = first_hit;
        if constexpr (ADAPT) A.sum_y2[k_out] = s2;
      }
      if constexpr (!ADAPT) {  // (adaptive passes: adapt_resolve_kernel writes the outputs of every pixel of the tile)
        if (P.antialiasing) color = color / (float)s_end;  // main.cpp:800 (s_end = SPP * SPP on a frame's last pass)

#ifdef P3D_PT_PROFILE
        PT_REGION(9)
        prof.flush();
#endif
        if (sub == 0) {  // SUB == 4: lane 0 of the pixel holds its colour
          const size_t k = k_out;
          if (P.rgb) {
            P.rgb[3 * k] = color.x; P.rgb[3 * k + 1] = color.y; P.rgb[3 * k + 2] = color.z;
          }
          if (P.hit_id) P.hit_id[k] = first_hit;
          if (P.rgb8) store_rgb8(P.rgb8 + 3 * k, color, P.gamma);
        }
      }
    }
    if constexpr (!ADAPT) break;
  }
  if (STATS) flush_stats<STATS>(ct, P.stats);
  if constexpr (!ADAPT) record_tile_cost(P, tx, ty, t_begin);
  P3D_TL_END()
