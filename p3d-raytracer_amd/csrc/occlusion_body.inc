// occlusion_body.inc — the body of occlusion_kernel, included into each of the kernels of that name (occlusion_query.hpp): `P` is
// the kernel's OcclusionParams, `filters` its source of filters (queries.hpp FilterParams or NoFilterSource).  Text and not a
// function, as nearest_k_body.inc: the unfiltered kernel holds no trace of a filter.
  static_assert(TEAM >= 1 && TEAM <= kBlock && (TEAM & (TEAM - 1)) == 0, "a team is a power of two of lanes within one wave");
  extern __shared__ float4 smem[];
  const uint32_t gid = blockIdx.x * kBlock + threadIdx.x;  // (the host refuses n x TEAM past 2^32)
  Stack st;
  query_stack_bind(st, smem, P.stack, gid);
  const uint32_t i = gid / TEAM, lane = threadIdx.x % TEAM;
  const bool in = i < P.n;
  const size_t row = in ? i : 0;  // (a team past the end reads point 0 and writes nothing)
  const unsigned long long team_mask = (TEAM == 64 ? ~0ull : ((1ull << (TEAM & 63)) - 1ull)) << (threadIdx.x - lane);
  Counters<false> ct;
  OcclusionFrame f;
  occlusion_load_frame(P.point, P.normal, row, P.bias, f);
  const float limit = P.max_dist ? P.max_dist[row] : INFINITY;
  const auto filter = filters.load((uint32_t)row, P.sc.n_objs);  // (one row per POINT: every lane of the team holds the same filter)
  const F3 origin = f3(f.origin[0], f.origin[1], f.origin[2]);
  uint32_t count = 0;
  F3 bent = f3(0, 0, 0);
  const uint32_t trips = (P.samples + (TEAM - 1)) / TEAM;  // (samples <= 2^32 - 1: the sum is taken in 64 bits)
  for (uint32_t trip = 0; trip < trips; ++trip) {
    const uint64_t k = (uint64_t)trip * TEAM + lane;
    const bool valid = in && k < P.samples;
    bool open = false;
    F3 d = f3(0, 0, 0);
    if (valid) {
      float dir[3];
      occlusion_direction(f, P.seed, P.point_offset + i, P.sample_begin + (uint32_t)k, dir);
      d = f3(dir[0], dir[1], dir[2]);
      RayS ray;
      ray_set(ray, origin, d);
      stack_clear(st);
      open = !(ACCEL == P3D_ACCEL_BVH ? bvh_segment_any(P.sc, st, ray, limit, filter, ct) : brute_segment_any(P.sc, ray, limit, filter, ct));
    }
    count += (uint32_t)__popcll(__ballot(valid && open) & team_mask);
    if (open) bent = bent + d;
  }
  if (P.bent) {
#pragma unroll
    for (int m = TEAM / 2; m >= 1; m >>= 1)
      bent = bent + f3(__shfl_xor(bent.x, m, kBlock), __shfl_xor(bent.y, m, kBlock), __shfl_xor(bent.z, m, kBlock));
  }
  if (in && lane == 0) {
    if (P.accumulate) {
      P.unoccluded[i] += count;
      if (P.bent) store_f3(P.bent, row, f3(P.bent[3 * row], P.bent[3 * row + 1], P.bent[3 * row + 2]) + bent);
    } else {
      P.unoccluded[i] = count;
      if (P.bent) store_f3(P.bent, row, bent);
    }
  }
