// occlusion_query.hpp — hemisphere occlusion at points in device memory (p3d_occlusion_device) and its rays written out
// (p3d_occlusion_rays_device).  occlusion_kernel casts the cosine-weighted rays of host/occlusion_rule.hpp from every point and
// counts those that the segment query of ray_query.hpp (bvh_segment_any, brute_segment_any) calls free; occlusion_rays_kernel
// writes the same rays to memory.  DESIGN.md "Occlusion over a hemisphere".
#pragma once

#include "occlusion_rule.hpp"
#include "ray_query.hpp"  // bvh_segment_any, brute_segment_any; queries.hpp: QueryStack, query_stack_bind, store_f3

namespace p3d {

struct OcclusionParams {
  DevScene sc;
  uint32_t n;
  const float* point;      // n x 3
  const float* normal;     // n x 3, used as given
  const float* max_dist;   // n, or null: +inf
  uint64_t seed;
  uint32_t samples, sample_begin, point_offset;  // samples >= 1, sample_begin + samples <= 2^32
  uint32_t accumulate;     // add to what the outputs hold
  float bias;
  uint32_t* unoccluded;    // n
  float* bent;             // n x 3, or null
  QueryStack stack;
};

__device__ __forceinline__ void occlusion_load_frame(const float* point, const float* normal, size_t row, float bias, OcclusionFrame& f) {
  const float p[3] = {point[3 * row], point[3 * row + 1], point[3 * row + 2]};
  const float w[3] = {normal[3 * row], normal[3 * row + 1], normal[3 * row + 2]};
  occlusion_frame(p, w, bias, f);
}

// One TEAM of neighbouring lanes per point, TEAM a power of two <= 64 = kBlock: a block is one wavefront, so a team never
// straddles a wave.  Lane l of a team takes samples sample_begin + l, + TEAM, ...: the rays of a team share their origin, so
// they meet the same nodes at the top of the tree and, under a short limit, the same leaves (a team of 1 is the layout of
// ray_query_kernel: unrelated rays on neighbouring lanes).  Every lane of the wave runs the same number of trips and none
// returns early - a lane whose sample lies past the end, or whose point past n, carries valid = false through the loop -
// because the reductions read every lane: the count of a trip is a ballot under the team's mask, the bent normal one
// butterfly of fixed order over the team's lanes after the loop (each lane has summed its own free directions in sample
// order).  No atomics: the same call with the same TEAM gives the same bits.  Lane 0 of the team writes.
// The stack is a lane's QueryStack column, cleared before every sample: bvh_culled_walk leaves entries behind when a leaf
// ended the lane (queries.hpp).  The host sizes the spill area by the lanes launched (n x TEAM), not by the points.
// bvh_culled_walk steps by wave vote over the lanes that are in it; the lanes without a sample this trip wait at the ballot.
template <int ACCEL, int TEAM>
__global__ void __launch_bounds__(kBlock) occlusion_kernel(const OcclusionParams P) {
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
      open = !(ACCEL == P3D_ACCEL_BVH ? bvh_segment_any(P.sc, st, ray, limit, ct) : brute_segment_any(P.sc, ray, limit, ct));
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
}

struct OcclusionRaysParams {
  uint32_t n;
  const float* point;
  const float* normal;
  uint64_t seed;
  uint32_t samples, sample_begin, point_offset;
  float bias;
  float* origin;     // n * samples x 3, row i * samples + j
  float* direction;
};

// One row per thread (the host refuses n x samples past 2^32).  The frame of a point is worked out once per row: the writer
// is the check and the two-call path, not the product.
__global__ void __launch_bounds__(256) occlusion_rays_kernel(const OcclusionRaysParams R) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= (uint64_t)R.n * R.samples) return;
  const uint32_t i = (uint32_t)(r / R.samples), j = (uint32_t)(r - (uint64_t)i * R.samples);
  OcclusionFrame f;
  occlusion_load_frame(R.point, R.normal, i, R.bias, f);
  float dir[3];
  occlusion_direction(f, R.seed, R.point_offset + i, R.sample_begin + j, dir);
  store_f3(R.origin, (size_t)r, f3(f.origin[0], f.origin[1], f.origin[2]));
  store_f3(R.direction, (size_t)r, f3(dir[0], dir[1], dir[2]));
}

}  // namespace p3d
