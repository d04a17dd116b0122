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
// Two kernels of one name, told apart by their parameters, for the reason nearest_k_device_kernel has two: the one launched
// without filters holds no filter code.  The filtered one (p3d_occlusion_filtered_device) has one filter row per POINT, read once
// by every lane of the point's team before its first sample and used for all of them.
struct OcclusionFilteredParams {
  OcclusionParams q;
  FilterParams f;
};
template <int ACCEL, int TEAM>
__global__ void __launch_bounds__(kBlock) occlusion_kernel(const OcclusionParams P) {
  const NoFilterSource filters{};
#include "occlusion_body.inc"
}
template <int ACCEL, int TEAM>
__global__ void __launch_bounds__(kBlock) occlusion_kernel(const OcclusionFilteredParams PF) {
  const OcclusionParams& P = PF.q;
  const FilterParams& filters = PF.f;
#include "occlusion_body.inc"
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
