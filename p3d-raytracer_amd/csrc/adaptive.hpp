// adaptive.hpp — the step behind every pass of an adaptive frame (p3d_adaptive, include/p3d.h): resolve, decide, compact.
//
// One thread per pixel slot of the tile.  Slots run over the tile in 8x8 blocks, and inside a block over its four 4x4
// quarters, so that 64 consecutive slots are one 8x8 tile and 16 consecutive slots one 4x4 quarter: the list a wave
// compacts keeps the pixels of one tile together, and the groups pt_adaptive_kernel hands out stay coherent while most
// pixels are active.  The order of the waves' chunks in the list is whatever the atomic gives; no pixel's bits depend on
// which wave renders it.
#pragma once

#include "pt_kernel.hpp"

namespace p3d {

constexpr int kAdaptResolveThreads = 256;

struct AdaptResolveParams {
  const float* sum;       // [3 * pixel] running sums, [pixel] first hits, S2 (pt_adaptive_kernel)
  const int32_t* hit;
  const float* sum_y2;
  uint32_t* samples;      // [pixel] samples in the sums
  uint8_t* active;        // [pixel] 1 while the pixel takes samples
  float* rel_err;         // [pixel] error at the pixel's last pass
  uint32_t* list_out;     // the next pass's list and its count (0 on entry)
  uint32_t* count_out;
  uint32_t* count_done;   // the count the pass just rendered read: zeroed for the pass after next
  uint32_t* ticket;       // the group counter of pt_adaptive_kernel: zeroed for the next pass
  float* rgb;             // caller outputs (any may be null)
  int32_t* hit_id;
  uint8_t* rgb8;
  uint32_t* samples_out;
  int32_t w, h;
  uint32_t tiles8_x, slots;
  uint32_t n;               // the pass rendered n more samples of the listed pixels
  uint32_t min_samples;
  float rel_error, gamma;
  uint32_t init;            // 1: start of a frame - every pixel listed with 0 samples, no outputs
};

__device__ __forceinline__ float adapt_rel_err(F3 S, float S2, uint32_t samples) {  // include/p3d.h "Error metric"
  const float n = (float)samples;
  const float Y = 0.2126f * S.x + 0.7152f * S.y + 0.0722f * S.z;
  const float m = Y / n;
  const float v = fmaxf((S2 - Y * m) / (n - 1.0f), 0.0f);
  return sqrtf(v / n) / (m + 1.0e-3f);
}

__global__ void __launch_bounds__(kAdaptResolveThreads) adapt_resolve_kernel(const AdaptResolveParams R) {
  const uint32_t k = blockIdx.x * kAdaptResolveThreads + threadIdx.x;
  if (k == 0) {
    *R.ticket = 0;
    *R.count_done = 0;
  }
  const uint32_t t8 = k >> 6, quad = (k >> 4) & 3u, q = k & 15u;
  const int c = (int)((t8 % R.tiles8_x) * 8 + (quad & 1u) * 4 + (q & 3u));
  const int r = (int)((t8 / R.tiles8_x) * 8 + (quad >> 1) * 4 + (q >> 2));
  const bool valid = k < R.slots && c < R.w && r < R.h;
  const uint32_t p = valid ? (uint32_t)r * (uint32_t)R.w + (uint32_t)c : 0u;
  bool keep = false;
  if (valid && R.init) {
    R.samples[p] = 0;
    R.active[p] = 1;
    R.rel_err[p] = 0.0f;
    keep = true;
  } else if (valid) {
    uint32_t sp = R.samples[p];
    const F3 S = f3(R.sum[3 * p], R.sum[3 * p + 1], R.sum[3 * p + 2]);
    if (R.active[p]) {  // listed in this pass
      sp += R.n;
      R.samples[p] = sp;
      const float e = adapt_rel_err(S, R.sum_y2[p], sp);
      R.rel_err[p] = e;
      // (a mean luminance of -1e-3 or less - the reference's radiance can be negative behind glass - makes e negative, -0, inf
      // or NaN: no estimate of a relative error, the pixel goes on; e of a positive denominator has a clear sign bit)
      keep = !(sp >= R.min_samples && !(__float_as_uint(e) >> 31) && e < R.rel_error);
      if (!keep) R.active[p] = 0;  // for good
    }
    // the epilogue of pt_kernel for a frame of sp samples: the bits a plain accumulator has after sp samples
    const F3 color = S / (float)sp;
    if (R.rgb) {
      R.rgb[3 * p] = color.x; R.rgb[3 * p + 1] = color.y; R.rgb[3 * p + 2] = color.z;
    }
    if (R.hit_id) R.hit_id[p] = R.hit[p];
    if (R.rgb8) store_rgb8(R.rgb8 + 3 * p, color, R.gamma);
    if (R.samples_out) R.samples_out[p] = sp;
  }
  // wave-ballot compaction: one atomic per wave, the wave's pixels in slot order
  const uint32_t lane = threadIdx.x & 63u;
  const unsigned long long mask = __ballot(keep);
  uint32_t base = 0;
  if (lane == 0 && mask) base = atomicAdd(R.count_out, (uint32_t)__popcll(mask));
  base = __shfl(base, 0, 64);
  if (keep) R.list_out[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = p;
}

}  // namespace p3d
