// pt_kernel.hpp — the path tracer (Radiance, main.cpp:313-516) as a persistent per-lane
// bounce loop.
//
// The reference recurses:  R = E + e + f * R(child).  Here every lane owns one pixel (or, from
// 16 samples per pixel, a quarter of one: SUB = 4 below) and runs ONE flat loop whose body is
// a single bounce; a lane whose path ended starts its next
// sample (or pops its pending dielectric branch) in the same iteration instead of waiting
// for the slowest lane of the wave, so the wave only idles lanes in the very last
// iterations of a tile (the "persistent threads" bounce loop BASELINE.json asks for).  Radiance is carried as
//     L += T * (E + e);   T *= f
// which is the same sum evaluated outermost-first (the recursion evaluates innermost-
// first): results agree with the recursive oracle to float rounding (~1e-6 relative),
// far inside the 1e-4 tolerance; hit decisions and the RNG stream are identical.
//
// sin/cos: the reference calls libm (cosf/sinf main.cpp:400, cos/sin main.cpp:436).  libm
// differs between platforms by an ulp, which flips rare hit decisions and would make CPU
// and GPU paths diverge visibly at 256 spp.  Both this kernel and the oracle therefore use
// the same explicit double-precision routine (det_sincos, host/sampling_rule.hpp) built from + - * floor only.
#pragma once

#include "kernels.hpp"

#ifndef P3D_PT_WAVES
#define P3D_PT_WAVES 4  // minimum waves per SIMD asked of the register allocator: 128 VGPRs, 12-15 spilled dwords for the BVH
                        // instantiations.  cfg3: 3 waves 190 ms, 4 waves 160 ms, 5 waves (96 VGPRs, 51 spilled) 177 ms.  (Before the
                        // deferred dielectric branches left LDS, 4 waves did not fit and 3 was the optimum.)
#endif

namespace p3d {

// pending dielectric branch (main.cpp:512-513): 3 float4 per entry, 2 entries per lane, in the
// global scratch the Whitted kernel uses for its level records (rarely touched: only the first
// two bounces on glass fork; 6 KB of LDS per wave would cost the path tracer a wave per SIMD)
struct Pending {
  float4* base;     // &scratch[thread]; float4 q of entry e at base[(e * 3 + q) * stride]
  uint32_t stride;  // threads of the launch
  int n;
};

// Adaptive passes (p3d_adaptive, include/p3d.h; adaptive.hpp): the pixels a pass renders are the entries of a compacted
// list, handed out to the waves in groups of 16 (SUB = 4) or 64 (SUB = 1) by a ticket counter - the grid is sized to the
// resident waves, not to the frame.  Besides the running sum the kernel keeps S2, the sum of the squared luminance of
// every sample in sample order (lane 0 of the pixel adds it, in a register, next to the colour).
struct PtAdaptParams {
  const uint32_t* list;   // pixels (r * w + c of the tile) that take this pass's samples
  const uint32_t* count;  // entries of list
  uint32_t* ticket;       // next group of the list; 0 at launch (adapt_resolve_kernel resets it)
  float* sum_y2;          // [pixel] S2 of the samples so far
};

__device__ __forceinline__ float luma_sq(F3 L) {  // y^2 of one sample (include/p3d.h "Error metric")
  const float y = 0.2126f * L.x + 0.7152f * L.y + 0.0722f * L.z;
  return y * y;
}

template <int ACCEL, bool LDS, bool STATS, int SUB = 1>
__global__ void __launch_bounds__(kBlock, P3D_PT_WAVES) pt_kernel(const RenderParams P) {
  constexpr bool ADAPT = false;
  const PtAdaptParams A{};
#include "pt_body.inc"
}

template <int ACCEL, bool LDS, bool STATS, int SUB>
__global__ void __launch_bounds__(kBlock, P3D_PT_WAVES) pt_adaptive_kernel(const RenderParams P, const PtAdaptParams A) {
  constexpr bool ADAPT = true;
#include "pt_body.inc"
}

}  // namespace p3d
