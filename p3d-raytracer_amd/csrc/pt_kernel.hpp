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
// the same explicit double-precision routine (det_sincos) built from + - * floor only.
#pragma once

#include "kernels.hpp"

#ifndef P3D_PT_WAVES
#define P3D_PT_WAVES 4  // minimum waves per SIMD asked of the register allocator: 128 VGPRs, 12-15 spilled dwords for the BVH
                        // instantiations.  cfg3: 3 waves 190 ms, 4 waves 160 ms, 5 waves (96 VGPRs, 51 spilled) 177 ms.  (Before the
                        // deferred dielectric branches left LDS, 4 waves did not fit and 3 was the optimum.)
#endif

namespace p3d {

__device__ __forceinline__ void det_sincos(double x, double& s_out, double& c_out) {
  const double two_over_pi = 6.36619772367581382433e-01;
  const double pio2_hi = 1.57079632673412561417e+00, pio2_lo = 6.07710050650619224932e-11;
  const double kd = floor(x * two_over_pi + 0.5);
  const double r = (x - kd * pio2_hi) - kd * pio2_lo;
  const double z = r * r;
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03,
               S3 = -1.98412698298579493134e-04, S4 = 2.75573137070700676789e-06,
               S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03,
               C3 = 2.48015872894767294178e-05, C4 = -2.75573143513906633035e-07,
               C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double sp = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
  const double s = r + (z * r) * (S1 + z * sp);
  const double cp = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
  const double c = 1.0 - (0.5 * z - z * cp);
  const long long k = (long long)kd;
  switch (k & 3) {
    case 0: s_out = s; c_out = c; break;
    case 1: s_out = c; c_out = -s; break;
    case 2: s_out = -s; c_out = -c; break;
    default: s_out = -c; c_out = s; break;
  }
}

constexpr float kPIf = 3.141592653589793238462f;  // camera.h:13

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
