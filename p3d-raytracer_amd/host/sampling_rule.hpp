// sampling_rule.hpp — what a sampler draws with, in ONE place for its users on both sides of the boundary: the PCG stream of a
// (pixel or point, sample) pair and the sine and cosine of an angle.  The device kernels (csrc/device_core.hpp, pt_kernel.hpp,
// occlusion_query.hpp) and the host writer of the occlusion rays (host_queries.cpp, through occlusion_rule.hpp) must give the
// same bits, so neither side spells these out for itself.  Integers, and double arithmetic built from + - * floor only; both
// translation units are compiled without contraction (-ffp-contract=off).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIP__)
#define P3D_RULE_HD __host__ __device__ inline __attribute__((always_inline))  // (HIP's __forceinline__, whose header a host file does not include)
#else
#define P3D_RULE_HD inline
#endif

namespace p3d {

constexpr float kPIf = 3.141592653589793238462f;  // camera.h:13

// sin/cos: the reference calls libm (cosf/sinf main.cpp:400, cos/sin main.cpp:436).  libm differs between platforms by an ulp,
// which flips rare hit decisions and would make CPU and GPU paths diverge visibly at 256 spp.  The kernels, the oracle and the
// host writers therefore use the same explicit double-precision routine.
P3D_RULE_HD void det_sincos(double x, double& s_out, double& c_out) {
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

// ---------------------------------------------------------------------------
// RNG: one PCG-XSH-RR 64/32 stream per (pixel, sample); same definition as the oracle's.
// ---------------------------------------------------------------------------
P3D_RULE_HD uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
struct Rng {
  uint64_t state, inc;
  P3D_RULE_HD void seed_stream(uint64_t seed, uint32_t pixel, uint32_t sample) {
    const uint64_t k = mix64(seed ^ mix64(((uint64_t)pixel << 32) | (uint64_t)sample));
    inc = (mix64(k) << 1) | 1ull;
    state = k * 6364136223846793005ull + inc;
  }
  P3D_RULE_HD uint32_t next31() {
    const uint64_t old = state;
    state = old * 6364136223846793005ull + inc;
    const uint32_t xs = (uint32_t)(((old >> 18) ^ old) >> 27);
    const uint32_t rot = (uint32_t)(old >> 59);
    return ((xs >> rot) | (xs << ((0u - rot) & 31u))) >> 1;
  }
  // maths.h:67-70 with RAND_MAX = 2^31-1 ((float)RAND_MAX == 2^31); can return exactly 1.0f
  P3D_RULE_HD float rand_float() { return (float)next31() / 2147483648.0f; }
  // main.cpp:75-77
  P3D_RULE_HD double erand48() { return (double)next31() / 2147483647.0; }
};

}  // namespace p3d
