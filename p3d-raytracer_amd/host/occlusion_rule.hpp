// occlusion_rule.hpp — the rays of a hemisphere-occlusion query, in ONE place for their users: p3d_occlusion_rays
// (host_queries.cpp), which states them on host arrays, and occlusion_kernel and occlusion_rays_kernel
// (csrc/occlusion_query.hpp), whose rays must be the host form's bits.  Sample s of point i draws from the stream
// seed_stream(seed, point_offset + i, s) and is the cosine-weighted direction of the path tracer's diffuse bounce
// (main.cpp:391-405), spelled as csrc/pt_bounce.inc:49-57 spells it: the same operations in the same order.
//   r1 = 2 * kPIf * rand_float();  r2 = rand_float();  r2s = sqrtf(r2)
//   w = the normal AS GIVEN (not normalised here: a caller's unit normal stays its bits)
//   u = normalized(cross(|w.x| > 0.1 ? (0,1,0) : (1,0,0), w));  v = cross(w, u)
//   (s1, c1) = det_sincos((double)r1)
//   direction = normalized((u*(float)c1*r2s + v*(float)s1*r2s) + w*sqrtf(1 - r2))
//   origin    = point + w * bias                                 (bias 1e-4f: offsetIntersection, main.cpp:82-84)
// A normal that is zero or not finite gives NaN directions (0 / 0 in the normalisation of u); a NaN ray hits nothing, so every
// sample of such a point counts as free.  float32 throughout but for det_sincos, evaluated as written; both translation units are compiled
// without contraction (-ffp-contract=off) and with correctly rounded square root and division (prim_rule.hpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "p3d.h"
#include "sampling_rule.hpp"

namespace p3d {

// (double)a > 0.1 folded to float exactly: 0.1f is the float just above 0.1 (csrc/device_core.hpp gt_0p1)
P3D_RULE_HD bool occlusion_gt_0p1(float a) { return a >= 0.1f; }

// vector.cpp:84-99
P3D_RULE_HD void occlusion_cross(const float a[3], const float b[3], float out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
// vector.cpp:65-70: the reciprocal of the float length, three multiplies (csrc/device_core.hpp normalized)
P3D_RULE_HD void occlusion_normalize(float a[3]) {
  const float l = 1.0f / sqrtf(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
  a[0] = a[0] * l; a[1] = a[1] * l; a[2] = a[2] * l;
}

// What every sample of a point shares: the tangent frame around w, and where the rays start
struct OcclusionFrame {
  float u[3], v[3], w[3], origin[3];
};
P3D_RULE_HD void occlusion_frame(const float point[3], const float normal[3], float bias, OcclusionFrame& f) {
  for (int k = 0; k < 3; ++k) f.w[k] = normal[k];
  const float ey[3] = {0.0f, 1.0f, 0.0f}, ex[3] = {1.0f, 0.0f, 0.0f};
  occlusion_cross(occlusion_gt_0p1(fabsf(f.w[0])) ? ey : ex, f.w, f.u);
  occlusion_normalize(f.u);
  occlusion_cross(f.w, f.u, f.v);
  for (int k = 0; k < 3; ++k) f.origin[k] = point[k] + f.w[k] * bias;
}

// Sample `sample` of the point with stream index `index` (point_offset + i)
P3D_RULE_HD void occlusion_direction(const OcclusionFrame& f, uint64_t seed, uint32_t index, uint32_t sample, float d[3]) {
  Rng rng;
  rng.seed_stream(seed, index, sample);
  const float r1 = 2 * kPIf * rng.rand_float();
  const float r2 = rng.rand_float();
  const float r2s = sqrtf(r2);
  double s1, c1;
  det_sincos((double)r1, s1, c1);
  const float cz = sqrtf(1 - r2);
  for (int k = 0; k < 3; ++k) d[k] = (f.u[k] * (float)c1 * r2s + f.v[k] * (float)s1 * r2s) + f.w[k] * cz;
  occlusion_normalize(d);
}

// What the three entry points refuse of a p3d_occlusion_params alike -> the message, or null
inline const char* occlusion_params_refusal(const p3d_occlusion_params* p) {
  if (!p) return "null params";
  if (p->samples == 0) return "samples must be at least 1";
  if ((uint64_t)p->sample_begin + p->samples > 0x100000000ull) return "sample_begin + samples must not pass 2^32";
  if (p->flags & ~P3D_OCCLUSION_ACCUMULATE) return "unknown flag";
  if (!std::isfinite(p->bias)) return "bias must be finite";
  if (p->team > 64 || (p->team & (p->team - 1))) return "team must be 0 (the library chooses) or a power of two <= 64";
  return nullptr;
}

}  // namespace p3d
