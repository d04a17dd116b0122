// prim_rule.hpp — the arithmetic that turns nine geometry floats into an object, in ONE place for its users: the shape
// constructors of the host scene (scene_model.cpp: Triangle::Triangle, Sphere::GetBoundingBox) and the device kernels of
// p3d_scene_transform_prims, which moves an object and then does what the constructors do, and of
// p3d_scene_update_geometry_device, which gathers an object from device buffers first (both csrc/update_kernels.hpp).  The device
// routes must give the host route's bits, so neither side spells these expressions out for itself.  float32 throughout,
// evaluated left to right; both translation units are compiled without contraction (-ffp-contract=off) and with correctly
// rounded square root and division.
#pragma once

#include <cmath>

#if defined(__HIP__)
#define P3D_PRIM_HD __host__ __device__
#else
#define P3D_PRIM_HD
#endif

namespace p3d {

constexpr float kPrimEps = 0.0001f;  // scene.h:31 EPSILON: a triangle's box is grown by this on every side

// std::min / std::max as the constructors use them (the first argument wins a tie, so the sign of a zero is the host's)
P3D_PRIM_HD inline float prim_lo(float a, float b) { return b < a ? b : a; }
P3D_PRIM_HD inline float prim_hi(float a, float b) { return a < b ? b : a; }

// p' = M p for a row-major 3x4 matrix: x' = ((m0 x + m1 y) + m2 z) + m3, the y and z rows alike
P3D_PRIM_HD inline void xform_point(const float m[12], const float p[3], float out[3]) {
  const float x = p[0], y = p[1], z = p[2];  // (out may be p)
  for (int r = 0; r < 3; ++r) out[r] = ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

// scene.cpp:12-35: unit normal of (P1-P0)x(P2-P0), normalised as Vector::normalize does it (vector.cpp:65-70: the reciprocal
// of the float length taken in double, narrowed to float, three multiplies); box = min / max of the vertices -+ EPSILON
P3D_PRIM_HD inline void triangle_normal_box(const float v[9], float n[3], float lo[3], float hi[3]) {
  const float ax = v[3] - v[0], ay = v[4] - v[1], az = v[5] - v[2];
  const float bx = v[6] - v[0], by = v[7] - v[1], bz = v[8] - v[2];
  const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
  const float len = sqrtf(cx * cx + cy * cy + cz * cz);
  const float inv = static_cast<float>(1.0 / static_cast<double>(len));
  n[0] = cx * inv; n[1] = cy * inv; n[2] = cz * inv;
  for (int k = 0; k < 3; ++k) {
    lo[k] = prim_lo(prim_lo(v[k], v[3 + k]), v[6 + k]) - kPrimEps;
    hi[k] = prim_hi(prim_hi(v[k], v[3 + k]), v[6 + k]) + kPrimEps;
  }
}

// scene.cpp:194-198: centre -+ (radius, radius, radius)
P3D_PRIM_HD inline void sphere_box(const float c[3], float radius, float lo[3], float hi[3]) {
  for (int k = 0; k < 3; ++k) {
    lo[k] = c[k] - radius;
    hi[k] = c[k] + radius;
  }
}

// What p3d_scene_transform_prims accepts for an axis-aligned box: a positive scale per axis and a translation
// (p3d_scene_pose_device asks on the device, where its matrices are)
P3D_PRIM_HD inline bool xform_is_positive_diagonal(const float m[12]) {
  return m[0] > 0 && m[5] > 0 && m[10] > 0 && m[1] == 0 && m[2] == 0 && m[4] == 0 && m[6] == 0 && m[8] == 0 && m[9] == 0;
}

}  // namespace p3d
