// grid_rule.hpp — the arithmetic of the uniform grid's frame (grid.cpp:3-68), in ONE place for its two builders: Grid::Build
// on the host (accel_build.cpp) and the device build (csrc/grid_build.hpp).  The device grid must be the host's to the bit, so
// neither builder spells these expressions out for itself.  float32 throughout, evaluated left to right; both translation
// units are compiled without contraction (-ffp-contract=off) and with IEEE division.
#pragma once

#include <cmath>

#if defined(__HIP__)
#define P3D_GRID_HD __host__ __device__
#else
#define P3D_GRID_HD
#endif

namespace p3d {

constexpr float kGridEps = 0.0001f;    // the bounds are the union of the object boxes grown by this (grid.cpp:211-259)
constexpr float kGridDensity = 2.0f;   // `m`, grid.h:33

// Cells along an axis of width w = p1 - p0, still a float: the caller converts (the host as the reference does, the device
// after checking that it fits an int).  `s` is the reference's powf(n / volume, 1 / 3): the exponent is the integer 0, so it
// is 1 for every scene, NaN and infinite volumes included (Q11).
inline float grid_axis_cells(float m, float w, float s) { return truncf(m * w * s) + 1; }

// First or last cell along an axis that the box face at coordinate b overlaps, on an axis of n cells from p0 to p1
P3D_GRID_HD inline int grid_axis_cell(float b, float p0, float p1, int n) {
  const double t = (b - p0) * n / (p1 - p0);  // float: n converts to float, product before quotient
  const double lo = 0, hi = n - 1;
  return static_cast<int>(t < lo ? lo : (t > hi ? hi : t));  // clamp of maths.h:46-49, in double
}

}  // namespace p3d
