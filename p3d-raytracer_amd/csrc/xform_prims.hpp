// xform_prims.hpp — the device half of p3d_scene_transform_prims: objects of a live scene are set to T(rest) in place.
//
// One thread per covered object.  The host uploads the ranges sorted by `first`, each with the exclusive prefix sum of the
// counts in front of it; thread i finds its range by binary search in those prefixes, reads the object's rest record (three
// float4: the object-order geometry it was created with or last given by p3d_scene_update_prims) and its transform (four
// float4, the same address for a whole wave in the common case of long ranges), and writes what lbvh::scatter_prims writes:
// object-order geometry, shading normal and box.  The arithmetic is host/prim_rule.hpp's, so the result is what the host
// constructors give for the same numbers, to the bit.  About 150 bytes per object (48 read, 112 written): memory-bound.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/prim_rule.hpp"
#include "lbvh.hpp"

namespace p3d {
namespace xform {

// A range as it is staged: objects [first, first + count) take xforms[xform]; `before` = objects covered by the ranges in
// front of it in the sorted order (the slot of p3d_xform_range.reserved)
struct StagedRange {
  uint32_t first, count, xform, before;
};
static_assert(sizeof(StagedRange) == 16, "StagedRange is read as one uint4");

__device__ __forceinline__ bool box_usable(const float lo[3], const float hi[3]) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && fabsf(lo[k]) < INFINITY && fabsf(hi[k]) < INFINITY && lo[k] <= hi[k];  // (NaN fails all three)
  return ok;
}

// rest, ogeom: 3 float4 per object (geom_of's packing); xforms: 4 float4 per p3d_xform (m rows 0-2, then sphere_scale);
// an object whose new box is non-finite or inverted is not written and counted in *skipped
__global__ void transform_prims(const float4* rest, const uint4* ranges, uint32_t n_ranges, const float4* xforms, uint32_t n_xforms,
                                uint32_t total, uint32_t n_objs, float4* ogeom, float4* normals, float4* boxes, uint32_t* skipped) {
  const uint32_t i = blockIdx.x * lbvh::kThreads + threadIdx.x;
  if (i >= total) return;
  uint32_t lo_r = 0, hi_r = n_ranges;  // the last range with before <= i
  while (hi_r - lo_r > 1) {
    const uint32_t mid = (lo_r + hi_r) >> 1;
    if (ranges[mid].w <= i) lo_r = mid; else hi_r = mid;
  }
  const uint4 rg = ranges[lo_r];
  const uint32_t k = i - rg.w;
  if (k >= rg.y || rg.z >= n_xforms) return;  // (the host has checked all of this)
  const uint32_t obj = rg.x + k;
  if (obj >= n_objs) return;
  const float4 a = rest[3 * obj], b = rest[3 * obj + 1], c = rest[3 * obj + 2];
  const float4 m0 = xforms[4 * rg.z], m1 = xforms[4 * rg.z + 1], m2 = xforms[4 * rg.z + 2], m3 = xforms[4 * rg.z + 3];
  const float m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
  float v[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x};
  float n[3] = {0.f, 0.f, 0.f}, lo[3], hi[3];
  const uint32_t type = __float_as_uint(c.y) & 0xffu;
  if (type == P3D_PRIM_TRIANGLE) {
    xform_point(m, v, v);
    xform_point(m, v + 3, v + 3);
    xform_point(m, v + 6, v + 6);
    triangle_normal_box(v, n, lo, hi);
  } else if (type == P3D_PRIM_SPHERE) {
    xform_point(m, v, v);
    v[3] = v[3] * m3.x;
    sphere_box(v, v[3], lo, hi);
  } else if (type == P3D_PRIM_BOX) {
    xform_point(m, v, v);
    xform_point(m, v + 3, v + 3);
    for (int q = 0; q < 3; ++q) { lo[q] = v[q]; hi[q] = v[3 + q]; }
  } else {
    return;  // a plane: refused on the host
  }
  if (!box_usable(lo, hi)) {
    atomicAdd(skipped, 1u);
    return;
  }
  ogeom[3 * obj] = make_float4(v[0], v[1], v[2], v[3]);
  ogeom[3 * obj + 1] = make_float4(v[4], v[5], v[6], v[7]);
  ogeom[3 * obj + 2] = make_float4(v[8], c.y, c.z, 0.f);
  normals[obj] = make_float4(n[0], n[1], n[2], 0.f);
  boxes[2 * obj] = make_float4(lo[0], lo[1], lo[2], 0.f);
  boxes[2 * obj + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

}  // namespace xform
}  // namespace p3d
