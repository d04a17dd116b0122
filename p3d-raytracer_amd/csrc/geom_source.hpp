// geom_source.hpp — the device half of p3d_scene_update_geometry_device: triangles and spheres of a live scene take their nine
// geometry floats from buffers in DEVICE memory (a [V, 3] position array, gathered through an [F, 3] index array or read as a
// soup; an [N, 4] array of sphere centres and radii).
//
// One thread per covered object.  The host uploads the sources sorted by `first`, each with the exclusive prefix sum of the
// counts in front of it; thread i finds its source by binary search in those prefixes (as xform::transform_prims finds its
// range), CHECKS its three indices against n_elems, only then gathers the positions as scalar floats (the caller's memory is
// 4-byte aligned, no more), runs host/prim_rule.hpp's arithmetic and writes what lbvh::scatter_prims writes: object-order
// geometry, shading normal, box, and the rest copy if the scene has one.  Type, material and index are the object's own (read
// from its third geometry word).  About 72 bytes read (36 of indices, 36 of positions) and 112 written per triangle, 48 more
// with a rest copy: memory-bound.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/prim_rule.hpp"
#include "lbvh.hpp"
#include "xform_prims.hpp"  // xform::box_usable: the one copy of the test both routes skip an object by

namespace p3d {
namespace geomsrc {

// A p3d_geom_source as it is staged; `before` = objects covered by the sources in front of it in the sorted order
struct StagedSource {
  uint32_t first, count, kind, n_elems;
  const float* data;
  const uint32_t* index;
  uint32_t before, pad[3];
};
static_assert(sizeof(StagedSource) == 48, "StagedSource is staged behind a 16-byte counter block, three uint4 each");

// counters[0]: triangles with an index >= n_elems, counters[1]: objects whose new box is non-finite or inverted.  Neither kind
// of object is written.  No read of a source's `data` outside [0, n_elems) elements, none of `index` outside [0, 3 count).
__global__ void gather_geometry(const StagedSource* sources, uint32_t n_sources, uint32_t total, uint32_t n_objs, float4* ogeom,
                                float4* normals, float4* boxes, float4* rest, uint32_t* counters) {
  const uint32_t i = blockIdx.x * lbvh::kThreads + threadIdx.x;
  if (i >= total) return;
  uint32_t lo_s = 0, hi_s = n_sources;  // the last source with before <= i
  while (hi_s - lo_s > 1) {
    const uint32_t mid = (lo_s + hi_s) >> 1;
    if (sources[mid].before <= i) lo_s = mid; else hi_s = mid;
  }
  const StagedSource sg = sources[lo_s];
  const uint32_t k = i - sg.before;
  if (k >= sg.count) return;  // (the host has checked all of this)
  const uint32_t obj = sg.first + k;
  if (obj >= n_objs) return;
  const float4 c = ogeom[3 * obj + 2];  // geom_of: v[8], type | material << 8, the object index
  const uint32_t type = __float_as_uint(c.y) & 0xffu;
  if (type != sg.kind) return;
  float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float n[3] = {0.f, 0.f, 0.f}, lo[3], hi[3];
  if (type == P3D_PRIM_TRIANGLE) {
    uint32_t at[3] = {3 * k, 3 * k + 1, 3 * k + 2};  // (a soup: 3 count == n_elems fits 32 bits)
    if (sg.index)
      for (int q = 0; q < 3; ++q) at[q] = sg.index[3 * (size_t)k + q];
    if (at[0] >= sg.n_elems || at[1] >= sg.n_elems || at[2] >= sg.n_elems) {  // before the gather
      atomicAdd(&counters[0], 1u);
      return;
    }
    for (int q = 0; q < 3; ++q) {
      const float* p = sg.data + 3 * (size_t)at[q];
      v[3 * q] = p[0]; v[3 * q + 1] = p[1]; v[3 * q + 2] = p[2];
    }
    triangle_normal_box(v, n, lo, hi);
  } else if (type == P3D_PRIM_SPHERE) {
    if (k >= sg.n_elems) return;  // (n_elems == count)
    const float* p = sg.data + 4 * (size_t)k;
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
    sphere_box(v, v[3], lo, hi);
  } else {
    return;  // refused on the host
  }
  if (!xform::box_usable(lo, hi)) {
    atomicAdd(&counters[1], 1u);
    return;
  }
  const float4 g0 = make_float4(v[0], v[1], v[2], v[3]), g1 = make_float4(v[4], v[5], v[6], v[7]), g2 = make_float4(v[8], c.y, c.z, 0.f);
  ogeom[3 * obj] = g0;
  ogeom[3 * obj + 1] = g1;
  ogeom[3 * obj + 2] = g2;
  if (rest) {
    rest[3 * obj] = g0;
    rest[3 * obj + 1] = g1;
    rest[3 * obj + 2] = g2;
  }
  normals[obj] = make_float4(n[0], n[1], n[2], 0.f);
  boxes[2 * obj] = make_float4(lo[0], lo[1], lo[2], 0.f);
  boxes[2 * obj + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
}

}  // namespace geomsrc
}  // namespace p3d
