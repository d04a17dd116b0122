// update_kernels.hpp — the device half of the three geometry updates of a live scene: host records (p3d_scene_update_prims),
// transforms of the rest pose (p3d_scene_transform_prims, and p3d_scene_pose_device, which reads its matrices from device
// memory and its ranges from the scene's rig) and positions in device memory (p3d_scene_update_geometry_device, and
// p3d_scene_refit_device, which hands its sources over as a kernel argument).
//
// One thread per covered object, blocks of lbvh::kThreads.  Each kernel works out an object's nine geometry floats, shading
// normal and box its own way - the arithmetic is host/prim_rule.hpp's, so the result is what the host constructors give for
// the same numbers, to the bit - and hands them to store_object, the one place that writes the object-order geometry, the
// rest copy, the normals and the builder's boxes.  The two routes that name objects by spans (ranges, sources) are staged
// sorted by `first`, each span with the exclusive prefix sum of the counts in front of it; find_span is the one search.
// About 112 bytes written per object (160 with a rest copy) and 48 to 112 read, no reuse: memory-bound.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../host/prim_rule.hpp"
#include "lbvh.hpp"

namespace p3d {
namespace upd {

// One object of p3d_scene_update_prims as it is staged for scatter_prims: the caller's record and the object it replaces
struct UpdateRecord {
  p3d_prim prim;
  uint32_t object;
  uint32_t pad[3];
};
static_assert(sizeof(UpdateRecord) == 112, "UpdateRecord is read as seven float4");

// A span's first 16 bytes, the same for both kinds: objects [first, first + count); `before` = objects covered by the spans
// in front of it in the sorted order.  A range is this alone (`own`: its transform, `before` in the slot of
// p3d_xform_range.reserved); a source carries its buffers behind it (`own`: its kind).
struct StagedRange {
  uint32_t first, count, xform, before;
};
struct StagedSource {
  uint32_t first, count, kind, before;
  const float* data;
  const uint32_t* index;
  uint32_t n_elems, pad[3];
};
static_assert(sizeof(StagedRange) == 16 && sizeof(StagedSource) == 48, "a span is staged as one or three uint4, its head read as one");

// The bit p3d_scene_refit_device's kernel raises in the scene's status word when it skips an object (the kHoErr* bits of
// handoff.hpp are below it); the counts are in the scene's counter block
constexpr uint32_t kStatusRefitSkipped = 32u;
// The same for p3d_scene_pose_device's kernel, with a counter block of its own
constexpr uint32_t kStatusPoseSkipped = 64u;
// A rig (p3d_scene_set_rig) is one word per object: its transform slot, or this for an object no range names
constexpr uint32_t kRigNotPosed = 0xffffffffu;

__device__ __forceinline__ bool box_usable(const float lo[3], const float hi[3]) {
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = ok && fabsf(lo[k]) < INFINITY && fabsf(hi[k]) < INFINITY && lo[k] <= hi[k];  // (NaN fails all three)
  return ok;
}

// Thread i's span among n_spans of STRIDE uint4 each: the last one with before <= i, by binary search (a handful of cached
// 16-byte loads; one span is the common case).  -> its head {first, count, own, before}, its place `at`, the thread's
// position k in it and its object; false if there is no such object (the host has checked all of this)
template <int STRIDE>
__device__ __forceinline__ bool find_span(const uint4* spans, uint32_t n_spans, uint32_t i, uint32_t n_objs, uint32_t& at, uint4& head,
                                          uint32_t& k, uint32_t& obj) {
  uint32_t lo = 0, hi = n_spans;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (spans[STRIDE * mid].w <= i) lo = mid; else hi = mid;
  }
  at = lo;
  head = spans[STRIDE * lo];
  k = i - head.w;
  obj = head.x + k;
  return k < head.y && obj < n_objs;
}

// Object `obj` as every update leaves it: 3 float4 of object-order geometry packed as create_impl's geom_of packs it
// (v[0..3], v[4..7], then v[8], type | material << 8, the object index, 0), the same three into the rest copy if the scene
// has one and the route moves it (else null), the shading normal, and the two float4 of the box
__device__ __forceinline__ void store_object(uint32_t obj, float4 g0, float4 g1, float v8, uint32_t type_material, const float n[3],
                                             const float lo[3], const float hi[3], float4* ogeom, float4* rest, float4* normals,
                                             float4* boxes) {
  const float4 g2 = make_float4(v8, __uint_as_float(type_material), __uint_as_float(obj), 0.f);
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

// Replaces objects in place, one thread per record; the host has checked that every index is < n_objs and appears once.
// rest: the scene's rest geometry once p3d_scene_transform_prims has made it (else null): a replaced object rests where it is put
__global__ void scatter_prims(const UpdateRecord* recs, uint32_t n, uint32_t n_objs, float4* ogeom, float4* normals, float4* boxes, float4* rest) {
  const uint32_t i = blockIdx.x * lbvh::kThreads + threadIdx.x;
  if (i >= n) return;
  const float4* r = reinterpret_cast<const float4*>(recs + i);
  const float4 a = r[0], b = r[1], c = r[2], d = r[3], e = r[4], f = r[5], g = r[6];
  // p3d_prim: v[0..8] = a.xyzw b.xyzw c.x, type = c.y, material = c.z, n = d.xyz, bmin = e.xyz, bmax = f.xyz
  const uint32_t obj = __float_as_uint(g.x);
  if (obj >= n_objs) return;
  const float nr[3] = {d.x, d.y, d.z}, lo[3] = {e.x, e.y, e.z}, hi[3] = {f.x, f.y, f.z};
  store_object(obj, a, b, c.x, __float_as_uint(c.y) | (__float_as_uint(c.z) << 8), nr, lo, hi, ogeom, rest, normals, boxes);
}

// Object `obj` set to T(rest), the work of both transform kernels: a, b, c are its three float4 of the rest copy, m the
// row-major 3x4 matrix.  A triangle's vertices, a sphere's centre and a box's min and max go through xform_point; the
// triangle gets the loader's normal and box, the sphere radius * sphere_scale and its box.  -> false if the new box is
// non-finite or inverted: the object is not written.  A plane is left alone (the host refuses a range that covers one).
__device__ __forceinline__ bool transform_object(uint32_t obj, float4 a, float4 b, float4 c, const float m[12], float sphere_scale,
                                                 float4* ogeom, float4* normals, float4* boxes) {
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
    v[3] = v[3] * sphere_scale;
    sphere_box(v, v[3], lo, hi);
  } else if (type == P3D_PRIM_BOX) {
    xform_point(m, v, v);
    xform_point(m, v + 3, v + 3);
    for (int q = 0; q < 3; ++q) { lo[q] = v[q]; hi[q] = v[3 + q]; }
  } else {
    return true;
  }
  if (!box_usable(lo, hi)) return false;
  store_object(obj, make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), v[8], __float_as_uint(c.y), n, lo, hi, ogeom,
               nullptr, normals, boxes);
  return true;
}

// Sets objects to T(rest) in place.  rest: 3 float4 per object, the object-order geometry it was created with or last given
// by another route; xforms: 4 float4 per p3d_xform (m rows 0-2, then sphere_scale), one address for a whole wave inside a
// range.  An object whose new box is non-finite or inverted is not written and counted in *skipped.  The rest pose stays.
__global__ void transform_prims(const float4* rest, const uint4* ranges, uint32_t n_ranges, const float4* xforms, uint32_t n_xforms,
                                uint32_t total, uint32_t n_objs, float4* ogeom, float4* normals, float4* boxes, uint32_t* skipped) {
  const uint32_t i = blockIdx.x * lbvh::kThreads + threadIdx.x;
  if (i >= total) return;
  uint32_t at, k, obj;
  uint4 rg;
  if (!find_span<1>(ranges, n_ranges, i, n_objs, at, rg, k, obj) || rg.z >= n_xforms) return;
  const float4 a = rest[3 * obj], b = rest[3 * obj + 1], c = rest[3 * obj + 2];
  const float4 m0 = xforms[4 * rg.z], m1 = xforms[4 * rg.z + 1], m2 = xforms[4 * rg.z + 2], m3 = xforms[4 * rg.z + 3];
  const float m[12] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w, m2.x, m2.y, m2.z, m2.w};
  if (!transform_object(obj, a, b, c, m, m3.x, ogeom, normals, boxes)) atomicAdd(skipped, 1u);
}

// transform_prims with the ranges as the scene's rig and the matrices in the CALLER's device memory (p3d_scene_pose_device).
// rig: one word per object, its transform slot or kRigNotPosed - a thread is an object: no search, coalesced reads, any
// number of ranges.  xforms: 12 floats per slot, sphere_scale: one (null: 1 for every slot), read as scalar floats: the
// caller's memory is 4-byte aligned and no more.  What the host checks in the waiting form is checked here, per object, and
// a failing object keeps its geometry: counters[0] counts objects whose transform has a non-finite entry, whose
// sphere_scale is not finite and > 0 (whatever the object's type, as there), or that are boxes under a matrix that is not
// positive-diagonal; counters[1] objects whose new box is non-finite or inverted.  counters: the scene's own block, added to
// and never cleared here; *status takes kStatusPoseSkipped with them.  Thread i also zeroes visits[i], the fit's arrival
// counters, as gather_geometry_args does (lbvh::enqueue_fit, visits_clear).  No read of xforms outside [0, 12 n_xforms).
__global__ void pose_rig(const float4* rest, const uint32_t* rig, const float* xforms, const float* sphere_scale, uint32_t n_xforms,
                         uint32_t n_objs, float4* ogeom, float4* normals, float4* boxes, uint32_t* counters, uint32_t* status,
                         uint32_t* visits) {
  const uint32_t i = blockIdx.x * lbvh::kThreads + threadIdx.x;
  if (i >= n_objs) return;
  visits[i] = 0u;
  const uint32_t slot = rig[i];
  if (slot >= n_xforms) return;  // kRigNotPosed (the host has checked every other slot against n_xforms)
  const float* t = xforms + 12 * (size_t)slot;
  float m[12];
  bool ok = true;
  for (int q = 0; q < 12; ++q) {
    m[q] = t[q];
    ok = ok && fabsf(m[q]) < INFINITY;  // (NaN fails)
  }
  const float scale = sphere_scale ? sphere_scale[slot] : 1.0f;
  ok = ok && fabsf(scale) < INFINITY && scale > 0.0f;
  const float4 a = rest[3 * i], b = rest[3 * i + 1], c = rest[3 * i + 2];
  if ((__float_as_uint(c.y) & 0xffu) == P3D_PRIM_BOX) ok = ok && xform_is_positive_diagonal(m);
  if (!ok || !transform_object(i, a, b, c, m, scale, ogeom, normals, boxes)) {
    atomicAdd(&counters[ok ? 1 : 0], 1u);
    atomicOr(status, kStatusPoseSkipped);
  }
}

// Triangles and spheres take their nine geometry floats from buffers in DEVICE memory: a [V, 3] position array, gathered
// through an [F, 3] index array or read as a soup; an [N, 4] array of centres and radii.  Type and material are the object's
// own (read from its third geometry word).  A triangle's three indices are CHECKED against n_elems, and only then are the
// positions gathered, as scalar floats (the caller's memory is 4-byte aligned, no more).
// counters[0]: triangles with an index >= n_elems, counters[1]: objects whose new box is non-finite or inverted.  Neither kind
// of object is written.  No read of a source's `data` outside [0, n_elems) elements, none of `index` outside [0, 3 count).
// `skipped` (null: nothing more) takes kStatusRefitSkipped when an object fails: p3d_scene_refit_device, whose caller asks later.
__device__ __forceinline__ void gather_object(const StagedSource& sg, uint32_t k, uint32_t obj, float4* ogeom, float4* normals, float4* boxes,
                                              float4* rest, uint32_t* counters, uint32_t* skipped) {
  const float4 c = ogeom[3 * obj + 2];
  const uint32_t type = __float_as_uint(c.y) & 0xffu;
  if (type != sg.kind) return;
  float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float n[3] = {0.f, 0.f, 0.f}, lo[3], hi[3];
  if (type == P3D_PRIM_TRIANGLE) {
    uint32_t idx[3] = {3 * k, 3 * k + 1, 3 * k + 2};  // (a soup: 3 count == n_elems fits 32 bits)
    if (sg.index)
      for (int q = 0; q < 3; ++q) idx[q] = sg.index[3 * (size_t)k + q];
    if (idx[0] >= sg.n_elems || idx[1] >= sg.n_elems || idx[2] >= sg.n_elems) {  // before the gather
      atomicAdd(&counters[0], 1u);
      if (skipped) atomicOr(skipped, kStatusRefitSkipped);
      return;
    }
    for (int q = 0; q < 3; ++q) {
      const float* p = sg.data + 3 * (size_t)idx[q];
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
  if (!box_usable(lo, hi)) {
    atomicAdd(&counters[1], 1u);
    if (skipped) atomicOr(skipped, kStatusRefitSkipped);
    return;
  }
  store_object(obj, make_float4(v[0], v[1], v[2], v[3]), make_float4(v[4], v[5], v[6], v[7]), v[8], __float_as_uint(c.y), n, lo, hi, ogeom,
               rest, normals, boxes);
}

__global__ void gather_geometry(const StagedSource* sources, uint32_t n_sources, uint32_t total, uint32_t n_objs, float4* ogeom,
                                float4* normals, float4* boxes, float4* rest, uint32_t* counters) {
  const uint32_t i = blockIdx.x * lbvh::kThreads + threadIdx.x;
  if (i >= total) return;
  uint32_t at, k, obj;
  uint4 head;
  if (!find_span<3>(reinterpret_cast<const uint4*>(sources), n_sources, i, n_objs, at, head, k, obj)) return;
  const StagedSource sg = sources[at];
  gather_object(sg, k, obj, ogeom, normals, boxes, rest, counters, nullptr);
}

// gather_geometry with the sources as a kernel argument (p3d_scene_refit_device: no staging buffer, nothing to outlive the
// call): at most kMaxArgSources, sorted and with `before` filled like the staged ones.  The thread's source is picked by a
// chain of selects over constant indices - a search through the argument by a run-time index would first copy the table to
// scratch.  counters: the scene's own block, added to and never cleared here; *status takes kStatusRefitSkipped with them.
// The launch covers n_objs threads (total <= n_objs): thread i also zeroes visits[i], the fit's arrival counters, which
// spares the stream a memset launch between this kernel and the fit (lbvh::enqueue_fit, visits_clear).
constexpr uint32_t kMaxArgSources = 16;
struct ArgSources {
  StagedSource s[kMaxArgSources];
};
__global__ void gather_geometry_args(const ArgSources table, uint32_t n_sources, uint32_t total, uint32_t n_objs, float4* ogeom,
                                     float4* normals, float4* boxes, float4* rest, uint32_t* counters, uint32_t* status, uint32_t* visits) {
  const uint32_t i = blockIdx.x * lbvh::kThreads + threadIdx.x;
  if (i < n_objs) visits[i] = 0u;
  if (i >= total) return;
  StagedSource sg = table.s[0];
#pragma unroll
  for (uint32_t r = 1; r < kMaxArgSources; ++r)
    if (r < n_sources && table.s[r].before <= i) sg = table.s[r];  // (sorted: the last one with before <= i stays)
  const uint32_t k = i - sg.before, obj = sg.first + k;
  if (k >= sg.count || obj >= n_objs) return;
  gather_object(sg, k, obj, ogeom, normals, boxes, rest, counters, status);
}

}  // namespace upd
}  // namespace p3d
