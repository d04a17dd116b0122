// nearest_rule.hpp — the arithmetic of a nearest-surface query, in ONE place for its users: p3d_host_scene_nearest and
// p3d_host_scene_nearest_k (host_queries.cpp), which state the semantics by brute force, and nearest_k_device_kernel
// (csrc/nearest_query.hpp), whose answers must be the host forms' bits.  For a point p and an object's nine geometry floats (what p3d_prim.v holds for its
// kind) nearest_point gives the closest point q on the object's SURFACE and d2 = |p - q|^2, taken from q as stored.  Also
// here: the squared distance from p to a BVH node's box, and the two comparisons of a search - which candidate wins, and
// when a node may be dropped.  float32 throughout, evaluated as written; both translation units are compiled without
// contraction (-ffp-contract=off) and with correctly rounded square root and division (prim_rule.hpp).
#pragma once

#include <cmath>

#include "p3d.h"
#include "prim_rule.hpp"

namespace p3d {

// A node is dropped only if its box lies farther than the search radius times this.  The box distance and a primitive's d2
// are rounded along different paths (worst: a sphere touched along an axis, |p - c| - r cancels), so a bare `box_d2 > best`
// could drop the node that holds the object the brute force chooses.  A judgement, not a derived bound (DESIGN.md
// "Nearest-surface queries").
constexpr float kNearestSlack = 1.0f + 0x1p-10f;

// |p - q|^2 as every user sums it
P3D_PRIM_HD inline float nearest_d2(const float p[3], const float q[3]) {
  const float dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
  return (dx * dx + dy * dy) + dz * dz;
}

P3D_PRIM_HD inline float nearest_dot(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// Closest point on the closed triangle A B C: a vertex, an edge or the face, by the Voronoi region p lies in; the regions are
// told apart by the signs of the barycentric numerators, the point is built from A (an edge BC: from B)
P3D_PRIM_HD inline void nearest_on_triangle(const float v[9], const float p[3], float q[3]) {
  const float* a = v;
  const float* b = v + 3;
  const float* c = v + 6;
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const float d1 = nearest_dot(ab, ap), d2 = nearest_dot(ac, ap);
  if (d1 <= 0.0f && d2 <= 0.0f) {  // vertex A
    q[0] = a[0]; q[1] = a[1]; q[2] = a[2];
    return;
  }
  const float bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
  const float d3 = nearest_dot(ab, bp), d4 = nearest_dot(ac, bp);
  if (d3 >= 0.0f && d4 <= d3) {  // vertex B
    q[0] = b[0]; q[1] = b[1]; q[2] = b[2];
    return;
  }
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) {  // edge AB
    const float t = d1 / (d1 - d3);
    for (int k = 0; k < 3; ++k) q[k] = a[k] + ab[k] * t;
    return;
  }
  const float cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const float d5 = nearest_dot(ab, cp), d6 = nearest_dot(ac, cp);
  if (d6 >= 0.0f && d5 <= d6) {  // vertex C
    q[0] = c[0]; q[1] = c[1]; q[2] = c[2];
    return;
  }
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) {  // edge AC
    const float t = d2 / (d2 - d6);
    for (int k = 0; k < 3; ++k) q[k] = a[k] + ac[k] * t;
    return;
  }
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) {  // edge BC
    const float t = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    for (int k = 0; k < 3; ++k) q[k] = b[k] + (c[k] - b[k]) * t;
    return;
  }
  const float denom = 1.0f / ((va + vb) + vc);  // the face
  const float s = vb * denom, t = vc * denom;
  for (int k = 0; k < 3; ++k) q[k] = (a[k] + ab[k] * s) + ac[k] * t;
}

// q = c + (p - c) * (r / |p - c|), inside and outside alike: the surface, not the solid.  p == c: q = c + (r, 0, 0)
P3D_PRIM_HD inline void nearest_on_sphere(const float v[9], const float p[3], float q[3]) {
  const float d[3] = {p[0] - v[0], p[1] - v[1], p[2] - v[2]};
  const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  if (len == 0.0f) {
    q[0] = v[0] + v[3]; q[1] = v[1]; q[2] = v[2];
    return;
  }
  const float s = v[3] / len;
  for (int k = 0; k < 3; ++k) q[k] = v[k] + d[k] * s;
}

// Outside: the clamp of p to the box.  Inside or on it: p moved onto the nearest face; ties go to the lowest axis, then the
// min face.  (A NaN coordinate is "outside" and stays: its d2 is a NaN, which wins nothing.)
P3D_PRIM_HD inline void nearest_on_box(const float v[9], const float p[3], float q[3]) {
  const float* lo = v;
  const float* hi = v + 3;
  const bool inside = p[0] >= lo[0] && p[0] <= hi[0] && p[1] >= lo[1] && p[1] <= hi[1] && p[2] >= lo[2] && p[2] <= hi[2];
  if (!inside) {
    for (int k = 0; k < 3; ++k) q[k] = p[k] < lo[k] ? lo[k] : (p[k] > hi[k] ? hi[k] : p[k]);
    return;
  }
  int axis = 0;
  bool max_face = false;
  float least = p[0] - lo[0];
  for (int k = 0; k < 3; ++k) {
    const float to_min = p[k] - lo[k], to_max = hi[k] - p[k];
    if (to_min < least) { least = to_min; axis = k; max_face = false; }
    if (to_max < least) { least = to_max; axis = k; max_face = true; }
  }
  for (int k = 0; k < 3; ++k) q[k] = k == axis ? (max_face ? hi[k] : lo[k]) : p[k];
}

// q = p - ((p - A).N) N with the unit normal the scene stores: v = {N, A}
P3D_PRIM_HD inline void nearest_on_plane(const float v[9], const float p[3], float q[3]) {
  const float w[3] = {p[0] - v[3], p[1] - v[4], p[2] - v[5]};
  const float h = nearest_dot(w, v);
  for (int k = 0; k < 3; ++k) q[k] = p[k] - v[k] * h;
}

// -> d2, and q
P3D_PRIM_HD inline float nearest_point(uint32_t kind, const float v[9], const float p[3], float q[3]) {
  if (kind == P3D_PRIM_TRIANGLE) nearest_on_triangle(v, p, q);
  else if (kind == P3D_PRIM_SPHERE) nearest_on_sphere(v, p, q);
  else if (kind == P3D_PRIM_BOX) nearest_on_box(v, p, q);
  else nearest_on_plane(v, p, q);
  return nearest_d2(p, q);
}

// Squared distance from p to the box lo..hi: the sum of the squared clamped offsets, 0 inside.  A NaN bound clamps nothing
P3D_PRIM_HD inline float nearest_box_d2(const float p[3], const float lo[3], const float hi[3]) {
  const float dx = p[0] < lo[0] ? lo[0] - p[0] : (p[0] > hi[0] ? p[0] - hi[0] : 0.0f);
  const float dy = p[1] < lo[1] ? lo[1] - p[1] : (p[1] > hi[1] ? p[1] - hi[1] : 0.0f);
  const float dz = p[2] < lo[2] ? lo[2] - p[2] : (p[2] > hi[2] ? p[2] - hi[2] : 0.0f);
  return (dx * dx + dy * dy) + dz * dz;
}

// The cull, as a positive test: a NaN on either side drops nothing
P3D_PRIM_HD inline bool nearest_culls(float box_d2, float best) { return box_d2 > best * kNearestSlack; }

// Does (d2, object) beat the best so far?  The smaller d2, then the smaller object index: a total order, so the answer does
// not depend on the order of the visits.  A search starts at (radius^2, -1): nothing at or beyond the radius gets in
P3D_PRIM_HD inline bool nearest_wins(float d2, int32_t object, float best, int32_t best_object) {
  return d2 < best || (d2 == best && object < best_object);
}

// The squared radius a search starts with: +inf without a limit; with one, only max_dist > 0 finds anything (a NaN: nothing)
P3D_PRIM_HD inline bool nearest_radius(bool limited, float max_dist, float& best) {
  best = limited ? max_dist * max_dist : INFINITY;
  return !limited || max_dist > 0.0f;
}

// ---- the k nearest objects within a radius (p3d_host_scene_nearest_k, nearest_k_device_kernel) -----------------------------------
// A candidate list of at most k entries, sorted ascending by (d2, object): the order of nearest_wins.  The list itself lives
// where its user keeps it (an array on the host, LDS on the device) and is reached through four members:
//   float d2(uint32_t e) ; int32_t object(uint32_t e) ; void move(uint32_t to, uint32_t from) ; void set(uint32_t e, float d2,
//   int32_t object, uint32_t slot)          (slot: where the object's geometry lives, for the user's own use)
// Every object lies in exactly one leaf of both kinds of tree (and is visited once by a brute force), so a search offers it
// once: no de-duplication is needed, and none is done.

// What a candidate must beat to enter, and what a node is culled against.  While the list holds fewer than k entries it is
// (radius^2, -1), the start of a k = 1 search: d2 < radius^2 gets in.  Once the list is full it is the last entry, which an
// admitted candidate drops out.  One comparison for both states: nearest_wins(d2, object, gate.d2, gate.object); the cull is
// nearest_culls(box_d2, gate.d2), with the slack of the k = 1 search.  A NaN d2 wins against nothing and never enters.
struct NearestKGate {
  float d2;
  int32_t object;
};

// The gate of an empty list; false: the limit keeps nothing (nearest_radius)
P3D_PRIM_HD inline bool nearest_k_open(bool limited, float max_dist, NearestKGate& gate) {
  gate.object = -1;
  return nearest_radius(limited, max_dist, gate.d2);
}

P3D_PRIM_HD inline bool nearest_k_admits(float d2, int32_t object, const NearestKGate& gate) {
  return nearest_wins(d2, object, gate.d2, gate.object);
}

// Puts an ADMITTED candidate where it belongs: the entries it wins against move one place down, the last one of a full list
// out.  Updates count and the gate
template <class List>
P3D_PRIM_HD inline void nearest_k_insert(List& list, uint32_t& count, uint32_t k, NearestKGate& gate, float d2, int32_t object, uint32_t slot) {
  uint32_t e = count < k ? count++ : k - 1;
  for (; e > 0 && nearest_wins(d2, object, list.d2(e - 1), list.object(e - 1)); --e) list.move(e, e - 1);
  list.set(e, d2, object, slot);
  if (count == k) { gate.d2 = list.d2(k - 1); gate.object = list.object(k - 1); }
}

}  // namespace p3d
