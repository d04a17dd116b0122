// overlap_rule.hpp — does an object touch an axis-aligned box?  In ONE place for its users: p3d_host_scene_overlap_box
// (host_queries.cpp), which states the semantics by brute force, and overlap_box_device_kernel (csrc/overlap_query.hpp), whose
// answers must be the host form's bits.  For a query box lo .. hi (closed) and an object's nine geometry floats (what
// p3d_prim.v holds for its kind) overlap_box says whether the box overlaps the object's SURFACE - the closed triangle, a
// sphere's shell, a box's faces, the plane: the surface p3d_nearest_device measures to - or, with P3D_OVERLAP_SOLID, the solid
// sphere and the solid box.  Touching counts.  float32 throughout, evaluated as written; both translation units are compiled
// without contraction (-ffp-contract=off).  No division and no square root anywhere.
//
// TWO STAGES.  The first, for every kind but the plane, is plain comparisons of the query box against the object's own box as
// prim_rule.hpp makes it (a triangle: the extent of its vertices, which lies inside the stored box, grown by kPrimEps; a
// sphere: sphere_box, the stored box's bits; a box: its min and max): no arithmetic of this header.  So a true answer implies
// that the two boxes overlap by comparison, and with it every box that contains the object's by min / max: the tree is walked
// without slack (DESIGN.md "Overlap queries" has the argument).  Every test is a positive one: a NaN is never an overlap.
#pragma once

#include <cmath>

#include "p3d.h"
#include "nearest_rule.hpp"  // nearest_box_d2
#include "prim_rule.hpp"

namespace p3d {

// A query box finds something only if lo <= hi on every axis (a NaN: nothing).  Asked once per query, in front of the objects
P3D_PRIM_HD inline bool overlap_query_open(const float lo[3], const float hi[3]) {
  return lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
}

// Two closed boxes share a point: comparisons only, exact
P3D_PRIM_HD inline bool overlap_boxes(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3]) {
  return alo[0] <= bhi[0] && ahi[0] >= blo[0] && alo[1] <= bhi[1] && ahi[1] >= blo[1] && alo[2] <= bhi[2] && ahi[2] >= blo[2];
}
// The walk's side of the same fact: the boxes are APART on some axis.  For numbers the exact complement of overlap_boxes; a
// positive test too, so a NaN bound drops no node
P3D_PRIM_HD inline bool overlap_boxes_apart(const float alo[3], const float ahi[3], const float blo[3], const float bhi[3]) {
  return alo[0] > bhi[0] || ahi[0] < blo[0] || alo[1] > bhi[1] || ahi[1] < blo[1] || alo[2] > bhi[2] || ahi[2] < blo[2];
}

// ONE formulation of a separating axis, for all ten axes of a triangle: INTERVAL SUMS WITHOUT A CENTRE.  The triangle's
// interval on the axis a is the min and max of the three a . v_i; the box's is the sum over the coordinates of a_k lo_k or
// a_k hi_k, chosen by the sign of a_k.  The axis separates only if the gap between the intervals is strictly positive.
// Nothing is translated to a centre and no half extent is formed: the box's corners enter as given, so a box that is a point
// or a slab has an interval of exactly that, and a coordinate shared by a vertex and a face meets itself in the same
// product on both sides.  A null axis gives two intervals [0, 0] and separates nothing.
// The general form, for the triangle's normal:
P3D_PRIM_HD inline bool overlap_axis_separates(const float a[3], const float v[9], const float lo[3], const float hi[3]) {
  const float t0 = (a[0] * v[0] + a[1] * v[1]) + a[2] * v[2];
  const float t1 = (a[0] * v[3] + a[1] * v[4]) + a[2] * v[5];
  const float t2 = (a[0] * v[6] + a[1] * v[7]) + a[2] * v[8];
  const float t_min = prim_lo(prim_lo(t0, t1), t2), t_max = prim_hi(prim_hi(t0, t1), t2);
  const float b_min = ((a[0] > 0.0f ? a[0] * lo[0] : a[0] * hi[0]) + (a[1] > 0.0f ? a[1] * lo[1] : a[1] * hi[1])) + (a[2] > 0.0f ? a[2] * lo[2] : a[2] * hi[2]);
  const float b_max = ((a[0] > 0.0f ? a[0] * hi[0] : a[0] * lo[0]) + (a[1] > 0.0f ? a[1] * hi[1] : a[1] * lo[1])) + (a[2] > 0.0f ? a[2] * hi[2] : a[2] * lo[2]);
  return t_min > b_max || t_max < b_min;
}
// The same for an axis with a zero component, the product of an edge with a coordinate axis: the two live components ap, aq on
// the coordinates P, Q; the dead one is not multiplied
template <int P, int Q>
P3D_PRIM_HD inline bool overlap_axis2_separates(float ap, float aq, const float v[9], const float lo[3], const float hi[3]) {
  const float t0 = ap * v[P] + aq * v[Q], t1 = ap * v[3 + P] + aq * v[3 + Q], t2 = ap * v[6 + P] + aq * v[6 + Q];
  const float t_min = prim_lo(prim_lo(t0, t1), t2), t_max = prim_hi(prim_hi(t0, t1), t2);
  const float b_min = (ap > 0.0f ? ap * lo[P] : ap * hi[P]) + (aq > 0.0f ? aq * lo[Q] : aq * hi[Q]);
  const float b_max = (ap > 0.0f ? ap * hi[P] : ap * lo[P]) + (aq > 0.0f ? aq * hi[Q] : aq * lo[Q]);
  return t_min > b_max || t_max < b_min;
}
// The three products of the edge e with x, y and z: x^ x e = (0, -e_z, e_y), y^ x e = (e_z, 0, -e_x), z^ x e = (-e_y, e_x, 0)
P3D_PRIM_HD inline bool overlap_edge_separates(float ex, float ey, float ez, const float v[9], const float lo[3], const float hi[3]) {
  return overlap_axis2_separates<1, 2>(-ez, ey, v, lo, hi) || overlap_axis2_separates<0, 2>(ez, -ex, v, lo, hi) ||
         overlap_axis2_separates<0, 1>(-ey, ex, v, lo, hi);
}

// The closed triangle A B C.  Stage 1: the extent of the vertices (prim_lo / prim_hi in triangle_normal_box's order) against
// the query box: the three face normals of the box as axes.  Stage 2: the normal (B - A) x (C - A), then the edges A B, B C,
// C A, each with x, y, z.  A zero-area triangle has a null normal, and parallel (a segment) or null (a point) edges: the
// axes that are left are those of a segment against a box, which decide it, or none, and stage 1 has decided a point
P3D_PRIM_HD inline bool overlap_triangle(const float v[9], const float lo[3], const float hi[3]) {
  const float tlo[3] = {prim_lo(prim_lo(v[0], v[3]), v[6]), prim_lo(prim_lo(v[1], v[4]), v[7]), prim_lo(prim_lo(v[2], v[5]), v[8])};
  const float thi[3] = {prim_hi(prim_hi(v[0], v[3]), v[6]), prim_hi(prim_hi(v[1], v[4]), v[7]), prim_hi(prim_hi(v[2], v[5]), v[8])};
  if (!overlap_boxes(lo, hi, tlo, thi)) return false;
  const float abx = v[3] - v[0], aby = v[4] - v[1], abz = v[5] - v[2];
  const float acx = v[6] - v[0], acy = v[7] - v[1], acz = v[8] - v[2];
  const float n[3] = {aby * acz - abz * acy, abz * acx - abx * acz, abx * acy - aby * acx};
  if (overlap_axis_separates(n, v, lo, hi)) return false;
  if (overlap_edge_separates(abx, aby, abz, v, lo, hi)) return false;
  if (overlap_edge_separates(v[6] - v[3], v[7] - v[4], v[8] - v[5], v, lo, hi)) return false;
  if (overlap_edge_separates(-acx, -acy, -acz, v, lo, hi)) return false;
  return true;
}

// The sphere c, r: v = {c, r}.  Stage 1: sphere_box against the query box.  Stage 2: the box comes within r of the centre
// (nearest_box_d2, the walk's measure of the point query), and, for the shell, some corner lies at r or beyond: per axis the
// farther of the two faces, max(c - lo, hi - c), which is not negative for lo <= hi
P3D_PRIM_HD inline bool overlap_sphere(const float v[9], const float lo[3], const float hi[3], bool solid) {
  float slo[3], shi[3];
  sphere_box(v, v[3], slo, shi);
  if (!overlap_boxes(lo, hi, slo, shi)) return false;
  const float r2 = v[3] * v[3];
  if (!(nearest_box_d2(v, lo, hi) <= r2)) return false;
  if (solid) return true;
  const float fx = prim_hi(v[0] - lo[0], hi[0] - v[0]), fy = prim_hi(v[1] - lo[1], hi[1] - v[1]), fz = prim_hi(v[2] - lo[2], hi[2] - v[2]);
  return (fx * fx + fy * fy) + fz * fz >= r2;
}

// The box v = {min, max}.  Stage 1 is the solid's whole test.  The faces: the query box must not lie strictly inside the open
// interior.  Comparisons only: exact
P3D_PRIM_HD inline bool overlap_aabox(const float v[9], const float lo[3], const float hi[3], bool solid) {
  if (!overlap_boxes(lo, hi, v, v + 3)) return false;
  if (solid) return true;
  const bool inside = lo[0] > v[0] && hi[0] < v[3] && lo[1] > v[1] && hi[1] < v[4] && lo[2] > v[2] && hi[2] < v[5];
  return !inside;
}

// The plane v = {N, A}: the heights (x - A) . N of the eight corners; the smallest and the largest take, per axis, the face
// the sign of N's component names.  There is no first stage: a plane has no box (and no place in the tree)
P3D_PRIM_HD inline bool overlap_plane(const float v[9], const float lo[3], const float hi[3]) {
  const float l[3] = {lo[0] - v[3], lo[1] - v[4], lo[2] - v[5]}, h[3] = {hi[0] - v[3], hi[1] - v[4], hi[2] - v[5]};
  const float min_h = ((v[0] > 0.0f ? v[0] * l[0] : v[0] * h[0]) + (v[1] > 0.0f ? v[1] * l[1] : v[1] * h[1])) + (v[2] > 0.0f ? v[2] * l[2] : v[2] * h[2]);
  const float max_h = ((v[0] > 0.0f ? v[0] * h[0] : v[0] * l[0]) + (v[1] > 0.0f ? v[1] * h[1] : v[1] * l[1])) + (v[2] > 0.0f ? v[2] * h[2] : v[2] * l[2]);
  return min_h <= 0.0f && max_h >= 0.0f;
}

// Does the OPEN query box (overlap_query_open) lo .. hi overlap the object?  flags: 0 or P3D_OVERLAP_SOLID
P3D_PRIM_HD inline bool overlap_box(uint32_t kind, const float v[9], const float lo[3], const float hi[3], uint32_t flags) {
  const bool solid = (flags & P3D_OVERLAP_SOLID) != 0;
  if (kind == P3D_PRIM_TRIANGLE) return overlap_triangle(v, lo, hi);
  if (kind == P3D_PRIM_SPHERE) return overlap_sphere(v, lo, hi, solid);
  if (kind == P3D_PRIM_BOX) return overlap_aabox(v, lo, hi, solid);
  return overlap_plane(v, lo, hi);
}

}  // namespace p3d
