// nearest_segment_rule.hpp — the arithmetic of a nearest-surface query for a SEGMENT (an edge of a cloth mesh, the axis of a
// capsule, a piece of rope), in ONE place for its users: p3d_host_scene_nearest_segment_k (host_queries.cpp), which states the
// semantics by brute force, and nearest_segment_k_device_kernel (csrc/nearest_segment_query.hpp), whose answers must be the host
// form's bits.  For a segment a b and an object's nine geometry floats (what p3d_prim.v holds for its kind) segment_nearest
// gives the parameter s in [0, 1] of the point of the segment nearest to the object's SURFACE (nearest_rule.hpp: a sphere's
// shell inside and outside alike, the closed triangle, the plane), that point x = a + (b - a) s, the point q of the object
// nearest to it and d2 = |x - q|^2 from x and q as stored.  A segment that CROSSES the surface - it pierces the triangle, enters
// or leaves the shell, crosses the plane - has x = q, the crossing nearest to a, and d2 = +0.0 exactly.  Also here: the key of a
// BVH node, segment_box_d2.  The order of two candidates, the gate and the cull are nearest_rule.hpp's.  float32 throughout,
// evaluated as written; both translation units are compiled without contraction (-ffp-contract=off) and with correctly rounded
// square root and division (prim_rule.hpp).
#pragma once

#include <cmath>

#include "nearest_rule.hpp"

namespace p3d {

// x(s) = a + (b - a) s, as every user forms it.  x(0) is a; x(1) is a + (b - a), which may miss b by a rounding.  Rounding is
// monotone, so for 0 <= s <= 1 every coordinate of x(s) lies between those of x(0) and x(1): the extent segment_box_d2 takes
P3D_PRIM_HD inline void segment_at(const float a[3], const float b[3], float s, float x[3]) {
  for (int k = 0; k < 3; ++k) x[k] = a[k] + (b[k] - a[k]) * s;
}

// (a NaN stays a NaN: it makes a NaN d2, which wins nothing)
P3D_PRIM_HD inline float segment_clamp01(float t) { return t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t); }

// ha, hb: the signed heights of a and b over a plane (times any positive factor).  Does the closed segment meet the plane, and
// where first?  A positive test: a NaN height meets nothing.  a on the plane: s = 0; both on it: s = 0 as well
P3D_PRIM_HD inline bool segment_crosses(float ha, float hb, float& s) {
  if (!((ha <= 0.0f && hb >= 0.0f) || (ha >= 0.0f && hb <= 0.0f))) return false;
  s = ha == 0.0f ? 0.0f : ha / (ha - hb);  // same signs above and below, |ha - hb| >= |ha| after rounding too: 0 < s <= 1
  return true;
}

// The closest pair of the segments a b (parameter s) and p0 p1 (parameter t), by the textbook clamping in a FIXED order: the
// unclamped s of the two lines, clamped; the t nearest to x(s); if that t leaves [0, 1] it is clamped and s is taken again for
// the clamped end.  A degenerate segment (squared length 0, which a tiny one underflows to) is its first point; parallel lines
// (a zero determinant) start from s = 0.  Near-parallel lines make the first s uncertain, not the distance: along the common
// direction the distance is flat, and t and then s are taken again for what the first step chose
P3D_PRIM_HD inline void segment_pair(const float a[3], const float b[3], const float p0[3], const float p1[3], float& s, float& t) {
  const float d1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float d2[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const float r[3] = {a[0] - p0[0], a[1] - p0[1], a[2] - p0[2]};
  const float A = nearest_dot(d1, d1), E = nearest_dot(d2, d2), F = nearest_dot(d2, r);
  if (A == 0.0f) {
    s = 0.0f;
    t = E == 0.0f ? 0.0f : segment_clamp01(F / E);
    return;
  }
  const float C = nearest_dot(d1, r);
  if (E == 0.0f) {
    t = 0.0f;
    s = segment_clamp01(-C / A);
    return;
  }
  const float B = nearest_dot(d1, d2);
  const float det = A * E - B * B;
  s = det != 0.0f ? segment_clamp01((B * F - C * E) / det) : 0.0f;
  t = (B * s + F) / E;
  if (t < 0.0f) {
    t = 0.0f;
    s = segment_clamp01(-C / A);
  } else if (t > 1.0f) {
    t = 1.0f;
    s = segment_clamp01((B - C) / A);
  }
}

// Is x, a point of the triangle's plane, in the closed triangle?  Three edge functions against n = (B - A) x (C - A); they do not
// see a shift of x along n
P3D_PRIM_HD inline bool segment_in_triangle(const float v[9], const float n[3], const float x[3]) {
  bool in = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 3; ++k) {
    const float* from = v + 3 * k;
    const float* to = v + 3 * ((k + 1) % 3);
    const float e[3] = {to[0] - from[0], to[1] - from[1], to[2] - from[2]};
    const float u[3] = {x[0] - from[0], x[1] - from[1], x[2] - from[2]};
    const float cr[3] = {e[1] * u[2] - e[2] * u[1], e[2] * u[0] - e[0] * u[2], e[0] * u[1] - e[1] * u[0]};
    in = in && nearest_dot(cr, n) >= 0.0f;
  }
  return in;
}

// One running best of the triangle's candidates: a candidate replaces it only if it is strictly nearer, so on a tie the first
// in the order wins.  x is not kept: it is segment_at of the kept s, the bits d2 was taken from
struct SegmentBest {
  float d2, s;
  float q[3];
};
P3D_PRIM_HD inline void segment_offer(SegmentBest& best, bool first, float s, const float x[3], const float q[3]) {
  const float d2 = nearest_d2(x, q);
  if (first || d2 < best.d2) {
    best.d2 = d2; best.s = s;
    best.q[0] = q[0]; best.q[1] = q[1]; best.q[2] = q[2];
  }
}

// Triangle A B C.  First the piercing test: the segment meets the triangle's plane (not lying in it) at a point of the closed
// triangle; that point is x and q, d2 = +0.  Otherwise the nearest pair has a point of the segment's that is an endpoint, or
// a point of the triangle's that lies on an edge (were both interior, the segment could be moved closer along the face, or
// it pierces); so the minimum over five candidates, evaluated in sequence against one running best, in this order: x(0) and
// x(1) through nearest_on_triangle, then the edges A B, B C, C A through segment_pair
P3D_PRIM_HD inline float segment_triangle(const float v[9], const float a[3], const float b[3], float& s, float x[3], float q[3]) {
  const float ab[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
  const float ac[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
  const float n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
  const float wa[3] = {a[0] - v[0], a[1] - v[1], a[2] - v[2]};
  const float wb[3] = {b[0] - v[0], b[1] - v[1], b[2] - v[2]};
  const float ha = nearest_dot(wa, n), hb = nearest_dot(wb, n);  // heights times |n|
  float cross;
  if (!(ha == 0.0f && hb == 0.0f) && segment_crosses(ha, hb, cross)) {
    segment_at(a, b, cross, x);
    if (segment_in_triangle(v, n, x)) {
      s = cross;
      q[0] = x[0]; q[1] = x[1]; q[2] = x[2];
      return 0.0f;
    }
  }
  SegmentBest best;
  float c[3];
  segment_at(a, b, 0.0f, x);
  nearest_on_triangle(v, x, c);
  segment_offer(best, true, 0.0f, x, c);
  segment_at(a, b, 1.0f, x);
  nearest_on_triangle(v, x, c);
  segment_offer(best, false, 1.0f, x, c);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 3; ++k) {
    const float* p0 = v + 3 * k;
    const float* p1 = v + 3 * ((k + 1) % 3);
    float t;
    segment_pair(a, b, p0, p1, s, t);
    segment_at(a, b, s, x);
    for (int j = 0; j < 3; ++j) c[j] = p0[j] + (p1[j] - p0[j]) * t;
    segment_offer(best, false, s, x, c);
  }
  s = best.s;
  segment_at(a, b, s, x);
  q[0] = best.q[0]; q[1] = best.q[1]; q[2] = best.q[2];
  return best.d2;
}

// Sphere (centre m, radius r): its shell.  g(s) = |x(s) - m| is convex: its minimum is at the foot of m on the segment, its
// maximum at an endpoint.  Three cases, each a positive test (a NaN: d2 is a NaN):
//   outside  : min g > r.  x is the foot, q the shell's point under it
//   inside   : g(0) < r and g(1) < r.  The shell is nearest to the endpoint farthest from m; on a tie that is a
//   crossing : min g <= r <= max g.  x = q is the first s with g(s) = r: from outside the smaller root, from inside the larger
//              one, from the shell s = 0; the roots in sweep_rule.hpp's forms without a cancellation
P3D_PRIM_HD inline float segment_sphere(const float v[9], const float a[3], const float b[3], float& s, float x[3], float q[3]) {
  const float r = v[3];
  const float d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float w[3] = {a[0] - v[0], a[1] - v[1], a[2] - v[2]};
  const float dd = nearest_dot(d, d), wd = nearest_dot(w, d), ww = nearest_dot(w, w);
  const float foot = dd > 0.0f ? segment_clamp01(-wd / dd) : 0.0f;
  float e[3];
  segment_at(a, b, 1.0f, e);
  segment_at(a, b, foot, x);
  const float we[3] = {e[0] - v[0], e[1] - v[1], e[2] - v[2]};
  const float wx[3] = {x[0] - v[0], x[1] - v[1], x[2] - v[2]};
  const float ga = sqrtf(ww), gb = sqrtf(nearest_dot(we, we)), gm = sqrtf(nearest_dot(wx, wx));
  if (gm > r) {
    s = foot;
  } else if (ga < r && gb < r) {
    s = ga >= gb ? 0.0f : 1.0f;
    segment_at(a, b, s, x);
  } else if (gm <= r && (ga >= r || gb >= r)) {
    const float k = wd / dd;
    const float p[3] = {w[0] - d[0] * k, w[1] - d[1] * k, w[2] - d[2] * k};  // the foot of m on the line, from m
    float h2 = r * r - nearest_dot(p, p);
    if (!(h2 > 0.0f)) h2 = 0.0f;  // (gm and p round differently)
    const float root = sqrtf(h2 * dd), c0 = ww - r * r;
    if (!(dd > 0.0f)) s = 0.0f;
    else if (ga > r) s = segment_clamp01(c0 / (root - wd));                                     // wd < 0: the foot lies ahead
    else if (ga < r) s = segment_clamp01(wd > 0.0f ? -c0 / (wd + root) : (root - wd) / dd);
    else s = 0.0f;
    segment_at(a, b, s, x);
    q[0] = x[0]; q[1] = x[1]; q[2] = x[2];
    return s == s ? 0.0f : s;
  } else {
    s = 0.0f;
    segment_at(a, b, s, x);
    q[0] = x[0]; q[1] = x[1]; q[2] = x[2];
    return NAN;
  }
  nearest_on_sphere(v, x, q);
  return nearest_d2(x, q);
}

// Plane (v = {N, A}, N unit): the signed height is linear in s.  The segment crosses (or touches) the plane: x = q there, at a
// itself if a lies on it.  Otherwise the endpoint of the smaller |height|, a on a tie, and its foot
P3D_PRIM_HD inline float segment_plane(const float v[9], const float a[3], const float b[3], float& s, float x[3], float q[3]) {
  const float wa[3] = {a[0] - v[3], a[1] - v[4], a[2] - v[5]};
  const float wb[3] = {b[0] - v[3], b[1] - v[4], b[2] - v[5]};
  const float ha = nearest_dot(wa, v), hb = nearest_dot(wb, v);
  if (segment_crosses(ha, hb, s)) {
    segment_at(a, b, s, x);
    q[0] = x[0]; q[1] = x[1]; q[2] = x[2];
    return 0.0f;
  }
  s = fabsf(ha) <= fabsf(hb) ? 0.0f : 1.0f;
  segment_at(a, b, s, x);
  nearest_on_plane(v, x, q);
  return nearest_d2(x, q);
}

// -> d2, and s, x, q.  a == b in all three coordinates is a point: nearest_point at a, s = +0, x = a - every bit of the
// point query's answer.  A box is not part of this query (the entry points refuse a scene that holds one): a NaN, which wins
// nothing
P3D_PRIM_HD inline float segment_nearest(uint32_t kind, const float v[9], const float a[3], const float b[3], float& s, float x[3], float q[3]) {
  if (a[0] == b[0] && a[1] == b[1] && a[2] == b[2]) {
    s = 0.0f;
    x[0] = a[0]; x[1] = a[1]; x[2] = a[2];
    return nearest_point(kind, v, a, q);
  }
  if (kind == P3D_PRIM_TRIANGLE) return segment_triangle(v, a, b, s, x, q);
  if (kind == P3D_PRIM_SPHERE) return segment_sphere(v, a, b, s, x, q);
  if (kind == P3D_PRIM_PLANE) return segment_plane(v, a, b, s, x, q);
  s = 0.0f;
  for (int k = 0; k < 3; ++k) x[k] = q[k] = a[k];
  return NAN;
}

// ---- the traversal's key (nearest_segment_k_device_kernel under P3D_ACCEL_BVH) -----------------------------------------------------
// A lower bound of the squared distance from the segment to anything in the box lo..hi: per axis, the gap between the
// segment's own extent and the box's, 0 where they overlap; the sum of the squares.
//   - every x the rule forms is segment_at(a, b, s) with 0 <= s <= 1, whose coordinate k lies between a[k] and
//     a[k] + (b[k] - a[k]) by the monotony of rounding (segment_at): the extent is taken from THOSE two, not from b, so it
//     holds x exactly, in float32 and not only in real numbers;
//   - every q lies in the box of its object, which lies in the node's, up to the rounding of q itself (a point of an edge or
//     a shell is built by a multiply and an add);
//   - so |x[k] - q[k]| is at least the gap of axis k for every pair the rule measures, and d2 = |x - q|^2 at least the sum of
//     the squared gaps, up to that rounding of q and the three roundings of each sum.  This is the situation of the point
//     query (nearest_box_d2 against nearest_point), and kNearestSlack, under which nearest_culls takes the bound, is the
//     allowance it makes there.  For a == b it IS nearest_box_d2: the same values.
// Not exact: a segment that runs diagonally past a box is farther than its extent's gap.  It is tight where the segment is
// short against the boxes it is culled against - edges, links.  A NaN bound of a node gives a gap of 0 on its axis: it culls
// nothing.  (A NaN in the segment: every d2 is a NaN and nothing is found, whatever is culled.)
P3D_PRIM_HD inline float segment_box_d2(const float a[3], const float b[3], const float lo[3], const float hi[3]) {
  float g[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 3; ++k) {
    const float e = a[k] + (b[k] - a[k]);
    const float least = a[k] < e ? a[k] : e, most = a[k] < e ? e : a[k];
    g[k] = most < lo[k] ? lo[k] - most : (least > hi[k] ? least - hi[k] : 0.0f);
  }
  return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

}  // namespace p3d
