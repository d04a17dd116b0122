// sweep_rule.hpp — the arithmetic of a sphere sweep (continuous collision detection of a moving ball), in ONE place for its
// users: p3d_host_scene_sweep_sphere (host_queries.cpp), which states the semantics by brute force, and sweep_sphere_device_kernel
// (csrc/sweep_query.hpp), whose answers must be the host form's bits.  A ball of radius r moves with its centre on
// c(t) = o + t d (d as given: t is in units of d).  For an object's nine geometry floats (what p3d_prim.v holds for its kind)
// sweep_contact gives T = min { t >= 0 : dist(c(t)) <= r }, dist being the distance to the object's SURFACE as
// nearest_rule.hpp's nearest_point defines it: sphere shell inside and outside alike, closed triangle, plane.  Also here: the
// entry parameter of the ray into a BVH node's box grown by the ball, and the two comparisons of a search - which contact
// wins, and when a node may be dropped.  float32 throughout, evaluated as written; both translation units are compiled
// without contraction (-ffp-contract=off) and with correctly rounded square root and division (prim_rule.hpp).
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "nearest_rule.hpp"

namespace p3d {

// A node is dropped only if the ray enters its grown box later than the best contact time (or the limit) times this, and
// the box is grown by r times this plus kSweepPad.  The entry parameter and an object's T are rounded along different paths
// (worst: a start that just touches, where T = 0 comes from nearest_point's d2 <= r^2 and the entry from three slab
// quotients), so a bare `entry > best` against the box grown by r alone could drop the node that holds the object the brute
// force chooses.  The factor covers the relative error of a root, the pad (the scene's own EPSILON, by which a triangle's box
// is grown already) a start at the surface where r is zero or tiny.  A judgement, not a derived bound (DESIGN.md "Sphere
// sweeps").
constexpr float kSweepSlack = 1.0f + 0x1p-10f;
constexpr float kSweepPad = kPrimEps;

constexpr int32_t kSweepNoObject = INT32_MAX;  // the object a search starts with: every real index beats it on a tie

// One query, as every user holds it.  ok: the query can find something at all
struct SweepRay {
  float o[3], d[3];
  float r, rr;     // rr = r * r
  float dd;        // d . d; 0: the ball stands still, only a start that overlaps is a contact (T = 0)
  float limit;     // t_max, or FLT_MAX without one: a contact later than this is none
  bool ok;
};

// r NaN or negative, a NaN in o or d, a limit that is NaN or <= 0: nothing is found
P3D_PRIM_HD inline void sweep_ray(const float o[3], const float d[3], float r, bool limited, float t_max, SweepRay& s) {
  bool ok = r >= 0.0f && (!limited || t_max > 0.0f);
  for (int k = 0; k < 3; ++k) {
    s.o[k] = o[k]; s.d[k] = d[k];
    ok = ok && o[k] == o[k] && d[k] == d[k];
  }
  s.r = r; s.rr = r * r;
  s.dd = nearest_dot(d, d);
  s.limit = limited ? t_max : FLT_MAX;
  s.ok = ok;
}

// The line w + t d against the ball |x| <= rho about the origin, by the foot of the origin on the line: b = w.d, the foot
// p = w - d (b / dd), its squared length against rho^2.  -> false: the line misses the ball; else s = sqrt((rho^2 - p.p) dd),
// the half chord times dd: the roots are (-b -+ s) / dd.  p is formed as a vector, so no two squares of the distance to the
// obstacle are subtracted: the error of s is relative to rho^2, not to w.w (b^2 - dd c, the textbook discriminant, lost
// three digits on a ball far from a triangle it grazes)
P3D_PRIM_HD inline bool sweep_chord(const float w[3], const float d[3], float dd, float rho2, float& b, float& s) {
  b = nearest_dot(w, d);
  const float k = b / dd;
  const float p[3] = {w[0] - d[0] * k, w[1] - d[1] * k, w[2] - d[2] * k};
  const float h2 = rho2 - nearest_dot(p, p);
  if (!(h2 >= 0.0f)) return false;
  s = sqrtf(h2 * dd);
  return true;
}

// The first t >= 0 at which |w + t d| = rho, coming from outside (c = w.w - rho^2 > 0) and moving closer (b < 0): the smaller
// root, as c / (s - b): both terms of the divisor are positive, nothing cancels
P3D_PRIM_HD inline bool sweep_enter_ball(const float w[3], const float d[3], float dd, float rho2, float& t) {
  const float c = nearest_dot(w, w) - rho2;
  float b, s;
  if (!(c > 0.0f) || !(dd > 0.0f) || !sweep_chord(w, d, dd, rho2, b, s) || !(b < 0.0f)) return false;
  t = c / (s - b);
  return true;
}

// The same where the ball is the whole obstacle (a sphere from outside, a vertex): c <= 0 is a start that touches.  The
// caller's overlap test rounds differently and may have let it through by an ulp: T = 0
P3D_PRIM_HD inline bool sweep_enter_ball_or_touch(const float w[3], const float d[3], float dd, float rho2, float& t) {
  if (nearest_dot(w, w) - rho2 <= 0.0f) {
    t = 0.0f;
    return true;
  }
  return sweep_enter_ball(w, d, dd, rho2, t);
}

// Sphere (centre m, radius R): from outside the shell the ball meets it when |c(t) - m| = R + r (the smaller root); from
// inside, when |c(t) - m| = R - r (the larger root: the centre leaves the ball of that radius).  The caller has seen that
// the start does not overlap, so R - r > 0 inside
P3D_PRIM_HD inline bool sweep_sphere(const float v[9], const SweepRay& s, float& t) {
  const float w[3] = {s.o[0] - v[0], s.o[1] - v[1], s.o[2] - v[2]};
  const float ww = nearest_dot(w, w);
  if (sqrtf(ww) > v[3]) {
    const float rho = v[3] + s.r;
    return sweep_enter_ball_or_touch(w, s.d, s.dd, rho * rho, t);
  }
  const float rho = v[3] - s.r;
  const float c = ww - rho * rho;  // < 0: inside
  if (c >= 0.0f) {  // (as in sweep_enter_ball_or_touch)
    t = 0.0f;
    return true;
  }
  float b, root;
  if (!(c < 0.0f) || !sweep_chord(w, s.d, s.dd, rho * rho, b, root)) return false;
  t = b > 0.0f ? -c / (b + root) : (root - b) / s.dd;  // the larger root, the form without a cancellation
  return true;
}

// Plane (v = {N, A}, N unit): the signed height h(t) = (c(t) - A).N reaches +r from above or -r from below, only when the
// centre moves towards the plane
P3D_PRIM_HD inline bool sweep_plane(const float v[9], const SweepRay& s, float& t) {
  const float w[3] = {s.o[0] - v[3], s.o[1] - v[4], s.o[2] - v[5]};
  const float h0 = nearest_dot(w, v), hd = nearest_dot(s.d, v);
  const bool above = h0 > 0.0f;
  if (above ? !(hd < 0.0f) : !(hd > 0.0f)) return false;
  const float q = ((above ? s.r : -s.r) - h0) / hd;
  t = q > 0.0f ? q : 0.0f;  // (the overlap test and h0 round differently: a start it let through by an ulp touches at 0)
  return true;
}

// The ray against the cylinder of radius r about the edge p0 p1, entered from outside, with the foot of c(t) on the edge
// (foot parameter in [0, 1]).  With e = p1 - p0 and w = o - p0: the parts of w and d across the edge, as vectors, meet the
// disc of radius r as a ray meets a ball
P3D_PRIM_HD inline bool sweep_edge(const float* p0, const float* p1, const SweepRay& s, float& t) {
  const float e[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
  const float w[3] = {s.o[0] - p0[0], s.o[1] - p0[1], s.o[2] - p0[2]};
  const float ee = nearest_dot(e, e), we = nearest_dot(w, e), de = nearest_dot(s.d, e);
  const float kw = we / ee, kd = de / ee;
  const float wx[3] = {w[0] - e[0] * kw, w[1] - e[1] * kw, w[2] - e[2] * kw};
  const float dx[3] = {s.d[0] - e[0] * kd, s.d[1] - e[1] * kd, s.d[2] - e[2] * kd};
  float q;
  if (!sweep_enter_ball(wx, dx, nearest_dot(dx, dx), s.rr, q)) return false;  // (along the edge, or a point for an edge: the vertices decide)
  const float foot = we + q * de;  // times e.e
  if (!(foot >= 0.0f && foot <= ee)) return false;
  t = q;
  return true;
}

P3D_PRIM_HD inline bool sweep_vertex(const float* p, const SweepRay& s, float& t) {
  const float w[3] = {s.o[0] - p[0], s.o[1] - p[1], s.o[2] - p[2]};
  return sweep_enter_ball_or_touch(w, s.d, s.dd, s.rr, t);
}

// Is x, a point of the triangle's plane, in the closed triangle?  Three edge functions against n = (b - a) x (c - a)
P3D_PRIM_HD inline bool sweep_in_triangle(const float* a, const float* b, const float* c, const float n[3], const float x[3]) {
  const float* from[3] = {a, b, c};
  const float* to[3] = {b, c, a};
  bool in = true;
  for (int k = 0; k < 3; ++k) {
    const float e[3] = {to[k][0] - from[k][0], to[k][1] - from[k][1], to[k][2] - from[k][2]};
    const float u[3] = {x[0] - from[k][0], x[1] - from[k][1], x[2] - from[k][2]};
    const float cr[3] = {e[1] * u[2] - e[2] * u[1], e[2] * u[0] - e[0] * u[2], e[0] * u[1] - e[1] * u[0]};
    in = in && nearest_dot(cr, n) >= 0.0f;
  }
  return in;
}

// Triangle a b c.  The face: the centre reaches the plane offset by r on the side it starts on; taken only if the foot of
// c(t) on the plane lies in the closed triangle, and then it is the triangle's answer (before it the centre is farther than
// r from the plane).  Otherwise the smallest root among the three edge cylinders and the three vertex spheres: each is a
// contact with a part of the triangle, so none is earlier than the first contact, and the first contact is one of them
P3D_PRIM_HD inline bool sweep_triangle(const float v[9], const SweepRay& s, float& t) {
  const float* a = v;
  const float* b = v + 3;
  const float* c = v + 6;
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float n[3] = {ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]};
  const float w[3] = {s.o[0] - a[0], s.o[1] - a[1], s.o[2] - a[2]};
  const float h0 = nearest_dot(w, n), hd = nearest_dot(s.d, n);  // heights times |n|
  const float off = s.r * sqrtf(nearest_dot(n, n));
  const bool above = h0 > 0.0f;
  if ((above ? h0 > off : -h0 > off) && (above ? hd < 0.0f : hd > 0.0f)) {
    const float q = ((above ? off : -off) - h0) / hd;
    const float cq[3] = {s.o[0] + s.d[0] * q, s.o[1] + s.d[1] * q, s.o[2] + s.d[2] * q};
    // the foot of c(q): c(q) less its height along n, which is +-off / |n| there; the edge functions do not see a shift along n
    if (q >= 0.0f && sweep_in_triangle(a, b, c, n, cq)) {
      t = q;
      return true;
    }
  }
  bool found = false;
  float best = 0.0f, q;
  if (sweep_edge(a, b, s, q) && (!found || q < best)) { best = q; found = true; }
  if (sweep_edge(b, c, s, q) && (!found || q < best)) { best = q; found = true; }
  if (sweep_edge(c, a, s, q) && (!found || q < best)) { best = q; found = true; }
  if (sweep_vertex(a, s, q) && (!found || q < best)) { best = q; found = true; }
  if (sweep_vertex(b, s, q) && (!found || q < best)) { best = q; found = true; }
  if (sweep_vertex(c, s, q) && (!found || q < best)) { best = q; found = true; }
  t = best;
  return found;
}

// -> whether the ball meets the object at all, and T.  A start that overlaps (nearest_point's d2 <= r^2) is T = 0 for every
// kind.  A box is not swept (the entry points refuse a scene that holds one)
P3D_PRIM_HD inline bool sweep_contact(uint32_t kind, const float v[9], const SweepRay& s, float& t) {
  if (kind == P3D_PRIM_BOX) return false;
  float q[3];
  if (nearest_point(kind, v, s.o, q) <= s.rr) {
    t = 0.0f;
    return true;
  }
  if (!(s.dd > 0.0f)) return false;
  bool hit;
  if (kind == P3D_PRIM_TRIANGLE) hit = sweep_triangle(v, s, t);
  else if (kind == P3D_PRIM_SPHERE) hit = sweep_sphere(v, s, t);
  else hit = sweep_plane(v, s, t);
  return hit && t >= 0.0f;
}

// c(T), as every user forms it
P3D_PRIM_HD inline void sweep_centre(const SweepRay& s, float t, float c[3]) {
  for (int k = 0; k < 3; ++k) c[k] = s.o[k] + s.d[k] * t;
}

// Does (T, object) beat the best so far?  The smaller T, then the smaller object index: a total order, so the answer does
// not depend on the order of the visits.  A search starts at (limit, kSweepNoObject): T == limit still gets in, nothing later
P3D_PRIM_HD inline bool sweep_wins(float t, int32_t object, float best_t, int32_t best_object) {
  return t < best_t || (t == best_t && object < best_object);
}

// ---- the traversal's key (sweep_sphere_device_kernel under P3D_ACCEL_BVH) -------------------------------------------------------------
// What the slab test needs of a query, made once: 1 / d per axis (unused where d is 0) and by how much a box is grown.  The
// box grown by g on every side contains the Minkowski sum of box and ball for g >= r, so the test is conservative
struct SweepSlabs {
  float inv[3];
  float grow;
};
P3D_PRIM_HD inline void sweep_slabs(const SweepRay& s, SweepSlabs& k) {
  for (int a = 0; a < 3; ++a) k.inv[a] = 1.0f / s.d[a];
  k.grow = s.r * kSweepSlack + kSweepPad;
}

// The ray against the box lo..hi grown by k.grow -> false: the ray (t >= 0) misses it; true and the entry parameter, 0 when
// the origin is inside.  Every drop is a positive test: an axis with a NaN bound constrains nothing
P3D_PRIM_HD inline bool sweep_box_entry(const SweepRay& s, const SweepSlabs& k, const float lo[3], const float hi[3], float& entry) {
  float t_in = 0.0f, t_out = INFINITY;
  bool miss = false;
  for (int a = 0; a < 3; ++a) {
    const float l = (lo[a] - k.grow) - s.o[a], h = (hi[a] + k.grow) - s.o[a];  // the slab, seen from the origin
    if (s.d[a] == 0.0f) {
      miss = miss || l > 0.0f || h < 0.0f;
    } else {
      const float t0 = l * k.inv[a], t1 = h * k.inv[a];
      if (t0 <= t1) {
        t_in = t0 > t_in ? t0 : t_in; t_out = t1 < t_out ? t1 : t_out;
      } else if (t1 < t0) {
        t_in = t1 > t_in ? t1 : t_in; t_out = t0 < t_out ? t0 : t_out;
      }
    }
  }
  entry = t_in;
  return !(miss || t_in > t_out);
}

// The cull, as a positive test: a NaN on either side drops nothing.  best: the best T so far, the limit before there is one
P3D_PRIM_HD inline bool sweep_culls(float entry, float best) { return entry > best * kSweepSlack; }

}  // namespace p3d
