// host_queries.cpp — the p3d_host_scene_* queries of include/p3d*.h: every per-object query stated by brute force on the CPU,
// from the rule headers the kernels share.  Pure host code (no HIP).  What the statements have in common is written once: the
// packed view of the scene (pack_scene), the k-list search (k_list_search), the choice of the filters' source (with_host_filters).
#include <cfloat>
#include <cmath>
#include <string>
#include <vector>

#include "filter_rule.hpp"
#include "host_scene.hpp"
#include "nearest_rule.hpp"
#include "nearest_segment_rule.hpp"
#include "occlusion_rule.hpp"
#include "overlap_rule.hpp"
#include "p3d_error.hpp"
#include "query_refusals.hpp"
#include "sweep_rule.hpp"

namespace {

// The objects of a host scene as the rules take them: nine floats and a kind each, and the index of the first box (-1: none)
struct PackedScene {
  std::vector<float> v;
  std::vector<uint32_t> kind;
  int n_objs = 0, first_box = -1;
  const float* geom(int j) const { return &v[9 * static_cast<size_t>(j)]; }
};
PackedScene pack_scene(const p3d_host_scene& hs) {
  PackedScene ps;
  ps.n_objs = hs.scene.getNumObjects();
  ps.v.resize(9 * static_cast<size_t>(ps.n_objs));
  ps.kind.resize(ps.n_objs);
  for (int j = 0; j < ps.n_objs; ++j) {
    float normal[3];
    hs.scene.getObject(j)->pack(&ps.v[9 * static_cast<size_t>(j)], normal);
    ps.kind[j] = static_cast<uint32_t>(hs.scene.getObject(j)->kind());
    if (ps.kind[j] == P3D_PRIM_BOX && ps.first_box < 0) ps.first_box = j;
  }
  return ps;
}

// the candidate list of nearest_rule.hpp as the host keeps it: k entries in an array
struct HostNearestList {
  struct Entry { float d2; int32_t object; };
  Entry e_[P3D_NEAREST_K_MAX];
  float d2(uint32_t e) const { return e_[e].d2; }
  int32_t object(uint32_t e) const { return e_[e].object; }
  void move(uint32_t to, uint32_t from) { e_[to] = e_[from]; }
  void set(uint32_t e, float d2, int32_t object, uint32_t) { e_[e] = Entry{d2, object}; }
};

// Where a host form's queries get their filters from (filter_rule.hpp): the skip arrays of the call, or nothing
struct HostFilters {
  const int32_t* skip;
  uint32_t n_skip;
  const int32_t* skip_range;
  p3d::QueryFilter load(uint32_t i, uint32_t n_objs) const { return p3d::filter_load(n_skip ? skip : nullptr, n_skip, skip_range, i, n_objs); }
};
struct NoHostFilters {
  p3d::NoFilter load(uint32_t, uint32_t) const { return p3d::NoFilter{}; }
};
// The filter arguments of an entry point, refused or handed to body(filters) -> its code.  A call that names no filter runs
// the unfiltered instantiation, whose bits the filtered one promises for it anyway
template <class Body>
int with_host_filters(const std::string& pre, uint32_t n, const int32_t* skip, uint32_t n_skip, const int32_t* skip_range, Body&& body) {
  if (n_skip > P3D_FILTER_SKIP_MAX) return p3d::fail(P3D_ERR_INVALID, pre + p3d::kRefuseSkipCount);
  if (n && n_skip > 0 && !skip) return p3d::fail(P3D_ERR_INVALID, pre + "null skip with n > 0 and n_skip > 0");
  if (n_skip == 0 && !skip_range) return body(NoHostFilters{});
  return body(HostFilters{skip, n_skip, skip_range});
}

// The k-list search of the k-nearest queries: rule(i, j, x) -> d2 on every object j that the filter of query i does not name,
// in object order; the k smallest (d2, object index) under the limit in that order, counted, and k rows written: object and
// dist here, the rule's other outputs by store(row, x).  x, an Extra, starts as the row of nothing found.  It is not kept in
// the list: the rule is run once more on each listed object, which gives the same bits
template <class Extra, class Filters, class Rule, class Store>
void k_list_search(const PackedScene& ps, uint32_t n, uint32_t k, const float* max_dist, const Filters& filters, int32_t* count,
                   int32_t* object, float* dist, Rule&& rule, Store&& store) {
  using namespace p3d;
  for (uint32_t i = 0; i < n; ++i) {
    HostNearestList list;
    NearestKGate gate;
    uint32_t found = 0;
    const auto filter = filters.load(i, static_cast<uint32_t>(ps.n_objs));
    if (nearest_k_open(max_dist != nullptr, max_dist ? max_dist[i] : 0.0f, gate)) {
      for (int j = 0; j < ps.n_objs; ++j) {
        if (filter_skips(filter, j)) continue;
        Extra x;
        const float d2 = rule(i, j, x);
        if (nearest_k_admits(d2, j, gate)) nearest_k_insert(list, found, k, gate, d2, j, static_cast<uint32_t>(j));
      }
    }
    count[i] = static_cast<int32_t>(found);
    for (uint32_t e = 0; e < k; ++e) {
      const size_t row = static_cast<size_t>(i) * k + e;
      Extra x;
      const int32_t j = e < found ? list.object(e) : -1;
      if (j >= 0) rule(i, j, x);
      object[row] = j;
      if (dist) dist[row] = j >= 0 ? sqrtf(list.d2(e)) : FLT_MAX;
      store(row, x);
    }
  }
}

// The statement of the k-nearest query: nearest_rule.hpp under k_list_search
template <class Filters>
int host_nearest_k(const std::string& pre, p3d_host_scene* hs, uint32_t n, uint32_t k, const float* points, const float* max_dist,
                   const Filters& filters, int32_t* count, int32_t* object, float* dist, float* closest) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, pre + "null scene");
  if (k == 0 || k > P3D_NEAREST_K_MAX) return p3d::fail(P3D_ERR_INVALID, pre + p3d::kRefuseNearestK);
  if (n && (!points || !count || !object)) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  const PackedScene ps = pack_scene(*hs);
  struct Extra { float q[3] = {0.0f, 0.0f, 0.0f}; };
  k_list_search<Extra>(
      ps, n, k, max_dist, filters, count, object, dist,
      [&](uint32_t i, int j, Extra& x) { return p3d::nearest_point(ps.kind[j], ps.geom(j), points + 3 * static_cast<size_t>(i), x.q); },
      [&](size_t row, const Extra& x) {
        if (closest)
          for (int c = 0; c < 3; ++c) closest[3 * row + c] = x.q[c];
      });
  return P3D_OK;
}

// The statement of the nearest-surfaces-to-a-segment query: nearest_segment_rule.hpp under k_list_search
template <class Filters>
int host_nearest_segment_k(const std::string& pre, p3d_host_scene* hs, uint32_t n, uint32_t k, const float* a, const float* b,
                           const float* max_dist, const Filters& filters, int32_t* count, int32_t* object, float* dist, float* param,
                           float* on_segment, float* closest) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, pre + "null scene");
  const PackedScene ps = pack_scene(*hs);
  if (ps.first_box >= 0) return p3d::fail(P3D_ERR_UNSUPPORTED, pre + p3d::refuse_box(ps.first_box, p3d::kSegmentNoBox));
  if (k == 0 || k > P3D_NEAREST_K_MAX) return p3d::fail(P3D_ERR_INVALID, pre + p3d::kRefuseNearestK);
  if (n && (!a || !b || !count || !object)) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  struct Extra { float s = FLT_MAX, x[3] = {0.0f, 0.0f, 0.0f}, q[3] = {0.0f, 0.0f, 0.0f}; };
  k_list_search<Extra>(
      ps, n, k, max_dist, filters, count, object, dist,
      [&](uint32_t i, int j, Extra& x) {
        return p3d::segment_nearest(ps.kind[j], ps.geom(j), a + 3 * static_cast<size_t>(i), b + 3 * static_cast<size_t>(i), x.s, x.x, x.q);
      },
      [&](size_t row, const Extra& x) {
        if (param) param[row] = x.s;
        for (int c = 0; c < 3; ++c) {
          if (on_segment) on_segment[3 * row + c] = x.x[c];
          if (closest) closest[3 * row + c] = x.q[c];
        }
      });
  return P3D_OK;
}

// The statement of the sphere sweep: sweep_rule.hpp on every object the query's filter does not name, the smallest (T, object
// index) within the limit wins.  contact is not kept during the search: nearest_point is run once more at c(T) on the object found
template <class Filters>
int host_sweep_sphere(const std::string& pre, const p3d_host_scene* hs, uint32_t n, const float* origin, const float* direction,
                      const float* radius, const float* t_max, const Filters& filters, int32_t* object, float* t, float* centre,
                      float* contact) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, pre + "null scene");
  using namespace p3d;
  const PackedScene ps = pack_scene(*hs);
  if (ps.first_box >= 0) return p3d::fail(P3D_ERR_UNSUPPORTED, pre + refuse_box(ps.first_box, kSweepNoBox));
  if (n && (!origin || !direction || !radius || !object)) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  for (uint32_t i = 0; i < n; ++i) {
    const size_t row = 3 * static_cast<size_t>(i);
    SweepRay s;
    sweep_ray(origin + row, direction + row, radius[i], t_max != nullptr, t_max ? t_max[i] : 0.0f, s);
    float best = s.limit;
    int32_t best_object = kSweepNoObject;
    const auto filter = filters.load(i, static_cast<uint32_t>(ps.n_objs));
    if (s.ok) {
      for (int j = 0; j < ps.n_objs; ++j) {
        if (filter_skips(filter, j)) continue;
        float T;
        if (sweep_contact(ps.kind[j], ps.geom(j), s, T) && sweep_wins(T, j, best, best_object)) {
          best = T; best_object = j;
        }
      }
    }
    const bool found = best_object != kSweepNoObject;
    float c[3] = {0.0f, 0.0f, 0.0f}, q[3] = {0.0f, 0.0f, 0.0f};
    if (found) {
      sweep_centre(s, best, c);
      nearest_point(ps.kind[best_object], ps.geom(best_object), c, q);
    }
    object[i] = found ? best_object : -1;
    if (t) t[i] = found ? best : FLT_MAX;
    for (int k = 0; k < 3; ++k) {
      if (centre) centre[row + k] = c[k];
      if (contact) contact[row + k] = q[k];
    }
  }
  return P3D_OK;
}

// The statement of the overlap query: overlap_rule.hpp on every object the box's filter does not name, in object order; all
// of them counted, the first k listed (object order is index order: the k lowest, ascending)
template <class Filters>
int host_overlap_box(const std::string& pre, p3d_host_scene* hs, uint32_t n, uint32_t k, const float* lo, const float* hi,
                     const Filters& filters, uint32_t flags, int32_t* total, int32_t* object) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, pre + "null scene");
  if (k > P3D_NEAREST_K_MAX) return p3d::fail(P3D_ERR_INVALID, pre + p3d::kRefuseOverlapK);
  if (flags & ~P3D_OVERLAP_SOLID) return p3d::fail(P3D_ERR_INVALID, pre + p3d::kRefuseOverlapFlag);
  if (n && (!lo || !hi || !total || (k > 0 && !object))) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  using namespace p3d;
  const PackedScene ps = pack_scene(*hs);
  for (uint32_t i = 0; i < n; ++i) {
    const float* qlo = lo + 3 * static_cast<size_t>(i);
    const float* qhi = hi + 3 * static_cast<size_t>(i);
    int32_t* row = k ? object + static_cast<size_t>(i) * k : nullptr;
    uint32_t found = 0;
    const auto filter = filters.load(i, static_cast<uint32_t>(ps.n_objs));
    if (overlap_query_open(qlo, qhi)) {
      for (int j = 0; j < ps.n_objs; ++j) {
        if (filter_skips(filter, j)) continue;
        if (!overlap_box(ps.kind[j], ps.geom(j), qlo, qhi, flags)) continue;
        if (found < k) row[found] = j;
        ++found;
      }
    }
    total[i] = static_cast<int32_t>(found);
    for (uint32_t e = found; e < k; ++e) row[e] = -1;
  }
  return P3D_OK;
}

}  // namespace

extern "C" {

// The statement of the nearest-surface query: nearest_rule.hpp on every object, the smallest (d2, object index) wins
int p3d_host_scene_nearest(p3d_host_scene* hs, uint32_t n, const float* points, const float* max_dist, int32_t* object, float* dist,
                           float* closest) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_nearest: null scene");
  if (n && (!points || !object)) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_nearest: null array with n > 0");
  using namespace p3d;
  const PackedScene ps = pack_scene(*hs);
  for (uint32_t i = 0; i < n; ++i) {
    const float* p = points + 3 * static_cast<size_t>(i);
    float best, best_q[3] = {0.0f, 0.0f, 0.0f};
    int32_t best_object = -1;
    if (nearest_radius(max_dist != nullptr, max_dist ? max_dist[i] : 0.0f, best)) {
      for (int j = 0; j < ps.n_objs; ++j) {
        float q[3];
        const float d2 = nearest_point(ps.kind[j], ps.geom(j), p, q);
        if (nearest_wins(d2, j, best, best_object)) {
          best = d2; best_object = j;
          best_q[0] = q[0]; best_q[1] = q[1]; best_q[2] = q[2];
        }
      }
    }
    const bool found = best_object >= 0;
    object[i] = best_object;
    if (dist) dist[i] = found ? sqrtf(best) : FLT_MAX;
    if (closest)
      for (int k = 0; k < 3; ++k) closest[3 * static_cast<size_t>(i) + k] = found ? best_q[k] : 0.0f;
  }
  return P3D_OK;
}

int p3d_host_scene_nearest_k(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* points, const float* max_dist, int32_t* count,
                             int32_t* object, float* dist, float* closest) {
  return host_nearest_k("p3d_host_scene_nearest_k: ", hs, n, k, points, max_dist, NoHostFilters{}, count, object, dist, closest);
}
int p3d_host_scene_nearest_k_filtered(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* points, const float* max_dist,
                                      const int32_t* skip, uint32_t n_skip, const int32_t* skip_range, int32_t* count, int32_t* object,
                                      float* dist, float* closest) {
  const std::string pre = "p3d_host_scene_nearest_k_filtered: ";
  return with_host_filters(pre, n, skip, n_skip, skip_range, [&](const auto& filters) {
    return host_nearest_k(pre, hs, n, k, points, max_dist, filters, count, object, dist, closest);
  });
}

int p3d_host_scene_sweep_sphere(const p3d_host_scene* hs, uint32_t n, const float* origin, const float* direction, const float* radius,
                                const float* t_max, int32_t* object, float* t, float* centre, float* contact) {
  return host_sweep_sphere("p3d_host_scene_sweep_sphere: ", hs, n, origin, direction, radius, t_max, NoHostFilters{}, object, t, centre, contact);
}
int p3d_host_scene_sweep_sphere_filtered(const p3d_host_scene* hs, uint32_t n, const float* origin, const float* direction,
                                         const float* radius, const float* t_max, const int32_t* skip, uint32_t n_skip,
                                         const int32_t* skip_range, int32_t* object, float* t, float* centre, float* contact) {
  const std::string pre = "p3d_host_scene_sweep_sphere_filtered: ";
  return with_host_filters(pre, n, skip, n_skip, skip_range, [&](const auto& filters) {
    return host_sweep_sphere(pre, hs, n, origin, direction, radius, t_max, filters, object, t, centre, contact);
  });
}

int p3d_host_scene_nearest_segment_k(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* a, const float* b, const float* max_dist,
                                     const int32_t* skip, uint32_t n_skip, const int32_t* skip_range, int32_t* count, int32_t* object,
                                     float* dist, float* param, float* on_segment, float* closest) {
  const std::string pre = "p3d_host_scene_nearest_segment_k: ";
  return with_host_filters(pre, n, skip, n_skip, skip_range, [&](const auto& filters) {
    return host_nearest_segment_k(pre, hs, n, k, a, b, max_dist, filters, count, object, dist, param, on_segment, closest);
  });
}

// The key of a BVH node under the segment query, for the tests (host only)
int p3d_debug_segment_box_d2(uint32_t n, const float* a, const float* b, const float* lo, const float* hi, float* out) {
  if (n && (!a || !b || !lo || !hi || !out)) return p3d::fail(P3D_ERR_INVALID, "p3d_debug_segment_box_d2: null array with n > 0");
  for (size_t i = 0; i < n; ++i) out[i] = p3d::segment_box_d2(a + 3 * i, b + 3 * i, lo + 3 * i, hi + 3 * i);
  return P3D_OK;
}

int p3d_host_scene_overlap_box(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* lo, const float* hi, const int32_t* skip,
                               uint32_t n_skip, const int32_t* skip_range, uint32_t flags, int32_t* total, int32_t* object) {
  const std::string pre = "p3d_host_scene_overlap_box: ";
  return with_host_filters(pre, n, skip, n_skip, skip_range, [&](const auto& filters) {
    return host_overlap_box(pre, hs, n, k, lo, hi, filters, flags, total, object);
  });
}

// The statement of the rays of p3d_occlusion_device: occlusion_rule.hpp for every (point, sample), row i * samples + j
int p3d_occlusion_rays(uint32_t n, const float* point, const float* normal, const p3d_occlusion_params* params, float* origin,
                       float* direction) {
  const std::string pre = "p3d_occlusion_rays: ";
  if (const char* why = p3d::occlusion_params_refusal(params)) return p3d::fail(P3D_ERR_INVALID, pre + why);
  if (n == 0) return P3D_OK;
  if (!point || !normal || !origin || !direction) return p3d::fail(P3D_ERR_INVALID, pre + "null argument");
  if (static_cast<uint64_t>(n) * params->samples > 0xffffffffull)
    return p3d::fail(P3D_ERR_CAPACITY, pre + "n x samples rows do not fit 32 bits (split the batch)");
  for (uint32_t i = 0; i < n; ++i) {
    p3d::OcclusionFrame f;
    p3d::occlusion_frame(point + 3 * static_cast<size_t>(i), normal + 3 * static_cast<size_t>(i), params->bias, f);
    for (uint32_t j = 0; j < params->samples; ++j) {
      const size_t row = static_cast<size_t>(i) * params->samples + j;
      p3d::occlusion_direction(f, params->seed, params->point_offset + i, params->sample_begin + j, direction + 3 * row);
      for (int k = 0; k < 3; ++k) origin[3 * row + k] = f.origin[k];
    }
  }
  return P3D_OK;
}

}  // extern "C"
