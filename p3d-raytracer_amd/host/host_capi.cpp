// host_capi.cpp — the p3d_host_* half of include/p3d.h: .p3f -> Scene -> accel builds ->
// flat p3d_scene_desc.  Pure host code (no HIP).
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "accel_build.hpp"
#include "nearest_rule.hpp"
#include "nearest_segment_rule.hpp"
#include "occlusion_rule.hpp"
#include "overlap_rule.hpp"
#include "filter_rule.hpp"
#include "p3d.h"
#include "p3d_error.hpp"
#include "scene_model.hpp"
#include "sweep_rule.hpp"

struct p3d_host_scene {
  p3d::Scene scene;
  std::unique_ptr<p3d::BVH> bvh;
  std::unique_ptr<p3d::Grid> grid;
  std::vector<p3d_prim> prims;
  std::vector<p3d_material> materials;
  std::vector<p3d_light> lights;
  p3d_scene_desc desc{};
  bool flat_valid = false;
};

namespace {

// The p3d_camera of a constructed Camera (camera.h:34-63): what p3d_host_scene_desc and p3d_camera_look_at hand out.
void pack_camera(const p3d::Camera& c, p3d_camera& k) {
  k = p3d_camera{};
  k.eye[0] = c.eye.x; k.eye[1] = c.eye.y; k.eye[2] = c.eye.z;
  k.u[0] = c.u.x; k.u[1] = c.u.y; k.u[2] = c.u.z;
  k.v[0] = c.v.x; k.v[1] = c.v.y; k.v[2] = c.v.z;
  k.n[0] = c.n.x; k.n[1] = c.n.y; k.n[2] = c.n.z;
  k.plane_dist = c.plane_dist; k.w = c.w; k.h = c.h; k.focal_ratio = c.focal_ratio;
  k.aperture = c.aperture; k.res_x = c.res_x; k.res_y = c.res_y;
}

void flatten(p3d_host_scene& hs) {
  using namespace p3d;
  const Scene& S = hs.scene;
  hs.prims.assign(S.getNumObjects(), p3d_prim{});
  for (int i = 0; i < S.getNumObjects(); ++i) {
    const Object* o = S.getObject(i);
    p3d_prim& p = hs.prims[i];
    o->pack(p.v, p.n);
    p.type = static_cast<uint32_t>(o->kind());
    p.material = static_cast<uint32_t>(S.materialIndex(o->GetMaterial()));
    const AABB b = o->GetBoundingBox();
    p.bmin[0] = b.min.x; p.bmin[1] = b.min.y; p.bmin[2] = b.min.z;
    p.bmax[0] = b.max.x; p.bmax[1] = b.max.y; p.bmax[2] = b.max.z;
  }
  hs.materials.clear();
  for (const auto& m : S.allMaterials()) {
    p3d_material f{};
    const Color cd = m->GetDiffColor(), cs = m->GetSpecColor(), em = m->GetEmission();
    f.diff_color[0] = cd.r(); f.diff_color[1] = cd.g(); f.diff_color[2] = cd.b();
    f.spec_color[0] = cs.r(); f.spec_color[1] = cs.g(); f.spec_color[2] = cs.b();
    f.emission[0] = em.r(); f.emission[1] = em.g(); f.emission[2] = em.b();
    f.diffuse = m->GetDiffuse(); f.specular = m->GetSpecular(); f.shine = m->GetShine();
    f.transmittance = m->GetTransmittance(); f.refr_index = m->GetRefrIndex();
    f.reflection = m->GetReflection();
    hs.materials.push_back(f);
  }
  hs.lights.clear();
  for (int i = 0; i < S.getNumLights(); ++i) {
    const Light* l = S.getLight(i);
    p3d_light f{};
    f.position[0] = l->position.x; f.position[1] = l->position.y; f.position[2] = l->position.z;
    f.color[0] = l->color.r(); f.color[1] = l->color.g(); f.color[2] = l->color.b();
    hs.lights.push_back(f);
  }
  p3d_scene_desc& d = hs.desc;
  std::memset(&d, 0, sizeof(d));
  d.abi_version = P3D_ABI_VERSION;
  d.n_prims = static_cast<uint32_t>(hs.prims.size());
  d.n_materials = static_cast<uint32_t>(hs.materials.size());
  d.n_lights = static_cast<uint32_t>(hs.lights.size());
  d.prims = hs.prims.data();
  d.materials = hs.materials.data();
  d.lights = hs.lights.data();
  if (const Camera* c = S.GetCamera()) pack_camera(*c, d.camera);
  const Color bg = S.GetBackgroundColor();
  d.background[0] = bg.r(); d.background[1] = bg.g(); d.background[2] = bg.b();
  if (hs.bvh) {
    d.n_bvh_nodes = static_cast<uint32_t>(hs.bvh->flatNodes().size());
    d.bvh_nodes = hs.bvh->flatNodes().data();
    d.bvh_prim_index = hs.bvh->primOrder().data();
    d.n_bvh_prim_index = static_cast<uint32_t>(hs.bvh->primOrder().size());
    d.bvh_max_depth = hs.bvh->maxDepth();
  }
  if (hs.grid) {
    d.has_grid = 1;
    d.grid = hs.grid->describe();
  }
  hs.flat_valid = true;
}

std::vector<p3d::Object*> object_list(const p3d::Scene& S) {
  std::vector<p3d::Object*> v;
  for (int i = 0; i < S.getNumObjects(); ++i) v.push_back(S.getObject(i));
  return v;
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

}  // namespace

extern "C" {

int p3d_host_scene_load(const char* p3f_path, uint32_t flags, p3d_host_scene** out) {
  if (!p3f_path || !out) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_load: null argument");
  auto hs = std::make_unique<p3d_host_scene>();
  if (!hs->scene.load_p3f(p3f_path, (flags & P3D_LOAD_LEGACY_F11) != 0))
    return p3d::fail(P3D_ERR_IO, std::string("cannot open ") + p3f_path);
  *out = hs.release();
  return P3D_OK;
}

void p3d_host_scene_destroy(p3d_host_scene* hs) { delete hs; }

int p3d_host_scene_set_resolution(p3d_host_scene* hs, int32_t rx, int32_t ry) {
  if (!hs || !hs->scene.view.present) return p3d::fail(P3D_ERR_INVALID, "scene has no camera (`v` block)");
  if (rx > 0) hs->scene.view.xres = rx;
  if (ry > 0) hs->scene.view.yres = ry;
  hs->scene.rebuildCamera();
  hs->flat_valid = false;
  return P3D_OK;
}

int p3d_host_scene_set_lens(p3d_host_scene* hs, float aperture_ratio, float focal_ratio) {
  if (!hs || !hs->scene.view.present) return p3d::fail(P3D_ERR_INVALID, "scene has no camera (`v` block)");
  hs->scene.view.aperture = aperture_ratio;
  hs->scene.view.focal = focal_ratio;
  hs->scene.rebuildCamera();
  hs->flat_valid = false;
  return P3D_OK;
}

int p3d_host_scene_set_geometry(p3d_host_scene* hs, uint32_t n, const uint32_t* object, const float* v) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_geometry: null scene");
  if (n && (!object || !v)) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_geometry: null array with n > 0");
  using namespace p3d;
  const uint32_t n_objs = static_cast<uint32_t>(hs->scene.getNumObjects());
  for (uint32_t i = 0; i < n; ++i) {  // all or nothing
    if (object[i] >= n_objs) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_geometry: object index out of range");
    if (hs->scene.getObject(object[i])->kind() == Kind::Plane)
      return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_geometry: object " + std::to_string(object[i]) + " is a plane (three points make one; its nine floats are not them)");
  }
  if (n == 0) return P3D_OK;
  hs->bvh.reset();  // they hold pointers to the objects, and were built for the old boxes
  hs->grid.reset();
  hs->flat_valid = false;
  for (uint32_t i = 0; i < n; ++i) {
    const float* g = v + 9 * static_cast<size_t>(i);
    // what the loader's `s`, `p` and `box` handlers run (Scene::load_p3f)
    switch (hs->scene.getObject(object[i])->kind()) {
      case Kind::Sphere: hs->scene.replaceObject(object[i], new Sphere(Vector(g[0], g[1], g[2]), g[3])); break;
      case Kind::Triangle:
        hs->scene.replaceObject(object[i], new Triangle(Vector(g[0], g[1], g[2]), Vector(g[3], g[4], g[5]), Vector(g[6], g[7], g[8])));
        break;
      case Kind::Box: hs->scene.replaceObject(object[i], new aaBox(Vector(g[0], g[1], g[2]), Vector(g[3], g[4], g[5]))); break;
      case Kind::Plane: break;
    }
  }
  return P3D_OK;
}

// The records of materials [first, first + n) replaced in place: the objects keep their Material pointers, so a host BVH and
// grid already built stay valid; the next p3d_host_scene_desc flattens anew
int p3d_host_scene_set_materials(p3d_host_scene* hs, uint32_t first, uint32_t n, const p3d_material* materials) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_materials: null scene");
  const auto& all = hs->scene.allMaterials();
  if (static_cast<uint64_t>(first) + n > all.size())
    return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_materials: the range ends behind the scene's " + std::to_string(all.size()) + " materials");
  if (n && !materials) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_materials: null array with n > 0");
  if (n == 0) return P3D_OK;
  using namespace p3d;
  for (uint32_t i = 0; i < n; ++i) {
    const p3d_material& f = materials[i];
    Material& m = *all[first + i];
    m.SetDiffColor(Color(f.diff_color[0], f.diff_color[1], f.diff_color[2]));
    m.SetSpecColor(Color(f.spec_color[0], f.spec_color[1], f.spec_color[2]));
    m.SetEmission(Color(f.emission[0], f.emission[1], f.emission[2]));
    m.SetDiffuse(f.diffuse); m.SetSpecular(f.specular); m.SetShine(f.shine);
    m.SetTransmittance(f.transmittance); m.SetRefrIndex(f.refr_index);
    m.SetReflection(f.reflection);
  }
  hs->flat_valid = false;
  return P3D_OK;
}

// The same for lights [first, first + n) of the list as it is now (the replicated one after p3d_host_scene_replicate_lights)
int p3d_host_scene_set_lights(p3d_host_scene* hs, uint32_t first, uint32_t n, const p3d_light* lights) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_lights: null scene");
  const uint64_t count = static_cast<uint64_t>(hs->scene.getNumLights());
  if (static_cast<uint64_t>(first) + n > count)
    return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_lights: the range ends behind the scene's " + std::to_string(count) + " lights");
  if (n && !lights) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_set_lights: null array with n > 0");
  if (n == 0) return P3D_OK;
  using namespace p3d;
  for (uint32_t i = 0; i < n; ++i) {
    Light* l = hs->scene.getLight(first + i);
    l->position = Vector(lights[i].position[0], lights[i].position[1], lights[i].position[2]);
    l->color = Color(lights[i].color[0], lights[i].color[1], lights[i].color[2]);
  }
  hs->flat_valid = false;
  return P3D_OK;
}

// main.cpp:725-745: SPP x SPP copies of every light on a LIGHT_SIDE square, colour / SPP^2
int p3d_host_scene_replicate_lights(p3d_host_scene* hs, uint32_t spp_sqrt, float light_side) {
  if (!hs || spp_sqrt == 0) return p3d::fail(P3D_ERR_INVALID, "replicate_lights: bad argument");
  using namespace p3d;
  const int SPP = static_cast<int>(spp_sqrt);
  const float step = light_side / SPP;
  const float start = -light_side / 2 + step / 2;
  const float end = light_side / 2;
  std::vector<std::unique_ptr<Light>> grown;
  const int limit = hs->scene.getNumLights();
  for (int k = 0; k < limit; ++k) {
    const Light* light = hs->scene.getLight(k);
    const Color avg = light->color / static_cast<float>(SPP * SPP);
    for (float i = start; i < end; i += step)
      for (float j = start; j < end; j += step)
        grown.emplace_back(new Light(Vector(light->position.x + i, light->position.y + j, light->position.z), avg));
  }
  hs->scene.setLights(std::move(grown));
  hs->flat_valid = false;
  return P3D_OK;
}

int p3d_host_scene_desc(p3d_host_scene* hs, int build_bvh, int build_grid, const p3d_scene_desc** out) {
  if (!hs || !out) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_desc: null argument");
  for (int i = 0; i < hs->scene.getNumObjects(); ++i)
    if (!hs->scene.getObject(i)->GetMaterial())
      return p3d::fail(P3D_ERR_INVALID, "object declared before the first `f` line has no material");
  if (build_bvh && !hs->bvh) {  // built once: BVH::objs is append-only in the reference (bvh.cpp:101)
    hs->bvh = std::make_unique<p3d::BVH>();
    hs->bvh->build(object_list(hs->scene));
    hs->flat_valid = false;
  }
  if (build_grid && !hs->grid) {
    hs->grid = std::make_unique<p3d::Grid>();
    for (p3d::Object* o : object_list(hs->scene)) hs->grid->addObject(o);
    hs->grid->Build();
    hs->flat_valid = false;
  }
  if (!hs->flat_valid) flatten(*hs);
  *out = &hs->desc;
  return P3D_OK;
}

int p3d_host_scene_view(p3d_host_scene* hs, float from[3], float at[3], float up[3], float* angle, float* aperture_ratio,
                        float* focal_ratio) {
  if (!hs || !from || !at || !up || !angle || !aperture_ratio || !focal_ratio)
    return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_view: null argument");
  const p3d::Scene::ViewBlock& v = hs->scene.view;
  if (!v.present) return p3d::fail(P3D_ERR_INVALID, "scene has no camera (`v` block)");
  const p3d::Vector* src[3] = {&v.from, &v.at, &v.up};
  float* dst[3] = {from, at, up};
  for (int i = 0; i < 3; ++i) {
    dst[i][0] = src[i]->x; dst[i][1] = src[i]->y; dst[i][2] = src[i]->z;
  }
  *angle = v.angle;
  *aperture_ratio = v.aperture;
  *focal_ratio = v.focal;
  return P3D_OK;
}

// camera.h:34-63 as the loader runs it for a `v` block (Scene::rebuildCamera); hither / yon leave no trace in p3d_camera
int p3d_camera_look_at(const float from[3], const float at[3], const float up[3], float angle, int32_t res_x, int32_t res_y,
                       float aperture_ratio, float focal_ratio, p3d_camera* out) {
  if (!from || !at || !up || !out) return p3d::fail(P3D_ERR_INVALID, "p3d_camera_look_at: null argument");
  if (res_x <= 0 || res_y <= 0) return p3d::fail(P3D_ERR_INVALID, "p3d_camera_look_at: the resolution must be positive");
  const p3d::Camera c(p3d::Vector(from[0], from[1], from[2]), p3d::Vector(at[0], at[1], at[2]), p3d::Vector(up[0], up[1], up[2]), angle,
                      0.0f, 0.0f, res_x, res_y, aperture_ratio, focal_ratio);
  pack_camera(c, *out);
  return P3D_OK;
}

int p3d_host_scene_has_skybox(p3d_host_scene* hs) { return hs && hs->scene.SkyboxLoaded() ? 1 : 0; }

int p3d_host_scene_load_skybox(p3d_host_scene* hs, const char* sky_dir) {
  if (!hs || !sky_dir) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_load_skybox: null argument");
  return hs->scene.LoadSkybox(sky_dir) ? P3D_OK : P3D_ERR_IO;  // (the message names the face that could not be read)
}

int p3d_host_scene_skybox_face(p3d_host_scene* hs, int face, const uint8_t** img, uint32_t* res_x, uint32_t* res_y) {
  if (!hs || !img) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_skybox_face: null argument");
  *img = hs->scene.SkyboxFace(face, res_x, res_y);
  return *img ? P3D_OK : p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_skybox_face: no cubemap loaded, or face not in 0..5");
}

// The statement of the nearest-surface query: nearest_rule.hpp on every object, the smallest (d2, object index) wins
int p3d_host_scene_nearest(p3d_host_scene* hs, uint32_t n, const float* points, const float* max_dist, int32_t* object, float* dist,
                           float* closest) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_nearest: null scene");
  if (n && (!points || !object)) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_nearest: null array with n > 0");
  using namespace p3d;
  const int n_objs = hs->scene.getNumObjects();
  std::vector<float> v(9 * static_cast<size_t>(n_objs));
  std::vector<uint32_t> kind(n_objs);
  for (int j = 0; j < n_objs; ++j) {
    float normal[3];
    hs->scene.getObject(j)->pack(&v[9 * static_cast<size_t>(j)], normal);
    kind[j] = static_cast<uint32_t>(hs->scene.getObject(j)->kind());
  }
  for (uint32_t i = 0; i < n; ++i) {
    const float* p = points + 3 * static_cast<size_t>(i);
    float best, best_q[3] = {0.0f, 0.0f, 0.0f};
    int32_t best_object = -1;
    if (nearest_radius(max_dist != nullptr, max_dist ? max_dist[i] : 0.0f, best)) {
      for (int j = 0; j < n_objs; ++j) {
        float q[3];
        const float d2 = nearest_point(kind[j], &v[9 * static_cast<size_t>(j)], p, q);
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

}  // extern "C"

namespace {

// Where a host form's queries get their filters from (filter_rule.hpp): the skip arrays of a *_filtered call, or nothing
struct HostFilters {
  const int32_t* skip;
  uint32_t n_skip;
  const int32_t* skip_range;
  p3d::QueryFilter load(uint32_t i, uint32_t n_objs) const { return p3d::filter_load(n_skip ? skip : nullptr, n_skip, skip_range, i, n_objs); }
};
struct NoHostFilters {
  p3d::NoFilter load(uint32_t, uint32_t) const { return p3d::NoFilter{}; }
};
// What the filtered host forms refuse of their filter
int check_host_filter(const HostFilters& f, uint32_t n, const std::string& pre) {
  if (f.n_skip > P3D_FILTER_SKIP_MAX) return p3d::fail(P3D_ERR_INVALID, pre + "n_skip must be 0 .. P3D_FILTER_SKIP_MAX (8)");
  if (n && f.n_skip > 0 && !f.skip) return p3d::fail(P3D_ERR_INVALID, pre + "null skip with n > 0 and n_skip > 0");
  return P3D_OK;
}

// The statement of the k-nearest query: nearest_rule.hpp on every object the query's filter does not name, the k smallest
// (d2, object index) under the limit in that order.  q is not kept in the list: the rule is run once more on each listed
// object, which gives the same bits
template <class Filters>
int host_nearest_k(const std::string& pre, p3d_host_scene* hs, uint32_t n, uint32_t k, const float* points, const float* max_dist,
                   const Filters& filters, int32_t* count, int32_t* object, float* dist, float* closest) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, pre + "null scene");
  if (k == 0 || k > P3D_NEAREST_K_MAX) return p3d::fail(P3D_ERR_INVALID, pre + "k must be 1 .. P3D_NEAREST_K_MAX (16)");
  if (n && (!points || !count || !object)) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  using namespace p3d;
  const int n_objs = hs->scene.getNumObjects();
  std::vector<float> v(9 * static_cast<size_t>(n_objs));
  std::vector<uint32_t> kind(n_objs);
  for (int j = 0; j < n_objs; ++j) {
    float normal[3];
    hs->scene.getObject(j)->pack(&v[9 * static_cast<size_t>(j)], normal);
    kind[j] = static_cast<uint32_t>(hs->scene.getObject(j)->kind());
  }
  for (uint32_t i = 0; i < n; ++i) {
    const float* p = points + 3 * static_cast<size_t>(i);
    HostNearestList list;
    NearestKGate gate;
    uint32_t found = 0;
    const auto filter = filters.load(i, static_cast<uint32_t>(n_objs));
    if (nearest_k_open(max_dist != nullptr, max_dist ? max_dist[i] : 0.0f, gate)) {
      for (int j = 0; j < n_objs; ++j) {
        if (filter_skips(filter, j)) continue;
        float q[3];
        const float d2 = nearest_point(kind[j], &v[9 * static_cast<size_t>(j)], p, q);
        if (nearest_k_admits(d2, j, gate)) nearest_k_insert(list, found, k, gate, d2, j, static_cast<uint32_t>(j));
      }
    }
    count[i] = static_cast<int32_t>(found);
    for (uint32_t e = 0; e < k; ++e) {
      const size_t row = static_cast<size_t>(i) * k + e;
      float q[3] = {0.0f, 0.0f, 0.0f};
      const int32_t j = e < found ? list.object(e) : -1;
      if (j >= 0) nearest_point(kind[j], &v[9 * static_cast<size_t>(j)], p, q);
      object[row] = j;
      if (dist) dist[row] = j >= 0 ? sqrtf(list.d2(e)) : FLT_MAX;
      if (closest)
        for (int c = 0; c < 3; ++c) closest[3 * row + c] = q[c];
    }
  }
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
  const int n_objs = hs->scene.getNumObjects();
  std::vector<float> v(9 * static_cast<size_t>(n_objs));
  std::vector<uint32_t> kind(n_objs);
  for (int j = 0; j < n_objs; ++j) {
    float normal[3];
    hs->scene.getObject(j)->pack(&v[9 * static_cast<size_t>(j)], normal);
    kind[j] = static_cast<uint32_t>(hs->scene.getObject(j)->kind());
    if (kind[j] == P3D_PRIM_BOX)
      return p3d::fail(P3D_ERR_UNSUPPORTED, pre + "object " + std::to_string(j) + " is a box: a ball against a box (a rounded box, and its inside) is not swept");
  }
  if (n && (!origin || !direction || !radius || !object)) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  for (uint32_t i = 0; i < n; ++i) {
    const size_t row = 3 * static_cast<size_t>(i);
    SweepRay s;
    sweep_ray(origin + row, direction + row, radius[i], t_max != nullptr, t_max ? t_max[i] : 0.0f, s);
    float best = s.limit;
    int32_t best_object = kSweepNoObject;
    const auto filter = filters.load(i, static_cast<uint32_t>(n_objs));
    if (s.ok) {
      for (int j = 0; j < n_objs; ++j) {
        if (filter_skips(filter, j)) continue;
        float T;
        if (sweep_contact(kind[j], &v[9 * static_cast<size_t>(j)], s, T) && sweep_wins(T, j, best, best_object)) {
          best = T; best_object = j;
        }
      }
    }
    const bool found = best_object != kSweepNoObject;
    float c[3] = {0.0f, 0.0f, 0.0f}, q[3] = {0.0f, 0.0f, 0.0f};
    if (found) {
      sweep_centre(s, best, c);
      nearest_point(kind[best_object], &v[9 * static_cast<size_t>(best_object)], c, q);
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

// The statement of the nearest-surfaces-to-a-segment query: nearest_segment_rule.hpp on every object the segment's filter does
// not name, in object order; the k smallest (d2, object index) under the limit in that order.  s, x and q are not kept in the
// list: the rule is run once more on each listed object, which gives the same bits
template <class Filters>
int host_nearest_segment_k(const std::string& pre, p3d_host_scene* hs, uint32_t n, uint32_t k, const float* a, const float* b,
                           const float* max_dist, const Filters& filters, int32_t* count, int32_t* object, float* dist, float* param,
                           float* on_segment, float* closest) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, pre + "null scene");
  using namespace p3d;
  const int n_objs = hs->scene.getNumObjects();
  std::vector<float> v(9 * static_cast<size_t>(n_objs));
  std::vector<uint32_t> kind(n_objs);
  for (int j = 0; j < n_objs; ++j) {
    float normal[3];
    hs->scene.getObject(j)->pack(&v[9 * static_cast<size_t>(j)], normal);
    kind[j] = static_cast<uint32_t>(hs->scene.getObject(j)->kind());
    if (kind[j] == P3D_PRIM_BOX)
      return p3d::fail(P3D_ERR_UNSUPPORTED, pre + "object " + std::to_string(j) + " is a box: a segment against a box's faces is not part of this query");
  }
  if (k == 0 || k > P3D_NEAREST_K_MAX) return p3d::fail(P3D_ERR_INVALID, pre + "k must be 1 .. P3D_NEAREST_K_MAX (16)");
  if (n && (!a || !b || !count || !object)) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  for (uint32_t i = 0; i < n; ++i) {
    const float* pa = a + 3 * static_cast<size_t>(i);
    const float* pb = b + 3 * static_cast<size_t>(i);
    HostNearestList list;
    NearestKGate gate;
    uint32_t found = 0;
    const auto filter = filters.load(i, static_cast<uint32_t>(n_objs));
    if (nearest_k_open(max_dist != nullptr, max_dist ? max_dist[i] : 0.0f, gate)) {
      for (int j = 0; j < n_objs; ++j) {
        if (filter_skips(filter, j)) continue;
        float s, x[3], q[3];
        const float d2 = segment_nearest(kind[j], &v[9 * static_cast<size_t>(j)], pa, pb, s, x, q);
        if (nearest_k_admits(d2, j, gate)) nearest_k_insert(list, found, k, gate, d2, j, static_cast<uint32_t>(j));
      }
    }
    count[i] = static_cast<int32_t>(found);
    for (uint32_t e = 0; e < k; ++e) {
      const size_t row = static_cast<size_t>(i) * k + e;
      float s = FLT_MAX, x[3] = {0.0f, 0.0f, 0.0f}, q[3] = {0.0f, 0.0f, 0.0f};
      const int32_t j = e < found ? list.object(e) : -1;
      if (j >= 0) segment_nearest(kind[j], &v[9 * static_cast<size_t>(j)], pa, pb, s, x, q);
      object[row] = j;
      if (dist) dist[row] = j >= 0 ? sqrtf(list.d2(e)) : FLT_MAX;
      if (param) param[row] = s;
      for (int c = 0; c < 3; ++c) {
        if (on_segment) on_segment[3 * row + c] = x[c];
        if (closest) closest[3 * row + c] = q[c];
      }
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
  if (k > P3D_NEAREST_K_MAX) return p3d::fail(P3D_ERR_INVALID, pre + "k must be 0 .. P3D_NEAREST_K_MAX (16)");
  if (flags & ~P3D_OVERLAP_SOLID) return p3d::fail(P3D_ERR_INVALID, pre + "unknown flag (P3D_OVERLAP_SOLID is the only one)");
  if (n && (!lo || !hi || !total || (k > 0 && !object))) return p3d::fail(P3D_ERR_INVALID, pre + "null array with n > 0");
  using namespace p3d;
  const int n_objs = hs->scene.getNumObjects();
  std::vector<float> v(9 * static_cast<size_t>(n_objs));
  std::vector<uint32_t> kind(n_objs);
  for (int j = 0; j < n_objs; ++j) {
    float normal[3];
    hs->scene.getObject(j)->pack(&v[9 * static_cast<size_t>(j)], normal);
    kind[j] = static_cast<uint32_t>(hs->scene.getObject(j)->kind());
  }
  for (uint32_t i = 0; i < n; ++i) {
    const float* qlo = lo + 3 * static_cast<size_t>(i);
    const float* qhi = hi + 3 * static_cast<size_t>(i);
    int32_t* row = k ? object + static_cast<size_t>(i) * k : nullptr;
    uint32_t found = 0;
    const auto filter = filters.load(i, static_cast<uint32_t>(n_objs));
    if (overlap_query_open(qlo, qhi)) {
      for (int j = 0; j < n_objs; ++j) {
        if (filter_skips(filter, j)) continue;
        if (!overlap_box(kind[j], &v[9 * static_cast<size_t>(j)], qlo, qhi, flags)) continue;
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

int p3d_host_scene_overlap_box(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* lo, const float* hi, const int32_t* skip,
                               uint32_t n_skip, const int32_t* skip_range, uint32_t flags, int32_t* total, int32_t* object) {
  const std::string pre = "p3d_host_scene_overlap_box: ";
  const HostFilters filters{skip, n_skip, skip_range};
  if (int rc = check_host_filter(filters, n, pre)) return rc;
  if (n_skip == 0 && !skip_range) return host_overlap_box(pre, hs, n, k, lo, hi, NoHostFilters{}, flags, total, object);
  return host_overlap_box(pre, hs, n, k, lo, hi, filters, flags, total, object);
}

int p3d_host_scene_nearest_segment_k(p3d_host_scene* hs, uint32_t n, uint32_t k, const float* a, const float* b, const float* max_dist,
                                     const int32_t* skip, uint32_t n_skip, const int32_t* skip_range, int32_t* count, int32_t* object,
                                     float* dist, float* param, float* on_segment, float* closest) {
  const std::string pre = "p3d_host_scene_nearest_segment_k: ";
  const HostFilters filters{skip, n_skip, skip_range};
  if (int rc = check_host_filter(filters, n, pre)) return rc;
  if (n_skip == 0 && !skip_range)
    return host_nearest_segment_k(pre, hs, n, k, a, b, max_dist, NoHostFilters{}, count, object, dist, param, on_segment, closest);
  return host_nearest_segment_k(pre, hs, n, k, a, b, max_dist, filters, count, object, dist, param, on_segment, closest);
}

// The key of a BVH node under the segment query, for the tests (host only)
int p3d_debug_segment_box_d2(uint32_t n, const float* a, const float* b, const float* lo, const float* hi, float* out) {
  if (n && (!a || !b || !lo || !hi || !out)) return p3d::fail(P3D_ERR_INVALID, "p3d_debug_segment_box_d2: null array with n > 0");
  for (size_t i = 0; i < n; ++i) out[i] = p3d::segment_box_d2(a + 3 * i, b + 3 * i, lo + 3 * i, hi + 3 * i);
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
  const HostFilters filters{skip, n_skip, skip_range};
  if (int rc = check_host_filter(filters, n, pre)) return rc;
  return host_nearest_k(pre, hs, n, k, points, max_dist, filters, count, object, dist, closest);
}
int p3d_host_scene_sweep_sphere(const p3d_host_scene* hs, uint32_t n, const float* origin, const float* direction, const float* radius,
                                const float* t_max, int32_t* object, float* t, float* centre, float* contact) {
  return host_sweep_sphere("p3d_host_scene_sweep_sphere: ", hs, n, origin, direction, radius, t_max, NoHostFilters{}, object, t, centre, contact);
}
int p3d_host_scene_sweep_sphere_filtered(const p3d_host_scene* hs, uint32_t n, const float* origin, const float* direction,
                                         const float* radius, const float* t_max, const int32_t* skip, uint32_t n_skip,
                                         const int32_t* skip_range, int32_t* object, float* t, float* centre, float* contact) {
  const std::string pre = "p3d_host_scene_sweep_sphere_filtered: ";
  const HostFilters filters{skip, n_skip, skip_range};
  if (int rc = check_host_filter(filters, n, pre)) return rc;
  return host_sweep_sphere(pre, hs, n, origin, direction, radius, t_max, filters, object, t, centre, contact);
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

int p3d_host_scene_bind_device(p3d_host_scene* hs, p3d_scene* scene) {
  if (!hs) return p3d::fail(P3D_ERR_INVALID, "p3d_host_scene_bind_device: null argument");
  if (hs->bvh) hs->bvh->bindDevice(scene);
  if (hs->grid) hs->grid->bindDevice(scene);
  return hs->scene.bindDevice(scene) ? P3D_OK : P3D_ERR_NO_DEVICE;
}

}  // extern "C"

namespace p3d {
HostClasses host_classes(::p3d_host_scene* hs) { return HostClasses{&hs->scene, hs->bvh.get(), hs->grid.get()}; }
}  // namespace p3d
