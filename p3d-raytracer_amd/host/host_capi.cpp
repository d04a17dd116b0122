// host_capi.cpp — the p3d_host_* half of include/p3d.h: .p3f -> Scene -> accel builds ->
// flat p3d_scene_desc.  Pure host code (no HIP).  The queries on a host scene are host_queries.cpp's.
#include <cstring>
#include <string>

#include "host_scene.hpp"
#include "p3d_error.hpp"

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
