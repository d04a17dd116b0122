// capi_scene.hpp — scene create / destroy / skybox: the device half (the host-only half is capi_scene_layout.hpp)
#pragma once
#include "capi_scene_layout.hpp"

extern "C" {

int p3d_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  return n;
}

void p3d_scene_destroy(p3d_scene* s) {
  if (!s) return;
  (void)hipSetDevice(s->device);
  for (void* p : {(void*)s->d_blob, (void*)s->d_cell_start, (void*)s->d_cell_items, (void*)s->d_emitters, (void*)s->d_stats, (void*)s->d_status, (void*)s->d_refit_skipped,
                  (void*)s->d_halo_verdict, (void*)s->d_sky[0], (void*)s->d_sky[1], (void*)s->d_sky[2], (void*)s->d_sky[3], (void*)s->d_sky[4], (void*)s->d_sky[5]})
    if (p) (void)hipFree(p);
  drop_schedules(s);
  s->lbvh_ws.release();
  s->grid_ws.release();
  for (hipEvent_t e : {s->ev0, s->ev1, s->ev_mid, s->ev_p1, s->ev_tail_go, s->ev_tail_done})
    if (e) (void)hipEventDestroy(e);
  delete s;  // (every Scratch of the scene frees itself here)
}

}  // extern "C"

namespace {

// The linear BVH of p3d_scene_create_device_bvh, built over the uploaded object-order geometry (lbvh.hpp)
int build_device_bvh(p3d_scene* s, const p3d_scene_desc* d) {
  DevScene& v = s->dev;
  if (d->n_prims > 0x07ffffffu) return fail(P3D_ERR_CAPACITY, "p3d_scene_create_device_bvh: too many objects");
  std::vector<float4> boxes((size_t)2 * d->n_prims);
  for (uint32_t i = 0; i < d->n_prims; ++i)
    for (int k = 0; k < 3; ++k)
      if (!(std::fabs(d->prims[i].bmin[k]) < INFINITY) || !(std::fabs(d->prims[i].bmax[k]) < INFINITY) || !(d->prims[i].bmin[k] <= d->prims[i].bmax[k]))
        v.odd_boxes = 1u;  // (the built tree's boxes are unions of these)
  for (uint32_t i = 0; i < d->n_prims; ++i) {
    boxes[2 * i] = make_float4(d->prims[i].bmin[0], d->prims[i].bmin[1], d->prims[i].bmin[2], 0.f);
    boxes[2 * i + 1] = make_float4(d->prims[i].bmax[0], d->prims[i].bmax[1], d->prims[i].bmax[2], 0.f);
  }
  float4* d_boxes = nullptr;
  P3D_HIP(hipMalloc((void**)&d_boxes, boxes.size() * sizeof(float4)));
  hipError_t e = hipMemcpy(d_boxes, boxes.data(), boxes.size() * sizeof(float4), hipMemcpyHostToDevice);
  lbvh::Result built;
  if (e == hipSuccess)
    e = lbvh::build(d_boxes, s->d_blob + s->off_ogeom, d->n_prims, s->d_blob + s->off_nodes, s->d_blob + s->off_bgeom, &built);
  (void)hipFree(d_boxes);
  if (e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("device BVH build: ") + hipGetErrorString(e));
  v.n_nodes = built.n_nodes;
  v.n_slots = d->n_prims;
  s->has_bvh = true;
  s->bvh_max_depth = built.max_depth;
  s->device_bvh_ms = built.build_ms;
  s->create_boxes = std::move(boxes);
  return P3D_OK;
}

int upload_grid(p3d_scene* s, const p3d_grid_desc& g) {
  DevScene& v = s->dev;
  P3D_HIP(hipMalloc((void**)&s->d_cell_start, (size_t)(g.n_cells + 1) * 4));
  P3D_HIP(hipMemcpy(s->d_cell_start, g.cell_start, (size_t)(g.n_cells + 1) * 4, hipMemcpyHostToDevice));
  P3D_HIP(hipMalloc((void**)&s->d_cell_items, (size_t)std::max<uint32_t>(g.n_items, 1) * 4));
  if (g.n_items) P3D_HIP(hipMemcpy(s->d_cell_items, g.cell_items, (size_t)g.n_items * 4, hipMemcpyHostToDevice));
  v.grid.bmin = to_f3(g.bmin); v.grid.bmax = to_f3(g.bmax);
  v.grid.nx = g.nx; v.grid.ny = g.ny; v.grid.nz = g.nz;
  v.grid.cell_start = s->d_cell_start; v.grid.cell_items = s->d_cell_items;
  s->has_grid = s->uploaded_grid = true;
  return P3D_OK;
}

// Validate (host only), set device, lay out (host only; after the device so that its one refusal keeps its place), upload,
// optional device build, grid, small allocations, events.
// device_bvh: the BVH arrays of the descriptor are ignored and a linear BVH is built on the GPU (lbvh.hpp)
int create_impl(const p3d_scene_desc* d_in, int device, bool device_bvh, p3d_scene** out) {
  if (!d_in || !out) return fail(P3D_ERR_INVALID, "p3d_scene_create: null argument");
  p3d_scene_desc d_local = *d_in;
  if (device_bvh) {  // sizes of the device-built tree: 2 n - 1 nodes, one leaf slot per object
    d_local.n_bvh_nodes = 0; d_local.bvh_nodes = nullptr;
    d_local.n_bvh_prim_index = 0; d_local.bvh_prim_index = nullptr;
    d_local.bvh_max_depth = 0;
  }
  const p3d_scene_desc* d = &d_local;
  if (int rc = validate_scene_desc(d)) return rc;
  int ndev = 0;
  P3D_HIP(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(P3D_ERR_NO_DEVICE, "p3d_scene_create: no such HIP device");
  P3D_HIP(hipSetDevice(device));

  SceneLayout L;
  if (int rc = layout_bvh(d, L)) return rc;
  assemble_blob(d, device_bvh && d->n_prims ? 2 * d->n_prims - 1 : 0, device_bvh ? d->n_prims : 0, L);
  // every early return below frees what was allocated so far (device memory, events)
  auto s = std::unique_ptr<p3d_scene, void (*)(p3d_scene*)>(new p3d_scene(), &p3d_scene_destroy);
  s->device = device;
  s->off_nodes = L.off_nodes; s->off_bgeom = L.off_bgeom; s->off_ogeom = L.off_ogeom;
  s->off_normals = L.off_normals; s->off_mats = L.off_mats; s->off_lights = L.off_lights;
  s->blob_f4 = (uint32_t)L.blob.size();
  P3D_HIP(hipMalloc((void**)&s->d_blob, L.blob.size() * sizeof(float4)));
  P3D_HIP(hipMemcpy(s->d_blob, L.blob.data(), L.blob.size() * sizeof(float4), hipMemcpyHostToDevice));
  if (!L.emitters.empty()) {
    P3D_HIP(hipMalloc((void**)&s->d_emitters, L.emitters.size() * 4));
    P3D_HIP(hipMemcpy(s->d_emitters, L.emitters.data(), L.emitters.size() * 4, hipMemcpyHostToDevice));
    s->emitters_cap = (uint32_t)L.emitters.size();
  }
  s->obj_tm.resize(d->n_prims);
  for (uint32_t i = 0; i < d->n_prims; ++i) s->obj_tm[i] = d->prims[i].type | (d->prims[i].material << 8);
  DevScene& v = s->dev;
  v.nodes = s->d_blob + s->off_nodes;
  v.bgeom = s->d_blob + s->off_bgeom;
  v.ogeom = s->d_blob + s->off_ogeom;
  v.normals = s->d_blob + s->off_normals;
  v.mats = s->d_blob + s->off_mats;
  v.lights = s->d_blob + s->off_lights;
  v.emitters = s->d_emitters;
  v.n_nodes = L.n_nodes;
  v.odd_boxes = L.odd_boxes ? 1u : 0u;
  v.n_slots = d->n_bvh_prim_index;
  v.n_objs = d->n_prims;
  v.n_mats = d->n_materials;
  v.n_lights = d->n_lights;
  v.n_emitters = (uint32_t)L.emitters.size();
  v.cam = dev_camera(d->camera);
  v.bg = to_f3(d->background);
  s->has_bvh = d->n_bvh_nodes > 0;
  if (device_bvh && d->n_prims)
    if (int rc = build_device_bvh(s.get(), d)) return rc;
  s->device_bvh = device_bvh;
  if (!device_bvh) s->bvh_max_depth = std::max(d->bvh_max_depth, L.real_depth);
  if (s->has_bvh) {  // root box, from the node array as uploaded or built
    float4 root[2];
    P3D_HIP(hipMemcpy(root, s->d_blob + s->off_nodes, sizeof(root), hipMemcpyDeviceToHost));
    s->root_min[0] = root[0].x; s->root_min[1] = root[0].y; s->root_min[2] = root[0].z;
    s->root_max[0] = root[1].x; s->root_max[1] = root[1].y; s->root_max[2] = root[1].z;
  }
  if (d->has_grid)
    if (int rc = upload_grid(s.get(), d->grid)) return rc;
  P3D_HIP(hipMalloc((void**)&s->d_stats, kNumStats * sizeof(unsigned long long)));
  P3D_HIP(hipMalloc((void**)&s->d_status, sizeof(uint32_t)));
  P3D_HIP(hipMemset(s->d_status, 0, sizeof(uint32_t)));
  P3D_HIP(hipMalloc((void**)&s->d_halo_verdict, sizeof(uint32_t)));
  P3D_HIP(hipMemset(s->d_halo_verdict, 0, sizeof(uint32_t)));
  for (uint32_t i = 0; i < d->n_prims; ++i) s->has_spheres = s->has_spheres || d->prims[i].type == P3D_PRIM_SPHERE;
  for (uint32_t i = 0; i < d->n_prims; ++i) s->has_planes = s->has_planes || d->prims[i].type == P3D_PRIM_PLANE;
  for (uint32_t i = d->n_prims; i-- > 0;)
    if ((s->obj_tm[i] & 0xffu) == P3D_PRIM_BOX) s->first_box = i;
  for (uint32_t i = 0; i < d->n_materials; ++i)
    if (d->materials[i].transmittance != 0 && d->materials[i].reflection > 0) s->zero_weight_reflections = true;
  P3D_HIP(hipEventCreate(&s->ev0));
  P3D_HIP(hipEventCreate(&s->ev1));
  P3D_HIP(hipEventCreate(&s->ev_mid));
  P3D_HIP(hipEventCreate(&s->ev_p1));
  P3D_HIP(hipEventCreateWithFlags(&s->ev_tail_go, hipEventDisableTiming));
  P3D_HIP(hipEventCreateWithFlags(&s->ev_tail_done, hipEventDisableTiming));
  *out = s.release();
  return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_scene_create(const p3d_scene_desc* d, int device, p3d_scene** out) { return create_impl(d, device, false, out); }

int p3d_scene_create_device_bvh(const p3d_scene_desc* d, int device, p3d_scene** out, float* build_ms) {
  const int rc = create_impl(d, device, true, out);
  if (rc == P3D_OK && build_ms) *build_ms = (*out)->device_bvh_ms;
  return rc;
}

int p3d_scene_set_skybox(p3d_scene* s, const p3d_skybox_desc* sky) {
  if (!s || !sky) return fail(P3D_ERR_INVALID, "p3d_scene_set_skybox: null argument");
  for (int f = 0; f < 6; ++f) {
    const p3d_skybox_face& a = sky->face[f];
    if (!a.img || a.res_x == 0 || a.res_y == 0 || (a.bpp != 3 && a.bpp != 4) || (uint64_t)a.res_x * a.res_y > (1ull << 28))
      return fail(P3D_ERR_INVALID, "p3d_scene_set_skybox: bad face (need img, res > 0, bpp 3 or 4)");
  }
  P3D_HIP(hipSetDevice(s->device));
  for (int f = 0; f < 6; ++f) {
    const p3d_skybox_face& a = sky->face[f];
    const size_t n = (size_t)a.res_x * a.res_y;
    std::vector<uint32_t> rgba(n);  // one 4-byte texel fetch instead of three byte loads
    for (size_t i = 0; i < n; ++i)
      rgba[i] = (uint32_t)a.img[i * a.bpp] | ((uint32_t)a.img[i * a.bpp + 1] << 8) | ((uint32_t)a.img[i * a.bpp + 2] << 16);
    if (s->d_sky[f]) { (void)hipFree(s->d_sky[f]); s->d_sky[f] = nullptr; }
    P3D_HIP(hipMalloc((void**)&s->d_sky[f], n * 4));
    P3D_HIP(hipMemcpy(s->d_sky[f], rgba.data(), n * 4, hipMemcpyHostToDevice));
    s->dev.sky[f] = s->d_sky[f];
    s->dev.sky_w[f] = a.res_x;
    s->dev.sky_h[f] = a.res_y;
  }
  s->has_sky = true;
  return P3D_OK;
}

}  // extern "C"
