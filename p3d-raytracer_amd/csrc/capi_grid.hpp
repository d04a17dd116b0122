// capi_grid.hpp — the uniform grid of a live scene, built on the device (grid_build.hpp): p3d_scene_build_grid, the rebuild
// inside p3d_scene_update_prims, and p3d_scene_export_grid
#pragma once
#include "capi_common.hpp"

namespace {

// The builder's state of a scene of p3d_scene_create_device_bvh, with the object boxes the tree in d_blob was built from:
// allocated by the first update or the first grid build, whichever comes first.  The device is current and idle.
int ensure_box_workspace(p3d_scene* s, const char* who) {
  lbvh::Workspace& w = s->lbvh_ws;
  if (w.n) return P3D_OK;
  hipError_t e = w.alloc(s->dev.n_objs, true);
  if (e == hipSuccess) e = hipMemcpy(w.boxes, s->create_boxes.data(), s->create_boxes.size() * sizeof(float4), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    w.release();
    return fail(P3D_ERR_NO_DEVICE, std::string(who) + ": workspace: " + hipGetErrorString(e));
  }
  std::vector<float4>().swap(s->create_boxes);
  s->lbvh_topology = false;
  return P3D_OK;
}

// Builds the grid over lbvh_ws.boxes into the scene's cell arrays, on the null stream, and waits for it.  The device is idle
// and no frame is enqueued.  On any failure the scene is left WITHOUT a grid (has_grid = false); the arrays it owns stay
// allocated for a later build.
int rebuild_grid(p3d_scene* s, const char* who) {
  const std::string pre = std::string(who) + ": grid: ";
  s->has_grid = false;
  auto hip_fail = [&](const char* what, hipError_t e) {
    // an allocation that does not fit is the scene's size, not the device's fault
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? P3D_ERR_CAPACITY : P3D_ERR_NO_DEVICE, pre + what + ": " + hipGetErrorString(e));
  };
  grid_build::Workspace& w = s->grid_ws;
  if (!w.n) {
    if (hipError_t e = w.alloc(s->dev.n_objs); e != hipSuccess) {
      w.release();
      return hip_fail("workspace", e);
    }
  }
  float lo[3], hi[3];
  if (hipError_t e = grid_build::box_union(w, s->lbvh_ws.boxes, lo, hi); e != hipSuccess) return hip_fail("bounds", e);
  // Grid::Build scans with strict < and >, which keeps the first of two equal values: against a plain min / max that can
  // only differ in the sign of a zero, and -0 - 1e-4 == +0 - 1e-4 (as for the sum): the difference ends here.
  grid_build::Dims d;
  uint64_t n_cells = 1;
  for (int k = 0; k < 3; ++k) {
    d.p0[k] = lo[k] - kGridEps;
    d.p1[k] = hi[k] + kGridEps;
    const float cells = grid_axis_cells(kGridDensity, d.p1[k] - d.p0[k], 1.0f);
    if (!(cells >= 1.0f) || !(cells < 2147483648.0f))
      return fail(P3D_ERR_CAPACITY, pre + "the cell count of an axis does not fit an int");
    d.n[k] = static_cast<int>(cells);
    if (n_cells <= grid_build::kMaxCells) n_cells *= (uint64_t)d.n[k];  // (< 2^28 * 2^31: no overflow)
  }
  if (n_cells > grid_build::kMaxCells)
    return fail(P3D_ERR_CAPACITY, pre + std::to_string(d.n[0]) + " x " + std::to_string(d.n[1]) + " x " + std::to_string(d.n[2]) + " cells are more than 2^28");
  uint64_t total = 0;
  if (hipError_t e = grid_build::count_pairs(w, s->lbvh_ws.boxes, d, &total); e != hipSuccess) return hip_fail("count", e);
  if (total > 0xffffffffull) return fail(P3D_ERR_CAPACITY, pre + std::to_string(total) + " cell items do not fit uint32");
  if (hipError_t e = w.ensure_pairs(total); e != hipSuccess) return hip_fail("pair arrays", e);
  auto grow = [&](uint32_t*& p, uint64_t& cap, uint64_t need) {
    if (need <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc((void**)&p, (size_t)need * sizeof(uint32_t));
    if (e == hipSuccess) cap = need;
    return e;
  };
  if (hipError_t e = grow(s->d_cell_start, s->cell_start_cap, n_cells + 1); e != hipSuccess) return hip_fail("cell_start", e);
  if (hipError_t e = grow(s->d_cell_items, s->cell_items_cap, std::max<uint64_t>(total, 1)); e != hipSuccess) return hip_fail("cell_items", e);
  hipError_t e = grid_build::enqueue_cells(w, d, (uint32_t)n_cells, (uint32_t)total, s->d_cell_start, s->d_cell_items);
  if (e == hipSuccess) e = hipStreamSynchronize(0);
  if (e != hipSuccess) return hip_fail("build", e);
  DevGrid& g = s->dev.grid;
  g.bmin = to_f3(d.p0); g.bmax = to_f3(d.p1);
  g.nx = d.n[0]; g.ny = d.n[1]; g.nz = d.n[2];
  g.cell_start = s->d_cell_start; g.cell_items = s->d_cell_items;
  s->grid_items = (uint32_t)total;
  s->has_grid = true;
  return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_scene_build_grid(p3d_scene* s, float* build_ms) {
  if (!s) return fail(P3D_ERR_INVALID, "p3d_scene_build_grid: null scene");
  if (!s->device_bvh)
    return fail(P3D_ERR_INVALID, "p3d_scene_build_grid: the scene was not created by p3d_scene_create_device_bvh (only those keep their objects' boxes on the device)");
  if (s->uploaded_grid) return fail(P3D_ERR_INVALID, "p3d_scene_build_grid: the scene was created with the host's grid");
  if (s->dev.n_objs == 0) return fail(P3D_ERR_UNSUPPORTED, "p3d_scene_build_grid: the scene has no objects");
  if (s->dev.odd_boxes) return fail(P3D_ERR_UNSUPPORTED, "p3d_scene_build_grid: the scene was created with a non-finite or inverted box");
  if (build_ms) *build_ms = 0.0f;
  P3D_HIP(hipSetDevice(s->device));
  // enqueued frames may read the grid that is about to be replaced: the tail stream, then the whole device
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  if (int rc = ensure_box_workspace(s, "p3d_scene_build_grid")) return rc;
  // a grid frame's tile costs and hand-off memos were recorded for the grid that goes away
  drop_schedules(s);
  s->ho_chain_key.clear();
  P3D_HIP(hipEventRecord(s->ev0, 0));
  if (int rc = rebuild_grid(s, "p3d_scene_build_grid")) return rc;
  P3D_HIP(hipEventRecord(s->ev1, 0));
  P3D_HIP(hipEventSynchronize(s->ev1));
  float ms = 0.0f;
  P3D_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
  if (build_ms) *build_ms = ms;
  return P3D_OK;
}

int p3d_scene_export_grid(p3d_scene* s, p3d_grid_desc* info, uint32_t* cell_start, uint32_t* n_cell_start, uint32_t* cell_items, uint32_t* n_cell_items) {
  if (!s) return fail(P3D_ERR_INVALID, "p3d_scene_export_grid: null scene");
  if (!info || !n_cell_start || !n_cell_items) return fail(P3D_ERR_INVALID, "p3d_scene_export_grid: null info or size argument");
  if (cell_start && !cell_items) return fail(P3D_ERR_INVALID, "p3d_scene_export_grid: cell_start without cell_items");
  if (!s->has_grid || s->uploaded_grid) return fail(P3D_ERR_INVALID, "p3d_scene_export_grid: the scene has no device-built grid (p3d_scene_build_grid)");
  const DevGrid& g = s->dev.grid;
  const uint32_t n_cells = (uint32_t)((uint64_t)g.nx * g.ny * g.nz), n_items = s->grid_items;
  *info = p3d_grid_desc{};
  info->bmin[0] = g.bmin.x; info->bmin[1] = g.bmin.y; info->bmin[2] = g.bmin.z;
  info->bmax[0] = g.bmax.x; info->bmax[1] = g.bmax.y; info->bmax[2] = g.bmax.z;
  info->nx = g.nx; info->ny = g.ny; info->nz = g.nz;
  info->n_cells = n_cells;
  info->n_items = n_items;
  const uint32_t have_start = *n_cell_start, have_items = *n_cell_items;
  *n_cell_start = n_cells + 1;
  *n_cell_items = n_items;
  if (!cell_start) return P3D_OK;
  if (have_start < n_cells + 1 || have_items < n_items)
    return fail(P3D_ERR_CAPACITY, "p3d_scene_export_grid: the arrays are too small (call with cell_start = NULL for the sizes)");
  P3D_HIP(hipSetDevice(s->device));
  if (int rc = p3d_scene_join(s, nullptr, 1)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  P3D_HIP(hipMemcpy(cell_start, s->d_cell_start, ((size_t)n_cells + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (n_items) P3D_HIP(hipMemcpy(cell_items, s->d_cell_items, (size_t)n_items * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return P3D_OK;
}

}  // extern "C"
