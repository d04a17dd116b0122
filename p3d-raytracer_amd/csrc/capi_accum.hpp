// capi_accum.hpp — p3d_accum (include/p3d.h)
#pragma once
#include "capi_frame.hpp"

// Progressive accumulation (include/p3d.h): a frame's samples in passes, its running sums kept on the device between them.
struct p3d_accum {
  p3d_scene* s = nullptr;
  int device = 0;       // (destroy needs no scene)
  p3d_config cfg{};
  p3d_tile tile{};
  uint32_t total = 0;   // SPP^2
  uint32_t done = 0;    // samples [0, done) of every pixel are in the sums
  bool failed = false;  // a pass returned an error: the sums are unknown until p3d_accum_reset
  uint64_t cam_gen = 0; // the scene's camera generation at create / reset
  uint64_t geom_gen = 0; // ... and its geometry generation (p3d_scene_update_prims)
  Scratch sum, hit;     // [3 * pixel] float running sums, [pixel] first hits
};

extern "C" {

int p3d_accum_create(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, p3d_accum** out) {
  if (!s || !cfg || !tile || !out) return fail(P3D_ERR_INVALID, "p3d_accum_create: null argument");
  *out = nullptr;
  if (!cfg->antialiasing)
    return fail(P3D_ERR_UNSUPPORTED, "p3d_accum_create: antialiasing = 0 renders one sample per pixel; there is nothing to accumulate");
  if (cfg->integrator == P3D_WHITTED && cfg->accel == P3D_ACCEL_BVH && cfg->stack_mode == P3D_STACK_LITERAL)
    return fail(P3D_ERR_UNSUPPORTED, "p3d_accum_create: Whitted over the BVH with P3D_STACK_LITERAL hands the hit_stack from a pixel's last "
                                     "sample to the next pixel's first, so no split over samples keeps the reference's order; use P3D_STACK_PER_PIXEL");
  if (int rc = check_frame(s, cfg, tile)) return rc;
  P3D_HIP(hipSetDevice(s->device));
  p3d_accum* a = new p3d_accum;
  a->s = s;
  a->device = s->device;
  a->cfg = *cfg;
  a->tile = *tile;
  a->total = cfg->spp_sqrt * cfg->spp_sqrt;
  restart_passes(a);
  const size_t n = (size_t)tile->w * tile->h;
  int rc = a->sum.ensure(n * 3 * sizeof(float));
  if (!rc) rc = a->hit.ensure(n * sizeof(int32_t));
  if (rc) {
    p3d_accum_destroy(a);
    return rc;
  }
  *out = a;
  return P3D_OK;
}

void p3d_accum_destroy(p3d_accum* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  delete a;
}

int p3d_accum_reset(p3d_accum* a) {
  if (!a) return fail(P3D_ERR_INVALID, "p3d_accum_reset: null accumulator");
  restart_passes(a);
  return P3D_OK;
}

uint32_t p3d_accum_samples_done(const p3d_accum* a) { return a ? a->done : 0u; }

int p3d_accum_render_device(p3d_accum* a, uint32_t n, float* d_rgb, int32_t* d_hit, uint8_t* d_rgb8, void* hip_stream, p3d_stats* stats) {
  if (!a) return fail(P3D_ERR_INVALID, "p3d_accum_render_device: null accumulator");
  if (int rc = check_pass(a, n, "p3d_accum")) return rc;
  const int rc = render_frame(a->s, &a->cfg, &a->tile, d_rgb, d_hit, d_rgb8, hip_stream, stats, a->done, a->done + n,
                             (float*)a->sum.p, (int32_t*)a->hit.p);
  if (rc) {
    a->failed = true;
    return rc;
  }
  a->done += n;
  return P3D_OK;
}

int p3d_accum_render(p3d_accum* a, uint32_t n, float* rgb, int32_t* hit_id, uint8_t* rgb8, p3d_stats* stats) {
  if (!a) return fail(P3D_ERR_INVALID, "p3d_accum_render: null accumulator");
  return render_to_host(a->s, (size_t)a->tile.w * a->tile.h, rgb, hit_id, rgb8, stats, [&](float* d_rgb, int32_t* d_hit, uint8_t* d_rgb8, p3d_stats* st) {
    return p3d_accum_render_device(a, n, d_rgb, d_hit, d_rgb8, nullptr, st);
  });
}

}  // extern "C"
