// capi_adaptive.hpp — p3d_adaptive (include/p3d.h; kernels: adaptive.hpp)
#pragma once
#include "capi_frame.hpp"

// Adaptive sampling (include/p3d.h): a progressive path-traced frame whose pixels stop taking samples once converged.
// Per pixel: the running sum, first hit, S2 and sample count; the list of the pixels the next pass renders and its count
// live on the device (two counts: the pass reads one while its resolve builds the other).
struct p3d_adaptive {
  p3d_scene* s = nullptr;
  int device = 0;
  p3d_config cfg{};
  p3d_tile tile{};
  p3d_adaptive_params prm{};
  uint32_t total = 0;     // SPP^2
  uint32_t done = 0;      // samples of the passes so far
  uint32_t passes = 0;    // passes since the reset: the list's count is counters[passes & 1]
  uint32_t resident = 0;  // workgroups the device holds at once
  bool failed = false;
  uint64_t cam_gen = 0;   // the scene's camera generation at create / reset
  uint64_t geom_gen = 0;  // ... and its geometry generation (p3d_scene_update_prims)
  Scratch sum, hit, sum_y2, samples, active, rel_err, list, counters;  // counters: count[2], ticket
  Scratch var;  // p3d_denoise_variance (host form): the device copy of its output
};

namespace {

size_t adapt_pixels(const p3d_adaptive* a) { return (size_t)a->tile.w * a->tile.h; }

AdaptResolveParams adapt_resolve_params(p3d_adaptive* a, bool init) {
  AdaptResolveParams R{};
  uint32_t* ctr = (uint32_t*)a->counters.p;
  R.sum = (const float*)a->sum.p; R.hit = (const int32_t*)a->hit.p; R.sum_y2 = (const float*)a->sum_y2.p;
  R.samples = (uint32_t*)a->samples.p; R.active = (uint8_t*)a->active.p; R.rel_err = (float*)a->rel_err.p;
  R.list_out = (uint32_t*)a->list.p;
  R.count_out = ctr + ((a->passes + (init ? 0 : 1)) & 1u);
  R.count_done = ctr + ((a->passes + (init ? 1 : 0)) & 1u);
  R.ticket = ctr + 2;
  R.w = a->tile.w; R.h = a->tile.h;
  R.tiles8_x = ((uint32_t)a->tile.w + 7) / 8;
  R.slots = R.tiles8_x * (((uint32_t)a->tile.h + 7) / 8) * 64;
  R.min_samples = a->prm.min_samples; R.rel_error = a->prm.rel_error; R.gamma = a->cfg.gamma;
  R.init = init ? 1u : 0u;
  return R;
}

// Back to 0 samples with every pixel listed; returns when the device has done it
int adapt_start(p3d_adaptive* a) {
  P3D_HIP(hipSetDevice(a->device));
  P3D_HIP(hipDeviceSynchronize());  // (no pass of this frame may still run; the caller's streams need not block on the null stream)
  restart_passes(a);
  a->passes = 0;
  P3D_HIP(hipMemsetAsync(a->counters.p, 0, 4 * sizeof(uint32_t), nullptr));
  const AdaptResolveParams R = adapt_resolve_params(a, true);
  hipLaunchKernelGGL(adapt_resolve_kernel, dim3((R.slots + kAdaptResolveThreads - 1) / kAdaptResolveThreads), dim3(kAdaptResolveThreads), 0, nullptr, R);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("adaptive reset launch: ") + hipGetErrorString(e));
  P3D_HIP(hipDeviceSynchronize());
  return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_adaptive_create(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, const p3d_adaptive_params* prm, p3d_adaptive** out) {
  if (!s || !cfg || !tile || !prm || !out) return fail(P3D_ERR_INVALID, "p3d_adaptive_create: null argument");
  *out = nullptr;
  if (cfg->integrator != P3D_PATHTRACE)
    return fail(P3D_ERR_UNSUPPORTED, "p3d_adaptive_create: adaptive sampling is for the path tracer (Whitted frames have few, cheap samples per pixel)");
  if (!cfg->antialiasing)
    return fail(P3D_ERR_UNSUPPORTED, "p3d_adaptive_create: antialiasing = 0 renders one sample per pixel; there is nothing to adapt");
  if (int rc = check_frame(s, cfg, tile)) return rc;
  const uint32_t total = cfg->spp_sqrt * cfg->spp_sqrt;
  if (!(prm->rel_error >= 0.0f)) return fail(P3D_ERR_INVALID, "p3d_adaptive_create: rel_error must be a number >= 0");
  if (prm->min_samples < 2 || prm->min_samples > total)
    return fail(P3D_ERR_INVALID, "p3d_adaptive_create: min_samples must lie in [2, SPP*SPP = " + std::to_string(total) + "]");
  if (prm->reserved[0] || prm->reserved[1]) return fail(P3D_ERR_INVALID, "p3d_adaptive_create: reserved fields must be 0");
  P3D_HIP(hipSetDevice(s->device));
  int cus = 0;
  P3D_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device));
  p3d_adaptive* a = new p3d_adaptive;
  a->s = s;
  a->device = s->device;
  a->cfg = *cfg;
  a->tile = *tile;
  a->prm = *prm;
  a->total = total;
  a->resident = (uint32_t)std::max(cus, 1) * 4 * P3D_PT_WAVES;  // 4 SIMDs per CU
  const size_t n = adapt_pixels(a);
  int rc = a->sum.ensure(n * 3 * sizeof(float));
  if (!rc) rc = a->hit.ensure(n * sizeof(int32_t));
  if (!rc) rc = a->sum_y2.ensure(n * sizeof(float));
  if (!rc) rc = a->samples.ensure(n * sizeof(uint32_t));
  if (!rc) rc = a->active.ensure(n);
  if (!rc) rc = a->rel_err.ensure(n * sizeof(float));
  if (!rc) rc = a->list.ensure(n * sizeof(uint32_t));
  if (!rc) rc = a->counters.ensure(4 * sizeof(uint32_t));
  if (!rc) rc = adapt_start(a);
  if (rc) {
    p3d_adaptive_destroy(a);
    return rc;
  }
  *out = a;
  return P3D_OK;
}

void p3d_adaptive_destroy(p3d_adaptive* a) {
  if (!a) return;
  (void)hipSetDevice(a->device);
  delete a;
}

int p3d_adaptive_reset(p3d_adaptive* a) {
  if (!a) return fail(P3D_ERR_INVALID, "p3d_adaptive_reset: null object");
  return adapt_start(a);
}

uint32_t p3d_adaptive_samples_done(const p3d_adaptive* a) { return a ? a->done : 0u; }

int p3d_adaptive_active_pixels(p3d_adaptive* a, uint32_t* n) {
  if (!a || !n) return fail(P3D_ERR_INVALID, "p3d_adaptive_active_pixels: null argument");
  P3D_HIP(hipSetDevice(a->device));
  P3D_HIP(hipDeviceSynchronize());
  P3D_HIP(hipMemcpy(n, (uint32_t*)a->counters.p + (a->passes & 1u), sizeof(uint32_t), hipMemcpyDeviceToHost));
  return P3D_OK;
}

int p3d_adaptive_render_device(p3d_adaptive* a, uint32_t n, float* d_rgb, int32_t* d_hit, uint8_t* d_rgb8, uint32_t* d_samples,
                               void* hip_stream, p3d_stats* stats) {
  if (!a) return fail(P3D_ERR_INVALID, "p3d_adaptive_render_device: null object");
  if (int rc = check_pass(a, n, "p3d_adaptive")) return rc;
  AdaptPass ap{};
  uint32_t* ctr = (uint32_t*)a->counters.p;
  ap.k.list = (const uint32_t*)a->list.p;
  ap.k.count = ctr + (a->passes & 1u);
  ap.k.ticket = ctr + 2;
  ap.k.sum_y2 = (float*)a->sum_y2.p;
  ap.r = adapt_resolve_params(a, false);
  ap.r.n = n;
  ap.r.rgb = d_rgb; ap.r.hit_id = d_hit; ap.r.rgb8 = d_rgb8; ap.r.samples_out = d_samples;
  ap.resident = a->resident;
  const int rc = render_adaptive_pass(a->s, &a->cfg, &a->tile, hip_stream, stats, a->done, a->done + n, (float*)a->sum.p, (int32_t*)a->hit.p, ap);
  if (rc) {
    a->failed = true;
    return rc;
  }
  a->done += n;
  ++a->passes;
  return P3D_OK;
}

int p3d_adaptive_render(p3d_adaptive* a, uint32_t n, float* rgb, int32_t* hit_id, uint8_t* rgb8, uint32_t* samples, p3d_stats* stats) {
  if (!a) return fail(P3D_ERR_INVALID, "p3d_adaptive_render: null object");
  const size_t px = adapt_pixels(a);
  if (int rc = render_to_host(a->s, px, rgb, hit_id, rgb8, stats, [&](float* d_rgb, int32_t* d_hit, uint8_t* d_rgb8, p3d_stats* st) {
        return p3d_adaptive_render_device(a, n, d_rgb, d_hit, d_rgb8, nullptr, nullptr, st);
      }))
    return rc;
  if (samples) P3D_HIP(hipMemcpy(samples, a->samples.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return P3D_OK;
}

int p3d_adaptive_read_state(p3d_adaptive* a, float* sum, float* sum_y2, uint32_t* samples, float* rel_err) {
  if (!a) return fail(P3D_ERR_INVALID, "p3d_adaptive_read_state: null object");
  P3D_HIP(hipSetDevice(a->device));
  P3D_HIP(hipDeviceSynchronize());
  const size_t px = adapt_pixels(a);
  if (sum) P3D_HIP(hipMemcpy(sum, a->sum.p, px * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (sum_y2) P3D_HIP(hipMemcpy(sum_y2, a->sum_y2.p, px * sizeof(float), hipMemcpyDeviceToHost));
  if (samples) P3D_HIP(hipMemcpy(samples, a->samples.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (rel_err) P3D_HIP(hipMemcpy(rel_err, a->rel_err.p, px * sizeof(float), hipMemcpyDeviceToHost));
  return P3D_OK;
}

}  // extern "C"
