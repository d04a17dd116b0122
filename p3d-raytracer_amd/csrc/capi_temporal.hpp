// capi_temporal.hpp — p3d_temporal (include/p3d.h; kernels: temporal.hpp)
#pragma once
#include "capi_common.hpp"

// Per pixel three float4 images (colour + history, moments + coverage, normal_depth), twice: the frame of parity k writes set
// k & 1 and reads the other.  The previous frame's camera is kept here and handed to the kernel by value.
struct p3d_temporal {
  int device = 0;
  int32_t w = 0, h = 0;
  uint32_t frames = 0;  // frames since create / reset
  p3d_camera prev{};    // the camera of the last frame (frames > 0)
  Scratch col[2], mom[2], nd[2];
  Scratch h_rgb, h_nd, h_ac, h_out, h_var, h_hist;  // the host-buffer call's device copies
};

namespace {

int check_temporal_params(const p3d_temporal_params* prm) {
  if (!(prm->alpha >= 0.0f && prm->alpha <= 1.0f) || !(prm->alpha_moments >= 0.0f && prm->alpha_moments <= 1.0f))
    return fail(P3D_ERR_INVALID, "p3d_temporal: alpha and alpha_moments must lie in [0, 1]");
  if (!(prm->max_history >= 1.0f)) return fail(P3D_ERR_INVALID, "p3d_temporal: max_history must be a number >= 1");
  if (!(prm->depth_tolerance > 0.0f) || !std::isfinite(prm->depth_tolerance))
    return fail(P3D_ERR_INVALID, "p3d_temporal: depth_tolerance must be a finite number > 0");
  if (!(prm->normal_tolerance >= -1.0f && prm->normal_tolerance <= 1.0f))
    return fail(P3D_ERR_INVALID, "p3d_temporal: normal_tolerance must lie in [-1, 1]");
  if (prm->variance_min_history > (1u << 24)) return fail(P3D_ERR_INVALID, "p3d_temporal: variance_min_history must be at most 2^24");
  if (!(prm->sigma_normal >= 0.0f) || !(prm->sigma_depth >= 0.0f) || !std::isfinite(prm->sigma_normal) || !std::isfinite(prm->sigma_depth))
    return fail(P3D_ERR_INVALID, "p3d_temporal: sigma_normal and sigma_depth must be finite numbers >= 0");
  if (prm->reserved[0] || prm->reserved[1]) return fail(P3D_ERR_INVALID, "p3d_temporal: reserved fields must be 0");
  return P3D_OK;
}

int check_temporal_camera(const p3d_temporal* tp, const p3d_camera* cam) {
  if (cam->res_x != tp->w || cam->res_y != tp->h)
    return fail(P3D_ERR_INVALID, "p3d_temporal: the camera renders " + std::to_string(cam->res_x) + "x" + std::to_string(cam->res_y) +
                                     ", the object is for " + std::to_string(tp->w) + "x" + std::to_string(tp->h));
  if (!camera_usable(*cam)) return fail(P3D_ERR_INVALID, "p3d_temporal: every camera field must be finite, and w, h and plane_dist > 0");
  if (cam->aperture != 0.0f)
    return fail(P3D_ERR_UNSUPPORTED, "p3d_temporal: a lens camera (aperture != 0) is not supported: the pinhole reprojection is not exact for it");
  return P3D_OK;
}

}  // namespace

extern "C" {

void p3d_temporal_params_default(p3d_temporal_params* prm) {
  if (!prm) return;
  *prm = p3d_temporal_params{};
  prm->alpha = 0.2f;  // SVGF's
  prm->alpha_moments = 0.2f;
  prm->max_history = 32.0f;
  prm->depth_tolerance = 0.1f;
  prm->normal_tolerance = 0.9f;
  prm->variance_min_history = 4;
  prm->sigma_normal = 128.0f;  // p3d_denoise_params_default's
  prm->sigma_depth = 1.0f;
}

int p3d_temporal_create(int device, int32_t w, int32_t h, p3d_temporal** out) {
  if (!out) return fail(P3D_ERR_INVALID, "p3d_temporal_create: null argument");
  *out = nullptr;
  if (w <= 0 || h <= 0 || (uint64_t)w * (uint64_t)h > (1ull << 28)) return fail(P3D_ERR_INVALID, "p3d_temporal_create: bad image size");
  P3D_HIP(hipSetDevice(device));
  p3d_temporal* t = new p3d_temporal;
  t->device = device;
  t->w = w;
  t->h = h;
  const size_t n = (size_t)w * h;
  int rc = P3D_OK;
  for (int k = 0; k < 2 && !rc; ++k) {
    rc = t->col[k].ensure(n * sizeof(float4));
    if (!rc) rc = t->mom[k].ensure(n * sizeof(float4));
    if (!rc) rc = t->nd[k].ensure(n * sizeof(float4));
  }
  if (rc) {
    p3d_temporal_destroy(t);
    return rc;
  }
  *out = t;
  return P3D_OK;
}

void p3d_temporal_destroy(p3d_temporal* t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  delete t;
}

int p3d_temporal_reset(p3d_temporal* t) {
  if (!t) return fail(P3D_ERR_INVALID, "p3d_temporal_reset: null object");
  t->frames = 0;
  t->prev = p3d_camera{};
  return P3D_OK;
}

uint32_t p3d_temporal_frames(const p3d_temporal* t) { return t ? t->frames : 0u; }

int p3d_temporal_accumulate_device(p3d_temporal* t, const p3d_temporal_params* prm, const p3d_camera* cam, const float* d_rgb,
                                   const float* d_normal_depth, const float* d_albedo_cov, float* d_out_rgb, float* d_out_var,
                                   float* d_out_history, void* hip_stream) {
  if (prm) if (int rc = check_temporal_params(prm)) return rc;
  if (!t || !prm || !cam || !d_rgb || !d_normal_depth || !d_albedo_cov || !d_out_rgb)
    return fail(P3D_ERR_INVALID, "p3d_temporal_accumulate: null argument");
  if (((uintptr_t)d_normal_depth | (uintptr_t)d_albedo_cov) & 15u)
    return fail(P3D_ERR_INVALID, "p3d_temporal_accumulate: the feature buffers must be 16-byte aligned");
  if (int rc = check_temporal_camera(t, cam)) return rc;
  P3D_HIP(hipSetDevice(t->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const uint32_t cur = t->frames & 1u, prv = cur ^ 1u;
  TemporalParams T{};
  T.cam = dev_camera(*cam);
  T.prev = dev_camera(t->prev);
  T.rgb = d_rgb; T.nd = (const float4*)d_normal_depth; T.ac = (const float4*)d_albedo_cov;
  T.col_prev = (const float4*)t->col[prv].p; T.mom_prev = (const float4*)t->mom[prv].p; T.nd_prev = (const float4*)t->nd[prv].p;
  T.col = (float4*)t->col[cur].p; T.mom = (float4*)t->mom[cur].p; T.ndc = (float4*)t->nd[cur].p;
  T.out_rgb = d_out_rgb; T.out_history = d_out_history; T.out_var = d_out_var;
  T.w = t->w; T.h = t->h;
  T.has_prev = t->frames > 0 ? 1u : 0u;
  T.same_view = T.has_prev && std::memcmp(&T.cam, &T.prev, sizeof(DevCamera)) == 0 ? 1u : 0u;
  T.alpha = prm->alpha; T.alpha_moments = prm->alpha_moments; T.max_history = prm->max_history;
  T.depth_tolerance = prm->depth_tolerance; T.normal_tolerance = prm->normal_tolerance;
  T.variance_min_history = (float)prm->variance_min_history;
  T.sigma_normal = prm->sigma_normal; T.sigma_depth = prm->sigma_depth;
  const dim3 grid(((uint32_t)t->w + kTemporalEdge - 1) / kTemporalEdge, ((uint32_t)t->h + kTemporalEdge - 1) / kTemporalEdge);
  hipLaunchKernelGGL(temporal_reproject_kernel, grid, dim3(kTemporalThreads), 0, st, T);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("p3d_temporal launch: ") + hipGetErrorString(e));
  if (d_out_var) {
    hipLaunchKernelGGL(temporal_variance_kernel, grid, dim3(kTemporalThreads), 0, st, T);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("p3d_temporal launch: ") + hipGetErrorString(e));
  }
  ++t->frames;
  t->prev = *cam;
  return P3D_OK;
}

int p3d_temporal_accumulate(p3d_temporal* t, const p3d_temporal_params* prm, const p3d_camera* cam, const float* rgb,
                            const float* normal_depth, const float* albedo_cov, float* out_rgb, float* out_var, float* out_history) {
  if (prm) if (int rc = check_temporal_params(prm)) return rc;  // (first: the parameters are checked without an object)
  if (!t || !prm || !cam || !rgb || !normal_depth || !albedo_cov || !out_rgb)
    return fail(P3D_ERR_INVALID, "p3d_temporal_accumulate: null argument");
  if (int rc = check_temporal_camera(t, cam)) return rc;
  P3D_HIP(hipSetDevice(t->device));
  const size_t n = (size_t)t->w * t->h;
  if (int rc = t->h_rgb.ensure(n * 3 * sizeof(float))) return rc;
  if (int rc = t->h_nd.ensure(n * sizeof(float4))) return rc;
  if (int rc = t->h_ac.ensure(n * sizeof(float4))) return rc;
  if (int rc = t->h_out.ensure(n * 3 * sizeof(float))) return rc;
  if (out_var) if (int rc = t->h_var.ensure(n * sizeof(float))) return rc;
  if (out_history) if (int rc = t->h_hist.ensure(n * sizeof(float))) return rc;
  P3D_HIP(hipMemcpy(t->h_rgb.p, rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice));
  P3D_HIP(hipMemcpy(t->h_nd.p, normal_depth, n * sizeof(float4), hipMemcpyHostToDevice));
  P3D_HIP(hipMemcpy(t->h_ac.p, albedo_cov, n * sizeof(float4), hipMemcpyHostToDevice));
  if (int rc = p3d_temporal_accumulate_device(t, prm, cam, (const float*)t->h_rgb.p, (const float*)t->h_nd.p, (const float*)t->h_ac.p,
                                              (float*)t->h_out.p, out_var ? (float*)t->h_var.p : nullptr,
                                              out_history ? (float*)t->h_hist.p : nullptr, nullptr))
    return rc;
  P3D_HIP(hipDeviceSynchronize());
  P3D_HIP(hipMemcpy(out_rgb, t->h_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (out_var) P3D_HIP(hipMemcpy(out_var, t->h_var.p, n * sizeof(float), hipMemcpyDeviceToHost));
  if (out_history) P3D_HIP(hipMemcpy(out_history, t->h_hist.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return P3D_OK;
}

}  // extern "C"
