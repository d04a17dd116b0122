// capi_denoise.hpp — feature buffers, the a-trous filter, the variance of an adaptive frame (kernels: features.hpp, denoise.hpp)
#pragma once
#include "capi_adaptive.hpp"

extern "C" {

int p3d_render_features_device(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, uint32_t samples, float* d_normal_depth,
                               float* d_albedo_cov, void* hip_stream) {
  if (!s || !cfg || !tile || !d_normal_depth || !d_albedo_cov) return fail(P3D_ERR_INVALID, "p3d_render_features: null argument");
  if (((uintptr_t)d_normal_depth | (uintptr_t)d_albedo_cov) & 15u) return fail(P3D_ERR_INVALID, "p3d_render_features: the feature buffers must be 16-byte aligned");
  if (tile->stripe_h > 0 && tile->stripe_stride > 1)
    return fail(P3D_ERR_UNSUPPORTED, "p3d_render_features: striped tiles are not supported (the denoiser filters a buffer as one image)");
  if (int rc = check_frame(s, cfg, tile)) return rc;
  const uint32_t total = cfg->antialiasing ? cfg->spp_sqrt * cfg->spp_sqrt : 1u;
  const uint32_t k = samples ? samples : std::min<uint32_t>(16, total);
  if (k > total)
    return fail(P3D_ERR_INVALID, "p3d_render_features: " + std::to_string(samples) + " samples asked, the frame has " + std::to_string(total) +
                                     (cfg->antialiasing ? " per pixel" : " (antialiasing = 0: only the pixel-centre ray)"));
  FeatureParams F{};
  F.normal_depth = (float4*)d_normal_depth;
  F.albedo_cov = (float4*)d_albedo_cov;
  F.samples = k;
  return render_feature_buffers(s, cfg, tile, hip_stream, k, F);
}

int p3d_render_features(p3d_scene* s, const p3d_config* cfg, const p3d_tile* tile, uint32_t samples, float* normal_depth, float* albedo_cov) {
  if (!s || !cfg || !tile || !normal_depth || !albedo_cov) return fail(P3D_ERR_INVALID, "p3d_render_features: null argument");
  if (tile->w <= 0 || tile->h <= 0) return fail(P3D_ERR_INVALID, "empty tile");
  P3D_HIP(hipSetDevice(s->device));
  const size_t n = (size_t)tile->w * tile->h;
  if (int rc = s->q_out.ensure(n * 2 * sizeof(float4))) return rc;
  float* d_nd = (float*)s->q_out.p;
  float* d_ac = d_nd + n * 4;
  if (int rc = p3d_render_features_device(s, cfg, tile, samples, d_nd, d_ac, nullptr)) return rc;
  P3D_HIP(hipMemcpy(normal_depth, d_nd, n * sizeof(float4), hipMemcpyDeviceToHost));
  P3D_HIP(hipMemcpy(albedo_cov, d_ac, n * sizeof(float4), hipMemcpyDeviceToHost));
  return P3D_OK;
}

void p3d_denoise_params_default(p3d_denoise_params* prm) {
  if (!prm) return;
  *prm = p3d_denoise_params{};
  prm->iterations = 5;
  prm->sigma_color = 4.0f;   // DESIGN.md "Denoising": chosen on the Cornell box, 16 against 1024 samples per pixel
  prm->sigma_luma = 64.0f;
  prm->sigma_normal = 128.0f;
  prm->sigma_depth = 1.0f;
  prm->sigma_albedo = 0.1f;
  prm->gamma = 1.0f;  // p3d_config_default's GAMMA
}

}  // extern "C"

// The denoiser: two float4 images (R, G, B, var) for the iterations to ping-pong between, made at create so that the
// device-buffer call neither allocates nor waits; the host-buffer call keeps device copies of its arrays besides.
struct p3d_denoiser {
  int device = 0;
  int32_t w = 0, h = 0;
  Scratch ping, pong;
  Scratch h_rgb, h_var, h_nd, h_ac, h_out, h_out8;
};

namespace {

int check_denoise_params(const p3d_denoise_params* prm, bool has_var) {
  if (prm->iterations > 8) return fail(P3D_ERR_INVALID, "p3d_denoise: iterations must be at most 8");
  for (float v : {prm->sigma_color, prm->sigma_luma, prm->sigma_normal, prm->sigma_depth, prm->sigma_albedo})
    if (!(v >= 0.0f)) return fail(P3D_ERR_INVALID, "p3d_denoise: every sigma must be a number >= 0");
  if (has_var && !(prm->sigma_luma > 0.0f)) return fail(P3D_ERR_INVALID, "p3d_denoise: sigma_luma must be > 0 with a variance buffer");
  if (!has_var && !(prm->sigma_color > 0.0f)) return fail(P3D_ERR_INVALID, "p3d_denoise: sigma_color must be > 0 without a variance buffer");
  if (!(prm->gamma > 0.0f)) return fail(P3D_ERR_INVALID, "p3d_denoise: gamma must be a number > 0");
  if (prm->reserved[0] || prm->reserved[1]) return fail(P3D_ERR_INVALID, "p3d_denoise: reserved fields must be 0");
  return P3D_OK;
}

}  // namespace

extern "C" {

int p3d_denoiser_create(int device, int32_t w, int32_t h, p3d_denoiser** out) {
  if (!out) return fail(P3D_ERR_INVALID, "p3d_denoiser_create: null argument");
  *out = nullptr;
  if (w <= 0 || h <= 0 || (uint64_t)w * (uint64_t)h > (1ull << 28)) return fail(P3D_ERR_INVALID, "p3d_denoiser_create: bad image size");
  P3D_HIP(hipSetDevice(device));
  p3d_denoiser* d = new p3d_denoiser;
  d->device = device;
  d->w = w;
  d->h = h;
  const size_t n = (size_t)w * h;
  int rc = d->ping.ensure(n * sizeof(float4));
  if (!rc) rc = d->pong.ensure(n * sizeof(float4));
  if (rc) {
    p3d_denoiser_destroy(d);
    return rc;
  }
  *out = d;
  return P3D_OK;
}

void p3d_denoiser_destroy(p3d_denoiser* d) {
  if (!d) return;
  (void)hipSetDevice(d->device);
  delete d;
}

int p3d_denoise_device(p3d_denoiser* d, const p3d_denoise_params* prm, const float* d_rgb, const float* d_var, const float* d_normal_depth,
                       const float* d_albedo_cov, float* d_out_rgb, uint8_t* d_out_rgb8, void* hip_stream) {
  if (!d || !prm || !d_rgb || !d_normal_depth || !d_albedo_cov) return fail(P3D_ERR_INVALID, "p3d_denoise: null argument");
  if (!d_out_rgb && !d_out_rgb8) return fail(P3D_ERR_INVALID, "p3d_denoise: no output");
  if (((uintptr_t)d_normal_depth | (uintptr_t)d_albedo_cov) & 15u) return fail(P3D_ERR_INVALID, "p3d_denoise: the feature buffers must be 16-byte aligned");
  if (int rc = check_denoise_params(prm, d_var != nullptr)) return rc;
  P3D_HIP(hipSetDevice(d->device));
  hipStream_t st = (hipStream_t)hip_stream;
  AtrousParams A{};
  A.rgb_in = d_rgb; A.var_in = d_var;
  A.nd = (const float4*)d_normal_depth; A.ac = (const float4*)d_albedo_cov;
  A.rgb_out = d_out_rgb; A.rgb8_out = d_out_rgb8;
  A.w = d->w; A.h = d->h;
  A.has_var = d_var ? 1u : 0u;
  A.sigma_luma = prm->sigma_luma; A.sigma_normal = prm->sigma_normal; A.sigma_depth = prm->sigma_depth; A.sigma_albedo = prm->sigma_albedo;
  A.gamma = prm->gamma;
  const dim3 grid(((uint32_t)d->w + kAtrousEdge - 1) / kAtrousEdge, ((uint32_t)d->h + kAtrousEdge - 1) / kAtrousEdge);
  const uint32_t n_launch = std::max<uint32_t>(prm->iterations, 1);  // (iterations = 0: one launch that copies the input)
  float4* buf[2] = {(float4*)d->ping.p, (float4*)d->pong.p};
  for (uint32_t i = 0; i < n_launch; ++i) {
    A.first = i == 0 ? 1u : 0u;
    A.last = i + 1 == n_launch ? 1u : 0u;
    A.in = buf[(i + 1) & 1u];
    A.out = buf[i & 1u];
    A.step = prm->iterations ? (int32_t)(1u << i) : 0;
    A.color_scale = (float)((double)(1u << (2 * i)) / ((double)prm->sigma_color * (double)prm->sigma_color));
    hipLaunchKernelGGL(atrous_kernel, grid, dim3(kAtrousThreads), 0, st, A);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("p3d_denoise launch: ") + hipGetErrorString(e));
  }
  return P3D_OK;
}

int p3d_denoise(p3d_denoiser* d, const p3d_denoise_params* prm, const float* rgb, const float* var, const float* normal_depth,
                const float* albedo_cov, float* out_rgb, uint8_t* out_rgb8) {
  if (!d || !prm || !rgb || !normal_depth || !albedo_cov) return fail(P3D_ERR_INVALID, "p3d_denoise: null argument");
  if (!out_rgb && !out_rgb8) return fail(P3D_ERR_INVALID, "p3d_denoise: no output");
  if (int rc = check_denoise_params(prm, var != nullptr)) return rc;
  P3D_HIP(hipSetDevice(d->device));
  const size_t n = (size_t)d->w * d->h;
  if (int rc = d->h_rgb.ensure(n * 3 * sizeof(float))) return rc;
  if (var) if (int rc = d->h_var.ensure(n * sizeof(float))) return rc;
  if (int rc = d->h_nd.ensure(n * sizeof(float4))) return rc;
  if (int rc = d->h_ac.ensure(n * sizeof(float4))) return rc;
  if (out_rgb) if (int rc = d->h_out.ensure(n * 3 * sizeof(float))) return rc;
  if (out_rgb8) if (int rc = d->h_out8.ensure(n * 3)) return rc;
  P3D_HIP(hipMemcpy(d->h_rgb.p, rgb, n * 3 * sizeof(float), hipMemcpyHostToDevice));
  if (var) P3D_HIP(hipMemcpy(d->h_var.p, var, n * sizeof(float), hipMemcpyHostToDevice));
  P3D_HIP(hipMemcpy(d->h_nd.p, normal_depth, n * sizeof(float4), hipMemcpyHostToDevice));
  P3D_HIP(hipMemcpy(d->h_ac.p, albedo_cov, n * sizeof(float4), hipMemcpyHostToDevice));
  if (int rc = p3d_denoise_device(d, prm, (const float*)d->h_rgb.p, var ? (const float*)d->h_var.p : nullptr, (const float*)d->h_nd.p,
                                  (const float*)d->h_ac.p, out_rgb ? (float*)d->h_out.p : nullptr, out_rgb8 ? (uint8_t*)d->h_out8.p : nullptr, nullptr))
    return rc;
  P3D_HIP(hipDeviceSynchronize());
  if (out_rgb) P3D_HIP(hipMemcpy(out_rgb, d->h_out.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost));
  if (out_rgb8) P3D_HIP(hipMemcpy(out_rgb8, d->h_out8.p, n * 3, hipMemcpyDeviceToHost));
  return P3D_OK;
}

int p3d_denoise_variance_device(p3d_adaptive* a, float* d_var, void* hip_stream) {
  if (!a || !d_var) return fail(P3D_ERR_INVALID, "p3d_denoise_variance: null argument");
  P3D_HIP(hipSetDevice(a->device));
  VarianceParams V{};
  V.sum = (const float*)a->sum.p; V.sum_y2 = (const float*)a->sum_y2.p; V.samples = (const uint32_t*)a->samples.p;
  V.var = d_var;
  V.n = (uint32_t)adapt_pixels(a);
  hipLaunchKernelGGL(adapt_variance_kernel, dim3((V.n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, V);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return fail(P3D_ERR_NO_DEVICE, std::string("p3d_denoise_variance launch: ") + hipGetErrorString(e));
  return P3D_OK;
}

int p3d_denoise_variance(p3d_adaptive* a, float* var) {
  if (!a || !var) return fail(P3D_ERR_INVALID, "p3d_denoise_variance: null argument");
  P3D_HIP(hipSetDevice(a->device));
  P3D_HIP(hipDeviceSynchronize());
  const size_t px = adapt_pixels(a);
  if (int rc = a->var.ensure(px * sizeof(float))) return rc;
  if (int rc = p3d_denoise_variance_device(a, (float*)a->var.p, nullptr)) return rc;
  P3D_HIP(hipDeviceSynchronize());
  P3D_HIP(hipMemcpy(var, a->var.p, px * sizeof(float), hipMemcpyDeviceToHost));
  return P3D_OK;
}

}  // extern "C"
