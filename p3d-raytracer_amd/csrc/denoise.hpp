// denoise.hpp — the edge-avoiding a-trous wavelet filter of p3d_denoise (include/p3d.h) and the per-pixel variance of an
// adaptive frame (p3d_denoise_variance).
//
// atrous_kernel is ONE iteration i of the filter (Dammertz et al. 2010; with a variance buffer, the luminance term of SVGF,
// Schied et al. 2017): a 5x5 B3-spline kernel whose taps lie 2^i pixels apart, every tap weighted by how alike its normal,
// depth, albedo and coverage are to the centre's and by a colour (or luminance) distance.  The host launches it once per
// iteration and ping-pongs between two float4 images (R, G, B, var) the denoiser owns; iteration 0 reads the caller's rgb
// (and var), the last one writes the caller's outputs.  Workgroups of 256 lanes cover 16x16 pixels, each wave one 8x8
// block, so that a wave's taps of one (dx, dy) are one 8x8 block of the image: eight 128-byte rows of float4.  The
// weights are evaluated in float32 with expf / powf / sqrtf (no fast math, no contraction); tests/atrous_reference.py is
// the float64 statement of the same formula the GPU result is checked against.
#pragma once

#include "device_core.hpp"

namespace p3d {

constexpr int kAtrousThreads = 256;  // 16x16 pixels, four 8x8 waves
constexpr int kAtrousEdge = 16;

struct AtrousParams {
  const float* rgb_in;   // iteration 0: the caller's w*h*3 colour and w*h variance (may be null)
  const float* var_in;
  const float4* in;      // later iterations: (R, G, B, var) of the one before
  const float4* nd;      // (n, t) per pixel: p3d_render_features
  const float4* ac;      // (albedo, coverage) per pixel
  float4* out;           // all but the last iteration
  float* rgb_out;        // the last iteration (either may be null)
  uint8_t* rgb8_out;
  int32_t w, h;
  int32_t step;          // 2^i; 0: no filtering, the input is the output (iterations = 0)
  uint32_t first, last, has_var;
  float color_scale;     // without variance: 4^i / sigma_color^2
  float sigma_luma, sigma_normal, sigma_depth, sigma_albedo;
  float gamma;
};

__device__ __forceinline__ float atrous_luma(float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }

__device__ __forceinline__ float4 atrous_colour(const AtrousParams& A, size_t q) {
  if (A.first) return make_float4(A.rgb_in[3 * q], A.rgb_in[3 * q + 1], A.rgb_in[3 * q + 2], A.var_in ? A.var_in[q] : 0.0f);
  return A.in[q];
}

__global__ void __launch_bounds__(kAtrousThreads) atrous_kernel(const AtrousParams A) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const int c = (int)(blockIdx.x * kAtrousEdge + (wave & 1u) * 8 + (lane & 7u));
  const int r = (int)(blockIdx.y * kAtrousEdge + (wave >> 1) * 8 + (lane >> 3));
  if (c >= A.w || r >= A.h) return;
  const size_t p = (size_t)r * (size_t)A.w + (size_t)c;
  const float4 cp = atrous_colour(A, p);
  float4 res = cp;
  if (A.step > 0) {
    const float kk[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    const float4 ndp = A.nd[p], acp = A.ac[p];
    const bool cov_p = acp.w != 0.0f;
    const float yp = atrous_luma(cp);
    // luminance term with variance: exp(-|Yp - Yq| / lum_den); the depth term's denominator
    const float lum_den = A.sigma_luma * sqrtf(cp.w) + 1.0e-4f;
    const float depth_den = A.sigma_depth * (float)A.step * ndp.w;
    float wsum = 0.0f, vsum = 0.0f;
    float rs = 0.0f, gs = 0.0f, bs = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
      const int qr = r + dy * A.step;
      if (qr < 0 || qr >= A.h) continue;
      for (int dx = -2; dx <= 2; ++dx) {
        const int qc = c + dx * A.step;
        if (qc < 0 || qc >= A.w) continue;
        const size_t q = (size_t)qr * (size_t)A.w + (size_t)qc;
        const float hk = kk[dx + 2] * kk[dy + 2];
        float4 cq = cp;
        float wt = 1.0f;  // the centre tap
        if (dx != 0 || dy != 0) {
          cq = atrous_colour(A, q);
          const float4 ndq = A.nd[q], acq = A.ac[q];
          const bool cov_q = acq.w != 0.0f;
          float wg;
          if (!cov_p && !cov_q) {
            wg = 1.0f;
          } else if (cov_p != cov_q) {
            wg = 0.0f;
          } else {
            wg = 1.0f;
            if (A.sigma_normal != 0.0f) {
              const float nn = ndp.x * ndq.x + ndp.y * ndq.y + ndp.z * ndq.z;
              wg = wg * powf(fmaxf(0.0f, nn), A.sigma_normal);
            }
            if (A.sigma_depth != 0.0f) wg = wg * expf(-fabsf(ndp.w - ndq.w) / depth_den);
            if (A.sigma_albedo != 0.0f) {
              const float ax = acp.x - acq.x, ay = acp.y - acq.y, az = acp.z - acq.z;
              wg = wg * expf(-(ax * ax + ay * ay + az * az) / (A.sigma_albedo * A.sigma_albedo));
            }
          }
          float wc;
          if (A.has_var) {
            wc = expf(-fabsf(yp - atrous_luma(cq)) / lum_den);
          } else {
            const float ex = cp.x - cq.x, ey = cp.y - cq.y, ez = cp.z - cq.z;
            wc = expf(-(ex * ex + ey * ey + ez * ez) * A.color_scale);
          }
          wt = wg * wc;
        }
        const float hw = hk * wt;
        wsum += hw;
        rs += hw * cq.x;
        gs += hw * cq.y;
        bs += hw * cq.z;
        vsum += (hw * hw) * cq.w;
      }
    }
    res = make_float4(rs / wsum, gs / wsum, bs / wsum, vsum / (wsum * wsum));
  }
  if (!A.last) {
    A.out[p] = res;
    return;
  }
  if (A.rgb_out) {
    A.rgb_out[3 * p] = res.x; A.rgb_out[3 * p + 1] = res.y; A.rgb_out[3 * p + 2] = res.z;
  }
  if (A.rgb8_out) store_rgb8(A.rgb8_out + 3 * p, f3(res.x, res.y, res.z), A.gamma);  // the render kernels' epilogue
}

// Variance of every pixel's mean luminance for p3d_denoise_variance: include/p3d.h "Error metric", float32 in that order.
struct VarianceParams {
  const float* sum;         // [3 * pixel] running sums of an adaptive frame
  const float* sum_y2;      // [pixel] S2
  const uint32_t* samples;  // [pixel] samples in the sums
  float* var;               // [pixel] out
  uint32_t n;
};

__global__ void __launch_bounds__(256) adapt_variance_kernel(const VarianceParams V) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= V.n) return;
  const uint32_t sp = V.samples[i];
  float var = 0.0f;
  if (sp >= 2) {
    const float n = (float)sp;
    const float Y = 0.2126f * V.sum[3 * i] + 0.7152f * V.sum[3 * i + 1] + 0.0722f * V.sum[3 * i + 2];
    const float m = Y / n;
    const float v = fmaxf((V.sum_y2[i] - Y * m) / (n - 1.0f), 0.0f);
    var = v / n;
  }
  V.var[i] = var;
}

}  // namespace p3d
