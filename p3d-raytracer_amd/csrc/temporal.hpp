// temporal.hpp — temporal accumulation of path-traced frames under a moving camera: p3d_temporal (include/p3d.h).
//
// SVGF's history (Schied et al. 2017) without its filter: every pixel of the new frame finds the surface point it sees, projects
// it into the previous frame's camera and takes the previous frame's integrated colour, luminance moments and history length
// from the four pixels around that point (bilinear weights, each tap kept only if it saw the same surface: coverage, depth and
// normal tests).  The new frame is blended in with weight max(alpha, 1/n), so a pixel with a history of n frames holds their
// running mean until 1/n drops below alpha.  The luminance moments give a variance per pixel that feeds p3d_denoise's
// luminance term; pixels with a short history take it from a 7x7 spatial estimate instead (temporal_variance_kernel).
//
// State per pixel, float4 images the object owns twice (ping-pong by frame parity, so no copy launch is needed): (R, G, B, n),
// (m1, m2, coverage, 0) and the frame's normal_depth.  temporal_reproject_kernel reads the previous frame's set and writes the
// current one.  Workgroups of 256 lanes cover 16x16 pixels, each wave one 8x8 block, as atrous_kernel (denoise.hpp).
//
// The projection and the blend are evaluated in float64 from the float32 inputs and state, and rounded to float32 once: a
// float32 projection carries ~1e-5 pixel of rounding at 128 pixels across, which the bilinear weights would turn into colour
// error well above what tests/temporal_reference.py (the float64 statement of the same formula) is compared at.  The kernel is
// bound by memory: the double arithmetic costs nothing measurable.  The spatial variance weights are float32 (expf / powf), as
// the denoiser's.  No fast math, no contraction.
#pragma once

#include "device_core.hpp"

namespace p3d {

constexpr int kTemporalThreads = 256;  // 16x16 pixels, four 8x8 waves
constexpr int kTemporalEdge = 16;
constexpr int kTemporalVarRadius = 3;  // the 7x7 spatial estimate

struct TemporalParams {
  DevCamera cam;          // the frame's camera
  DevCamera prev;         // the previous frame's (has_prev)
  const float* rgb;       // [3 * pixel] the frame's linear colour
  const float4* nd;       // [pixel] (n, t) of the frame: p3d_render_features
  const float4* ac;       // [pixel] (albedo, coverage)
  const float4* col_prev; // previous state: (R, G, B, n)
  const float4* mom_prev; //                 (m1, m2, coverage, 0)
  const float4* nd_prev;  //                 normal_depth
  float4* col;            // current state, same layout
  float4* mom;
  float4* ndc;
  float* out_rgb;         // [3 * pixel]
  float* out_history;     // [pixel] n (may be null)
  float* out_var;         // [pixel] luminance variance (may be null)
  int32_t w, h;
  uint32_t has_prev;      // 0: the first frame since create / reset
  uint32_t same_view;     // the previous camera is this one, bit for bit: every pixel projects onto itself
  float alpha, alpha_moments, max_history, depth_tolerance, normal_tolerance;
  float variance_min_history;
  float sigma_normal, sigma_depth;
};

__device__ __forceinline__ void temporal_pixel(int& c, int& r) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  c = (int)(blockIdx.x * kTemporalEdge + (wave & 1u) * 8 + (lane & 7u));
  r = (int)(blockIdx.y * kTemporalEdge + (wave >> 1) * 8 + (lane >> 3));
}

__global__ void __launch_bounds__(kTemporalThreads) temporal_reproject_kernel(const TemporalParams T) {
  int c, r;
  temporal_pixel(c, r);
  if (c >= T.w || r >= T.h) return;
  const size_t p = (size_t)r * (size_t)T.w + (size_t)c;
  const float4 ndp = T.nd[p], acp = T.ac[p];
  const double cr = T.rgb[3 * p], cg = T.rgb[3 * p + 1], cb = T.rgb[3 * p + 2];
  const bool cov_p = acp.w > 0.0f;
  double W = 0.0, hr = 0.0, hg = 0.0, hb = 0.0, hn = 0.0, h1 = 0.0, h2 = 0.0;
  if (T.has_prev) {
    F3 o, d;
    primary_ray(T.cam, (float)c + 0.5f, (float)r + 0.5f, o, d);
    (void)o;
    const DevCamera& q = T.prev;
    // e: the point seen (or, for a miss, the direction) relative to the previous eye
    double ex = d.x, ey = d.y, ez = d.z;
    if (cov_p) {
      const double t = ndp.w;
      ex = ((double)T.cam.eye.x + t * (double)d.x) - (double)q.eye.x;
      ey = ((double)T.cam.eye.y + t * (double)d.y) - (double)q.eye.y;
      ez = ((double)T.cam.eye.z + t * (double)d.z) - (double)q.eye.z;
    }
    const double dist = sqrt((ex * ex + ey * ey) + ez * ez);
    double px = c, py = r;
    bool in_front = true;
    if (!T.same_view) {
      const double a = (ex * (double)q.u.x + ey * (double)q.u.y) + ez * (double)q.u.z;
      const double b = (ex * (double)q.v.x + ey * (double)q.v.y) + ez * (double)q.v.z;
      const double cc = (ex * (double)q.n.x + ey * (double)q.n.y) + ez * (double)q.n.z;
      in_front = cc < 0.0;
      if (in_front) {
        const double s = -(double)q.plane_dist / cc;
        px = ((a * s) / (double)q.w + 0.5) * (double)q.res_x - 0.5;
        py = ((b * s) / (double)q.h + 0.5) * (double)q.res_y - 0.5;
      }
    }
    // (outside (-1, w) x (-1, h) no tap with a non-zero weight lies in the image; the test also keeps the int conversion safe)
    if (in_front && px > -1.0 && px < (double)T.w && py > -1.0 && py < (double)T.h) {
      const double fx0 = floor(px), fy0 = floor(py);
      const double fx = px - fx0, fy = py - fy0;
      const int x0 = (int)fx0, y0 = (int)fy0;
      const double np2 = ((double)ndp.x * ndp.x + (double)ndp.y * ndp.y) + (double)ndp.z * ndp.z;
      for (int k = 0; k < 4; ++k) {
        const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
        const double wk = ((k & 1) ? fx : 1.0 - fx) * ((k >> 1) ? fy : 1.0 - fy);
        if (wk == 0.0 || qx < 0 || qx >= T.w || qy < 0 || qy >= T.h) continue;
        const size_t qi = (size_t)qy * (size_t)T.w + (size_t)qx;
        const float4 mq = T.mom_prev[qi];
        if (cov_p != (mq.z > 0.0f)) continue;
        if (cov_p) {
          const float4 nq = T.nd_prev[qi];
          if (!(fabs((double)nq.w - dist) <= (double)T.depth_tolerance * dist)) continue;
          const double nn = ((double)ndp.x * nq.x + (double)ndp.y * nq.y) + (double)ndp.z * nq.z;
          const double nq2 = ((double)nq.x * nq.x + (double)nq.y * nq.y) + (double)nq.z * nq.z;
          if (!(nn >= ((double)T.normal_tolerance * sqrt(np2)) * sqrt(nq2))) continue;
        }
        const float4 cq = T.col_prev[qi];
        W += wk;
        hr += wk * cq.x; hg += wk * cq.y; hb += wk * cq.z; hn += wk * cq.w;
        h1 += wk * mq.x; h2 += wk * mq.y;
      }
    }
  }
  const double Y = (0.2126 * cr + 0.7152 * cg) + 0.0722 * cb;
  float n = 1.0f;
  double orr = cr, og = cg, ob = cb, m1 = Y, m2 = Y * Y;
  if (W >= 1.0e-3) {
    n = (float)fmin(hn / W + 1.0, (double)T.max_history);  // (kept in float32: equal histories stay whole numbers)
    const double a = fmax((double)T.alpha, 1.0 / (double)n), am = fmax((double)T.alpha_moments, 1.0 / (double)n);
    orr = (1.0 - a) * (hr / W) + a * cr;
    og = (1.0 - a) * (hg / W) + a * cg;
    ob = (1.0 - a) * (hb / W) + a * cb;
    m1 = (1.0 - am) * (h1 / W) + am * Y;
    m2 = (1.0 - am) * (h2 / W) + am * (Y * Y);
  }
  const float fr = (float)orr, fg = (float)og, fb = (float)ob;
  T.col[p] = make_float4(fr, fg, fb, n);
  T.mom[p] = make_float4((float)m1, (float)m2, acp.w, 0.0f);
  T.ndc[p] = ndp;
  T.out_rgb[3 * p] = fr; T.out_rgb[3 * p + 1] = fg; T.out_rgb[3 * p + 2] = fb;
  if (T.out_history) T.out_history[p] = n;
  if (T.out_var && n >= T.variance_min_history) T.out_var[p] = (float)fmax(0.0, m2 - m1 * m1);
}

// The variance of the pixels whose history is shorter than variance_min_history: the moments averaged over the 7x7
// neighbourhood of the current frame, weighted by p3d_denoise's w_g at step 1 (albedo term off) and 1 for the centre.
__global__ void __launch_bounds__(kTemporalThreads) temporal_variance_kernel(const TemporalParams T) {
  int c, r;
  temporal_pixel(c, r);
  if (c >= T.w || r >= T.h) return;
  const size_t p = (size_t)r * (size_t)T.w + (size_t)c;
  if (T.col[p].w >= T.variance_min_history) return;  // (temporal_reproject_kernel wrote it)
  const float4 ndp = T.ndc[p], mp = T.mom[p];
  const bool cov_p = mp.z > 0.0f;
  const float depth_den = T.sigma_depth * 1.0f * ndp.w;
  double ws = 0.0, s1 = 0.0, s2 = 0.0;
  for (int dy = -kTemporalVarRadius; dy <= kTemporalVarRadius; ++dy) {
    const int qr = r + dy;
    if (qr < 0 || qr >= T.h) continue;
    for (int dx = -kTemporalVarRadius; dx <= kTemporalVarRadius; ++dx) {
      const int qc = c + dx;
      if (qc < 0 || qc >= T.w) continue;
      const size_t q = (size_t)qr * (size_t)T.w + (size_t)qc;
      float wg = 1.0f;  // the centre tap
      float4 mq = mp;
      if (dx != 0 || dy != 0) {
        mq = T.mom[q];
        const bool cov_q = mq.z > 0.0f;
        if (cov_p != cov_q) {
          wg = 0.0f;
        } else if (cov_p) {
          const float4 ndq = T.ndc[q];
          if (T.sigma_normal != 0.0f) {
            const float nn = ndp.x * ndq.x + ndp.y * ndq.y + ndp.z * ndq.z;
            wg = wg * powf(fmaxf(0.0f, nn), T.sigma_normal);
          }
          if (T.sigma_depth != 0.0f) wg = wg * expf(-fabsf(ndp.w - ndq.w) / depth_den);
        }
      }
      ws += (double)wg;
      s1 += (double)wg * mq.x;
      s2 += (double)wg * mq.y;
    }
  }
  const double a1 = s1 / ws, a2 = s2 / ws;
  T.out_var[p] = (float)fmax(0.0, a2 - a1 * a1);
}

}  // namespace p3d
