// The bilinear cell and tap arithmetic of warp_affine_simple (opencood/models/sub_modules/torch_transformation_utils.py:323-332), shared
// by the fusion kernels (fusion_kernels.h) and the V2VNet message-passing kernels (v2v_kernels.h), which live in different translation
// units: device functions only, no kernel is defined here.
#pragma once
#include "common.h"

namespace gc {

// Bilinear cell of one (output pixel, agent), shared by the forward (both modes) and by the max backward's winner recomputation:
// float64 affine grid rounded to float32, grid_sampler unnormalize (align_corners=False), the four corners clamped into the map.
__device__ __forceinline__ void fuse_cell(const double* __restrict__ th, double xb, double yb, int H, int W, int (&idx)[4], unsigned& ok,
                                          float (&wt)[4]) {
  const float gx = (float)(th[0] * xb + th[1] * yb + th[2]);
  const float gy = (float)(th[3] * xb + th[4] * yb + th[5]);
  // grid_sampler unnormalize (align_corners=False): ((g + 1) * size - 1) / 2
  const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f;
  const float iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  // keep the integer conversion in range for far-away agents
  const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f);
  const int y0 = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f);
  const float tx = ix - fx, ty = iy - fy;  // == ix - ix_nw etc.
  const float wnw = (1.f - tx) * (1.f - ty), wne = tx * (1.f - ty), wsw = (1.f - tx) * ty, wse = tx * ty;
  const bool xl = x0 >= 0 && x0 < W, xr = x0 + 1 >= 0 && x0 + 1 < W;
  const bool yt = y0 >= 0 && y0 < H, yb_ = y0 + 1 >= 0 && y0 + 1 < H;
  const bool far = fx != (float)x0 || fy != (float)y0;  // clamped => everything out of range
  // every tap is LOADED, from the corner clamped into the map, and an invalid one is replaced by an exact zero afterwards: with a
  // branch per tap the loads of a channel were issued one memory latency after the other (the token-major kernel's lesson)
  const int xc0 = min(max(x0, 0), W - 1), xc1 = min(max(x0 + 1, 0), W - 1), yc0 = min(max(y0, 0), H - 1), yc1 = min(max(y0 + 1, 0), H - 1);
  idx[0] = yc0 * W + xc0; idx[1] = yc0 * W + xc1; idx[2] = yc1 * W + xc0; idx[3] = yc1 * W + xc1;
  ok = (xl && yt && !far ? 1u : 0u) | (xr && yt && !far ? 2u : 0u) | (xl && yb_ && !far ? 4u : 0u) | (xr && yb_ && !far ? 8u : 0u);
  wt[0] = wnw; wt[1] = wne; wt[2] = wsw; wt[3] = wse;
}

// One warped value: the four taps of a cell, an invalid tap contributing an exact zero (fixed fma order: the max backward recomputes
// the forward's values bit for bit with this).
__device__ __forceinline__ float fuse_sample(const float* __restrict__ plane, const int (&idx)[4], unsigned ok, const float (&wt)[4]) {
  float t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) t[k] = plane[idx[k]];
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) v = fmaf((ok >> k) & 1u ? t[k] : 0.f, wt[k], v);
  return v;
}

// The most matches a gather pass keeps per source pixel (fuse_bwd_plan_kernel's bound for a tame transform).
constexpr int FUSE_KM = 12;

// Every output pixel p whose bilinear cell (agent transform th) contains the source pixel (qx, qy), with its tap weight: f(p, wgt).
// Candidates = a window around q's pre-image (float64); each candidate's cell is recomputed with exactly fuse_body's arithmetic.
// Shared by the gather passes of the attention backward and of the max backward.
template <class F>
__device__ __forceinline__ void fuse_for_each_match(const double* __restrict__ th, int qx, int qy, int H, int W, F&& f) {
  const double gx = (2.0 * qx + 1.0) / (double)W - 1.0, gy = (2.0 * qy + 1.0) / (double)H - 1.0;
  const double det = th[0] * th[4] - th[1] * th[3];
  const double xb = (th[4] * (gx - th[2]) - th[1] * (gy - th[5])) / det, yb = (-th[3] * (gx - th[2]) + th[0] * (gy - th[5])) / det;
  const double pxf = ((xb + 1.0) * W - 1.0) * 0.5, pyf = ((yb + 1.0) * H - 1.0) * 0.5;
  const int x_lo = max((int)floor(pxf - 1.6), 0), x_hi = min((int)ceil(pxf + 1.6), W - 1);
  const int y_lo = max((int)floor(pyf - 1.6), 0), y_hi = min((int)ceil(pyf + 1.6), H - 1);
  for (int py = y_lo; py <= y_hi; ++py)
    for (int px = x_lo; px <= x_hi; ++px) {
      const double oxb = (2.0 * px + 1.0) / (double)W - 1.0, oyb = (2.0 * py + 1.0) / (double)H - 1.0;
      const float sgx = (float)(th[0] * oxb + th[1] * oyb + th[2]);
      const float sgy = (float)(th[3] * oxb + th[4] * oyb + th[5]);
      const float ix = ((sgx + 1.f) * (float)W - 1.f) * 0.5f, iy = ((sgy + 1.f) * (float)H - 1.f) * 0.5f;
      const float fx = floorf(ix), fy = floorf(iy);
      const int x0 = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f), y0 = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f);
      if (fx != (float)x0 || fy != (float)y0) continue;   // clamped: everything out of range
      const int dx = qx - x0, dy = qy - y0;
      if (dx < 0 || dx > 1 || dy < 0 || dy > 1) continue;
      const float tx = ix - fx, ty = iy - fy;
      const float wgt = (dx ? tx : 1.f - tx) * (dy ? ty : 1.f - ty);
      if (wgt == 0.f) continue;
      f(py * W + px, wgt);
    }
}

}  // namespace gc
