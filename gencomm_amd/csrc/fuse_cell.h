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

}  // namespace gc
