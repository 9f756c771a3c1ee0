// warp_affine_simple (opencood/models/sub_modules/torch_transformation_utils.py:323-332), written once: the sampling position of an
// output pixel, its bilinear cell and its taps.  Every kernel that warps an agent map into the ego frame calls these -- the fusion
// kernels (fusion_kernels.h: attention, max, token-major, their backwards), the V2VNet message-passing kernels (v2v_kernels.h) and
// warp_affine_kernel / warp_affine_bwd_kernel (v2xvit_kernels.h: V2X-ViT, where2comm, CoBEVT) -- which live in different translation
// units: device functions only, no kernel is defined here.  The max backward recomputes the forward's winners and the gather passes
// re-derive the forward's cells from them, so the layers below are the only place this arithmetic may be written.
//   fuse_base      affine_grid's base coordinate of an index
//   fuse_point     sampling position: north-west corner + fractions; false = far outside
//   fuse_cell_geo  + the four corners clamped into the map and their validity mask
//   fuse_cell      + the four tap weights
//   fuse_sample    one warped value from a cell
#pragma once
#include "common.h"

namespace gc {

// The cross-unit contract: this header is compiled with contraction on (`fast`, the build's default), stated here so that it does not
// follow from what an includer happened to parse before it.  Every warp kernel in both translation units inherits its rounding from
// this one place, and that is what makes recomputed winners and re-derived cells agree with the forward.
#pragma clang fp contract(fast)

// affine_grid base coordinate of index i on an axis of `size`, align_corners=False: (2i+1)/size - 1, in float64 like theta
__device__ __forceinline__ double fuse_base(int i, int size) { return (2.0 * i + 1.0) / (double)size - 1.0; }

// Sampling position of one (output pixel, agent): float64 affine grid rounded to float32, grid_sampler unnormalize
// (align_corners=False), the north-west corner (x0, y0) clamped into [-2, size + 1] and the fractions.  False when the clamp moved the
// corner: the agent is far away and everything is out of range.
__device__ __forceinline__ bool fuse_point(const double* __restrict__ th, double xb, double yb, int H, int W, int& x0, int& y0, float& tx,
                                           float& ty) {
  const float gx = (float)(th[0] * xb + th[1] * yb + th[2]);
  const float gy = (float)(th[3] * xb + th[4] * yb + th[5]);
  // grid_sampler unnormalize (align_corners=False): ((g + 1) * size - 1) / 2
  const float ix = ((gx + 1.f) * (float)W - 1.f) * 0.5f;
  const float iy = ((gy + 1.f) * (float)H - 1.f) * 0.5f;
  const float fx = floorf(ix), fy = floorf(iy);
  // keep the integer conversion in range for far-away agents
  x0 = (int)fminf(fmaxf(fx, -2.f), (float)W + 1.f);
  y0 = (int)fminf(fmaxf(fy, -2.f), (float)H + 1.f);
  tx = ix - fx; ty = iy - fy;  // == ix - ix_nw etc.
  return !(fx != (float)x0 || fy != (float)y0);
}

// Bilinear cell of one (output pixel, agent) without the weights: the four corners clamped into the map, the 4-bit mask of the valid
// ones (zero for a dead pixel, !live, and for a far-away agent) and the fractions.
__device__ __forceinline__ void fuse_cell_geo(const double* __restrict__ th, double xb, double yb, int H, int W, bool live, int (&idx)[4],
                                              unsigned& ok, float& tx, float& ty) {
  int x0, y0;
  const bool in = fuse_point(th, xb, yb, H, W, x0, y0, tx, ty) && live;
  const bool xl = x0 >= 0 && x0 < W, xr = x0 + 1 >= 0 && x0 + 1 < W;
  const bool yt = y0 >= 0 && y0 < H, yb_ = y0 + 1 >= 0 && y0 + 1 < H;
  // every tap is LOADED, from the corner clamped into the map, and an invalid one is replaced by an exact zero afterwards: with a
  // branch per tap the loads of a channel were issued one memory latency after the other (the token-major kernel's lesson)
  const int xc0 = min(max(x0, 0), W - 1), xc1 = min(max(x0 + 1, 0), W - 1), yc0 = min(max(y0, 0), H - 1), yc1 = min(max(y0 + 1, 0), H - 1);
  idx[0] = yc0 * W + xc0; idx[1] = yc0 * W + xc1; idx[2] = yc1 * W + xc0; idx[3] = yc1 * W + xc1;
  ok = (in && xl && yt ? 1u : 0u) | (in && xr && yt ? 2u : 0u) | (in && xl && yb_ ? 4u : 0u) | (in && xr && yb_ ? 8u : 0u);
}

// Bilinear cell of one (output pixel, agent), shared by the forwards, their backwards and the max backward's winner recomputation.
__device__ __forceinline__ void fuse_cell(const double* __restrict__ th, double xb, double yb, int H, int W, int (&idx)[4], unsigned& ok,
                                          float (&wt)[4]) {
  float tx, ty;
  fuse_cell_geo(th, xb, yb, H, W, true, idx, ok, tx, ty);
  wt[0] = (1.f - tx) * (1.f - ty); wt[1] = tx * (1.f - ty); wt[2] = (1.f - tx) * ty; wt[3] = tx * ty;
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
// Candidates = a window around q's pre-image (float64); each candidate's sampling position is fuse_point's, as in the forward.
// Shared by the gather passes of the attention backward and of the max backward.
// The matches among the candidates [x_lo, x_hi] x [y_lo, y_hi] (inside the map), row by row.
template <class F>
__device__ __forceinline__ void fuse_for_each_match_in(const double* __restrict__ th, int qx, int qy, int H, int W, int x_lo, int x_hi, int y_lo,
                                                       int y_hi, F&& f) {
  for (int py = y_lo; py <= y_hi; ++py)
    for (int px = x_lo; px <= x_hi; ++px) {
      int x0, y0;
      float tx, ty;
      if (!fuse_point(th, fuse_base(px, W), fuse_base(py, H), H, W, x0, y0, tx, ty)) continue;   // far: everything out of range
      const int dx = qx - x0, dy = qy - y0;
      if (dx < 0 || dx > 1 || dy < 0 || dy > 1) continue;
      const float wgt = (dx ? tx : 1.f - tx) * (dy ? ty : 1.f - ty);
      if (wgt == 0.f) continue;
      f(py * W + px, wgt);
    }
}

template <class F>
__device__ __forceinline__ void fuse_for_each_match(const double* __restrict__ th, int qx, int qy, int H, int W, F&& f) {
  const double gx = fuse_base(qx, W), gy = fuse_base(qy, H);
  const double det = th[0] * th[4] - th[1] * th[3];
  const double xb = (th[4] * (gx - th[2]) - th[1] * (gy - th[5])) / det, yb = (-th[3] * (gx - th[2]) + th[0] * (gy - th[5])) / det;
  const double pxf = ((xb + 1.0) * W - 1.0) * 0.5, pyf = ((yb + 1.0) * H - 1.0) * 0.5;
  const int x_lo = max((int)floor(pxf - 1.6), 0), x_hi = min((int)ceil(pxf + 1.6), W - 1);
  const int y_lo = max((int)floor(pyf - 1.6), 0), y_hi = min((int)ceil(pyf + 1.6), H - 1);
  fuse_for_each_match_in(th, qx, qy, H, W, x_lo, x_hi, y_lo, y_hi, f);
}

// The same for ANY transform: the candidates are the bounding box of the pre-image of the 2 x 2 cell around (qx, qy), from the L1 row norms
// of the inverse map in pixel units (the quantity fuse_bwd_plan_kernel bounds by 1.5 for a tame transform); the whole map where the
// transform is singular.  Slow where the map shrinks an agent much, exact, and without atomics.
template <class F>
__device__ __forceinline__ void fuse_for_each_match_wide(const double* __restrict__ th, int qx, int qy, int H, int W, F&& f) {
  int x_lo = 0, x_hi = W - 1, y_lo = 0, y_hi = H - 1;
  const double det = th[0] * th[4] - th[1] * th[3];
  if (fabs(det) > 1e-12 && fabs(det) < 1e12) {
    const double gx = fuse_base(qx, W), gy = fuse_base(qy, H);
    const double xb = (th[4] * (gx - th[2]) - th[1] * (gy - th[5])) / det, yb = (-th[3] * (gx - th[2]) + th[0] * (gy - th[5])) / det;
    const double pxf = ((xb + 1.0) * W - 1.0) * 0.5, pyf = ((yb + 1.0) * H - 1.0) * 0.5;
    const double m00 = th[0], m01 = th[1] * W / H, m10 = th[3] * H / W, m11 = th[4];   // det of this matrix == det
    const double hx = (fabs(m11) + fabs(m01)) / fabs(det) * 1.001 + 0.6, hy = (fabs(m10) + fabs(m00)) / fabs(det) * 1.001 + 0.6;
    const double xl = floor(pxf - hx), xh = ceil(pxf + hx), yl = floor(pyf - hy), yh = ceil(pyf + hy);
    if (xl == xl && xh == xh && yl == yl && yh == yh) {   // clamped as doubles: the conversions below stay in range
      x_lo = (int)fmin(fmax(xl, 0.0), (double)W); x_hi = (int)fmax(fmin(xh, (double)(W - 1)), -1.0);
      y_lo = (int)fmin(fmax(yl, 0.0), (double)H); y_hi = (int)fmax(fmin(yh, (double)(H - 1)), -1.0);
    }
  }
  fuse_for_each_match_in(th, qx, qy, H, W, x_lo, x_hi, y_lo, y_hi, f);
}

}  // namespace gc
