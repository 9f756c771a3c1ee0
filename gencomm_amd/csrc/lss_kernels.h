// Lift-Splat-Shoot camera encoder (reference: opencood/models/heter_encoders.py:83-241 LiftSplatShoot,
// sub_modules/lss_submodule.py:140-233 CamEncode_Resnet101, utils/camera_utils.py:129-246 bin_depths / QuickCumsum).
//
// The reference lifts every frustum point to a C-channel row (depth (x) feature: B N D fH fW C floats, 231 MB per agent at the
// m4 shape), masks, argsorts and gathers that tensor and runs QuickCumsum over it (cumsum + difference of prefix sums) to fill a
// 33.5 MB BEV map.  Here the outer product never exists:
//   lss_lift_kernel     one thread per image-feature pixel: softmax over the D depth logits -> prob [BN][D][fH][fW] (= one value
//                       per frustum point, in the reference's point order); get_geometry + voxel_pooling's cell arithmetic for the
//                       pixel's D points -> sort key (the reference's rank, or the sentinel ncells outside the grid); the image
//                       features transposed to pixel-major featT [BN][fH][fW][C] through LDS (one C-float row per point)
//   rocPRIM radix sort  (key, point) pairs, stable: within a cell the points stay in the reference's flattening order
//   lss_splat_kernel    output-driven: a workgroup owns 64 consecutive x-cells of one (b, z, y) row; each cell's interval
//                       [lower_bound(rank), lower_bound(rank + 1)) of the sorted keys is found by binary search (no interval
//                       table, no host synchronisation, no memset); a wave sums prob * featT row over the interval (lanes =
//                       channels, 256-byte row reads), the tile is staged in LDS and stored as 256-byte runs of the channel-major
//                       map.  Empty cells are written as zeros by the same stores.  Fixed summation order, no atomics.
//
// Backward (training the camera encoder, gencomm_lss_splat_bwd), pixel-driven -- no sort, no atomics, no memset:
//   lss_grad_rows_kernel  grad_out [B][nz C][ny][nx] transposed once through LDS to cell-major rows gT [B][nz][ny][nx][C], so that
//                         a frustum point reads the C gradient values of its cell as one contiguous row
//   lss_splat_bwd_kernel  one wave per pixel (lanes = channels, the pixel's feature row in registers) walks the D depth bins with
//                         four row reads in flight: dprob_d = <g_d, feat> (one DPP wave sum), dfeat += prob_d g_d in registers in the
//                         order of d, then the softmax backward in the same wave; d_depth_logit and d_feat are staged in LDS per
//                         workgroup (32 consecutive pixels of one camera) and stored along hw
// and the two trunk gradients the general convolution autograd lacks: maxpool3x3s2_bwd_kernel (input-driven gather, the forward's
// arg-max rule recomputed) and stem7x7_wgrad_kernel (+ its fixed-order reduction) for the 7x7 stride-2 pad-3 stem.
#pragma once
#include <rocprim/rocprim.hpp>

#include "common.h"

namespace gc {

// Contraction is off in this header for a historical reason, not a numerical one: since it was written it has been compiled behind
// iou3d_kernels.h, which used to leave `off` in force for every later include of its translation unit.  Its float64 comparisons and
// golden fixtures were taken on these bits, so the mode is pinned here rather than inherited; nothing in the arithmetic below is
// known to need it.
#pragma clang fp contract(off)

struct LssGeom {
  float lo[3], dx[3];   // bx - dx / 2 and dx (float32, as the reference's tensors)
  int nx, ny, nz;       // cells per axis
  int B, N, D, fH, fW, C;
};

// 3x3 inverse (adjugate over the determinant, in double, rounded once to float)
__device__ __forceinline__ void lss_inv3(const float* __restrict__ m, float* o) {
  const double a = m[0], b = m[1], c = m[2], d = m[3], e = m[4], f = m[5], g = m[6], h = m[7], i = m[8];
  const double A = e * i - f * h, Bc = -(d * i - f * g), Cc = d * h - e * g;
  const double det = a * A + b * Bc + c * Cc;
  const double r = 1.0 / det;
  o[0] = (float)(A * r);  o[1] = (float)(-(b * i - c * h) * r); o[2] = (float)((b * f - c * e) * r);
  o[3] = (float)(Bc * r); o[4] = (float)((a * i - c * g) * r);  o[5] = (float)(-(a * f - c * d) * r);
  o[6] = (float)(Cc * r); o[7] = (float)(-(a * h - b * g) * r); o[8] = (float)((a * e - b * d) * r);
}

// ((p - lo) / dx).long() inside [0, n): truncation toward zero, so (-1, 0) lands in cell 0 exactly as the reference's .long()
__device__ __forceinline__ int lss_cell(float p, float lo, float dx, int n) {
  const float v = __fdiv_rn(__fsub_rn(p, lo), dx);
  return (v > -1.f && v < (float)n) ? (int)v : -1;
}

// block = 64 threads = 64 consecutive pixels of the flattened [BN][fH][fW] grid
__global__ __launch_bounds__(64) void lss_lift_kernel(const float* __restrict__ logit, const float* __restrict__ feat,
                                                      const float* __restrict__ frustum, const float* __restrict__ rots,
                                                      const float* __restrict__ trans, const float* __restrict__ intrins,
                                                      const float* __restrict__ post_rots, const float* __restrict__ post_trans,
                                                      const LssGeom g, float* __restrict__ prob, float* __restrict__ featT,
                                                      unsigned* __restrict__ key, int* __restrict__ val, int* __restrict__ cell) {
  __shared__ float tile[64][65];
  const int HW = g.fH * g.fW, BN = g.B * g.N;
  const long long P = (long long)BN * HW;
  const long long p0 = (long long)blockIdx.x * 64;
  const int t = threadIdx.x;
  const long long p = p0 + t;
  const bool live = p < P;
  const int bn = live ? (int)(p / HW) : 0, hw = live ? (int)(p - (long long)bn * HW) : 0;

  // image features -> pixel-major rows (every thread of the block takes part: barriers below)
  for (int c0 = 0; c0 < g.C; c0 += 64) {
    const int cn = min(64, g.C - c0);
    if (live)
      for (int j = 0; j < cn; ++j) tile[t][j] = feat[((size_t)bn * g.C + c0 + j) * HW + hw];
    __syncthreads();
    for (int r = 0; r < 64 && p0 + r < P; ++r)
      if (t < cn) featT[(size_t)(p0 + r) * g.C + c0 + t] = tile[r][t];
    __syncthreads();
  }
  if (!live) return;

  // softmax over D (lss_submodule.py:221: F.softmax(depth_logit, dim=1))
  const float* __restrict__ lg = logit + (size_t)bn * g.D * HW + hw;
  float m = -INFINITY;
  for (int d = 0; d < g.D; ++d) m = fmaxf(m, lg[(size_t)d * HW]);
  float s = 0.f;
  for (int d = 0; d < g.D; ++d) s += expf(lg[(size_t)d * HW] - m);
  const float rs = 1.f / s;

  // get_geometry (heter_encoders.py:119-146): undo post-transformation, un-project, combine = rots . intrins^-1, + trans
  float pinv[9], iinv[9], comb[9];
  lss_inv3(post_rots + (size_t)bn * 9, pinv);
  lss_inv3(intrins + (size_t)bn * 9, iinv);
  const float* __restrict__ R = rots + (size_t)bn * 9;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) comb[i * 3 + j] = R[i * 3] * iinv[j] + R[i * 3 + 1] * iinv[3 + j] + R[i * 3 + 2] * iinv[6 + j];
  const float pt0 = post_trans[bn * 3], pt1 = post_trans[bn * 3 + 1], pt2 = post_trans[bn * 3 + 2];
  const float tr0 = trans[bn * 3], tr1 = trans[bn * 3 + 1], tr2 = trans[bn * 3 + 2];
  const int b = bn / g.N;
  const unsigned ncells = (unsigned)g.B * g.nz * g.ny * g.nx;
  for (int d = 0; d < g.D; ++d) {
    const size_t pt = ((size_t)bn * g.D + d) * HW + hw;
    prob[pt] = expf(lg[(size_t)d * HW] - m) * rs;
    const float* __restrict__ f = frustum + ((size_t)d * HW + hw) * 3;
    const float a0 = f[0] - pt0, a1 = f[1] - pt1, a2 = f[2] - pt2;
    const float q0 = pinv[0] * a0 + pinv[1] * a1 + pinv[2] * a2;
    const float q1 = pinv[3] * a0 + pinv[4] * a1 + pinv[5] * a2;
    const float q2 = pinv[6] * a0 + pinv[7] * a1 + pinv[8] * a2;
    const float u0 = q0 * q2, u1 = q1 * q2, u2 = q2;
    const float w0 = comb[0] * u0 + comb[1] * u1 + comb[2] * u2 + tr0;
    const float w1 = comb[3] * u0 + comb[4] * u1 + comb[5] * u2 + tr1;
    const float w2 = comb[6] * u0 + comb[7] * u1 + comb[8] * u2 + tr2;
    // voxel_pooling (heter_encoders.py:161-205): truncated cell coordinates, kept inside nx, rank = x (ny nz B) + y (nz B) + z B + b
    const int ix = lss_cell(w0, g.lo[0], g.dx[0], g.nx), iy = lss_cell(w1, g.lo[1], g.dx[1], g.ny), iz = lss_cell(w2, g.lo[2], g.dx[2], g.nz);
    const bool in = ix >= 0 && iy >= 0 && iz >= 0;
    const int rank = in ? ((ix * g.ny + iy) * g.nz + iz) * g.B + b : -1;
    key[pt] = in ? (unsigned)rank : ncells;
    val[pt] = (int)pt;
    if (cell != nullptr) cell[pt] = rank;
  }
}

// first index in keys[lo, hi) that is >= k
__device__ __forceinline__ int lss_lower_bound(const unsigned* __restrict__ keys, int lo, int hi, unsigned k) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

constexpr int kLssTx = 64, kLssCh = 128, kLssPad = kLssTx + 1;

// grid = (ceil(nx / 64), ny, B nz), block 256. out [B][nz C][ny][nx], channel z C + c (torch.cat(final.unbind(2), 1))
__global__ __launch_bounds__(256) void lss_splat_kernel(const unsigned* __restrict__ skey, const int* __restrict__ sval, int npts,
                                                        const float* __restrict__ prob, const float* __restrict__ featT,
                                                        const LssGeom g, float* __restrict__ out) {
  __shared__ float tile[kLssCh * kLssPad];
  __shared__ int lo_s[kLssTx], hi_s[kLssTx];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int x0 = blockIdx.x * kLssTx, y = blockIdx.y, b = blockIdx.z % g.B, z = blockIdx.z / g.B;
  const int HW = g.fH * g.fW, DHW = g.D * HW;
  if (tid < kLssTx) {
    const int x = x0 + tid;
    int lo = 0, hi = 0;
    if (x < g.nx) {
      const unsigned r = (unsigned)(((x * g.ny + y) * g.nz + z) * g.B + b);
      lo = lss_lower_bound(skey, 0, npts, r);
      hi = lss_lower_bound(skey, lo, npts, r + 1);
    }
    lo_s[tid] = lo;
    hi_s[tid] = hi;
  }
  __syncthreads();
  const size_t plane = (size_t)g.ny * g.nx;
  float* __restrict__ ob = out + ((size_t)b * g.nz * g.C + (size_t)z * g.C) * plane + (size_t)y * g.nx;
  for (int c0 = 0; c0 < g.C; c0 += kLssCh) {
    const int ca = c0 + lane, cb = c0 + 64 + lane;
    const bool va = ca < g.C, vb = cb < g.C;
    for (int cx = wv; cx < kLssTx; cx += 4) {
      const int k0 = lo_s[cx], k1 = hi_s[cx];
      float s0 = 0.f, s1 = 0.f;
      int k = k0;
      for (; k + 4 <= k1; k += 4) {   // four independent row reads in flight per wave
        int pt[4];
        float pr[4], fa[4], fb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) pt[j] = sval[k + j];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int bn = pt[j] / DHW, hw = (pt[j] - bn * DHW) % HW;
          const float* __restrict__ row = featT + ((size_t)bn * HW + hw) * g.C;
          pr[j] = prob[pt[j]];
          fa[j] = va ? row[ca] : 0.f;
          fb[j] = vb ? row[cb] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s0 = fmaf(pr[j], fa[j], s0);
          s1 = fmaf(pr[j], fb[j], s1);
        }
      }
      for (; k < k1; ++k) {
        const int p = sval[k];
        const int bn = p / DHW, hw = (p - bn * DHW) % HW;
        const float* __restrict__ row = featT + ((size_t)bn * HW + hw) * g.C;
        const float pr = prob[p];
        if (va) s0 = fmaf(pr, row[ca], s0);
        if (vb) s1 = fmaf(pr, row[cb], s1);
      }
      tile[lane * kLssPad + cx] = s0;
      tile[(64 + lane) * kLssPad + cx] = s1;
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x < g.nx)
      for (int c = wv; c < kLssCh && c0 + c < g.C; c += 4) ob[(size_t)(c0 + c) * plane + x] = tile[c * kLssPad + lane];
    __syncthreads();
  }
}

struct LssWs {
  size_t featT, prob, key, val, skey, sval, temp, temp_bytes, total;
};
inline LssWs lss_ws(long long npts, long long pixels, int C, int sort_bits) {
  LssWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  const size_t n = (size_t)(npts > 0 ? npts : 1);
  w.featT = take((size_t)pixels * C * 4);
  w.prob = take(n * 4);
  w.key = take(n * 4); w.val = take(n * 4);
  w.skey = take(n * 4); w.sval = take(n * 4);
  size_t t1 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t1, (unsigned*)nullptr, (unsigned*)nullptr, (int*)nullptr, (int*)nullptr, n, 0, sort_bits, (hipStream_t)0);
  w.temp_bytes = t1 + 256;
  w.temp = take(w.temp_bytes);
  w.total = off;
  return w;
}

// depth targets of depth_supervision (lss_submodule.py:172-190 get_gt_depth_dist in eval mode, camera_utils.py:138-181 bin_depths):
// clamp_max(d_max) on channel 3, bin index (UD / LID, fp32 operations in the reference's order), picked at downsample // 2 ::
// downsample; mask = index inside [0, num_bins) and finite; out-of-range indices clamped, then truncated to int64
struct LssDepthArgs {
  const float* imgs; long long* idx; unsigned char* mask;
  int BN, Cimg, H, W, ds, oH, oW, mode, nb;
  float dmin, dmax, bin;
};
__global__ __launch_bounds__(256) void lss_depth_target_kernel(const LssDepthArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.BN * a.oH * a.oW) return;
  const int j = (int)(i % a.oW), r = (int)((i / a.oW) % a.oH), bn = (int)(i / ((long long)a.oW * a.oH));
  const int sy = a.ds / 2 + r * a.ds, sx = a.ds / 2 + j * a.ds;
  float v = a.imgs[(((size_t)bn * a.Cimg + 3) * a.H + sy) * a.W + sx];
  if (v > a.dmax) v = a.dmax;   // clamp_max_: NaN stays NaN
  float f;
  if (a.mode == 0) f = __fdiv_rn(__fsub_rn(v, a.dmin), a.bin);   // UD
  else f = __fadd_rn(-0.5f, __fmul_rn(0.5f, __fsqrt_rn(__fadd_rn(1.f, __fdiv_rn(__fmul_rn(8.f, __fsub_rn(v, a.dmin)), a.bin)))));   // LID
  const bool finite = isfinite(f);
  const bool ok = f >= 0.f && f < (float)a.nb && finite;
  if (f < 0.f) f = 0.f;
  if (f >= (float)a.nb) f = (float)(a.nb - 1);
  if (!isfinite(f)) f = (float)(a.nb - 1);
  a.idx[i] = (long long)f;
  if (a.mask != nullptr) a.mask[i] = ok ? 1 : 0;
}

// nn.MaxPool2d(kernel_size=3, stride=2, padding=1) (the ResNet stem, torchvision resnet.py), NaN propagating as torch does
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H, int W,
                                                           int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % Wo), oy = (int)((i / Wo) % Ho);
  const long long nc = i / ((long long)Wo * Ho);
  const float* __restrict__ xp = x + (size_t)nc * H * W;
  float m = -INFINITY;
  for (int dy = 0; dy < 3; ++dy) {
    const int iy = oy * 2 - 1 + dy;
    if (iy < 0 || iy >= H) continue;
    for (int dx = 0; dx < 3; ++dx) {
      const int ix = ox * 2 - 1 + dx;
      if (ix < 0 || ix >= W) continue;
      const float v = xp[(size_t)iy * W + ix];
      if (v > m || isnan(v)) m = v;
    }
  }
  y[i] = m;
}

// ---- backward of the lift-splat ---------------------------------------------------------------------------------------------------
constexpr int kLssBwdPx = 32, kLssBwdPitch = kLssBwdPx + 1, kLssBwdCh = 128, kLssBwdMaxD = 256;

// grad_out [B nz][C][plane] -> gT [B nz][plane][C], plane = ny nx.  grid (ceil(plane / 64), ceil(C / 64), B nz), block 256
__global__ __launch_bounds__(256) void lss_grad_rows_kernel(const float* __restrict__ g, float* __restrict__ gT, int C, int plane) {
  __shared__ float tile[64][65];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int p0 = blockIdx.x * 64, c0 = blockIdx.y * 64;
  const size_t bz = blockIdx.z;
  const int cn = min(64, C - c0), pn = min(64, plane - p0);
  for (int c = wv; c < cn; c += 4)
    if (lane < pn) tile[c][lane] = g[(bz * C + c0 + c) * plane + p0 + lane];
  __syncthreads();
  for (int r = wv; r < pn; r += 4)
    if (lane < cn) gT[(bz * plane + p0 + r) * C + c0 + lane] = tile[lane][r];
}

struct LssBwdArgs {
  const float *gT, *prob, *featT;   // [B][nz][ny][nx][C], [BN][D][HW], [BN][HW][C]
  const int* cell;                  // [BN][D][HW]: the forward's rank of every frustum point, -1 outside the grid
  float *dlogit, *dfeat;            // [BN][D][HW], [BN][C][HW]
  int B, nx, ny, nz, D, HW, C;
};

// one point of the walk: dprob of bin `d` (lane 0 keeps it in LDS, summed over the channel chunks), dfeat accumulated in registers
#define GC_LSS_BWD_POINT(GA, GB, PR, DD)                                        \
  do {                                                                          \
    const float dp__ = wave_total(fmaf((GA), fa, (GB) * fb));                   \
    acc_a = fmaf((PR), (GA), acc_a);                                            \
    acc_b = fmaf((PR), (GB), acc_b);                                            \
    if (lane == 0) {                                                            \
      float* q__ = dl + (DD) * kLssBwdPitch + px;                               \
      *q__ = c0 == 0 ? dp__ : *q__ + dp__;                                      \
    }                                                                           \
  } while (0)

// grid (ceil(HW / 32), BN), block 256, dynamic LDS (D + 128) * 33 floats: the workgroup owns 32 consecutive pixels of one camera,
// wave w the pixels w, w + 4, ...
__global__ __launch_bounds__(256) void lss_splat_bwd_kernel(const LssBwdArgs a) {
  extern __shared__ float lss_bwd_smem[];
  float* dl = lss_bwd_smem;                                // [D][33]: dprob, then d_depth_logit
  float* ft = lss_bwd_smem + (size_t)a.D * kLssBwdPitch;   // [128][33]: d_feat of one channel chunk
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bn = blockIdx.y, hw0 = blockIdx.x * kLssBwdPx;
  const int D = a.D, HW = a.HW, C = a.C;
  const int npx = min(kLssBwdPx, HW - hw0);
  for (int c0 = 0; c0 < C; c0 += kLssBwdCh) {
    const int ca = c0 + lane, cb = ca + 64;
    const bool va = ca < C, vb = cb < C;
    for (int px = wv; px < npx; px += 4) {
      const int hw = hw0 + px;
      const float* __restrict__ frow = a.featT + ((size_t)bn * HW + hw) * C;
      const float fa = va ? frow[ca] : 0.f, fb = vb ? frow[cb] : 0.f;
      float acc_a = 0.f, acc_b = 0.f;
      for (int d0 = 0; d0 < D; d0 += 64) {
        const int dn = min(64, D - d0);
        // lane d: probability and gradient row of point (bn, d0 + d, hw)
        float pl = 0.f;
        int rl = -1;
        if (lane < dn) {
          const size_t pt = ((size_t)bn * D + d0 + lane) * HW + hw;
          pl = a.prob[pt];
          const int r = a.cell[pt];
          if (r >= 0) {   // rank = ((x ny + y) nz + z) B + b -> row ((b nz + z) ny + y) nx + x
            const int b = r % a.B, t = r / a.B, iz = t % a.nz, u = t / a.nz, iy = u % a.ny, ix = u / a.ny;
            rl = ((b * a.nz + iz) * a.ny + iy) * a.nx + ix;
          }
        }
        int d = 0;
        for (; d + 4 <= dn; d += 4) {   // four independent row reads in flight per wave
          int r[4];
          float pr[4], ga[4], gb[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            r[j] = __builtin_amdgcn_readlane(rl, d + j);
            pr[j] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pl), d + j));
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float* __restrict__ row = a.gT + (size_t)max(r[j], 0) * C;
            ga[j] = (va && r[j] >= 0) ? row[ca] : 0.f;
            gb[j] = (vb && r[j] >= 0) ? row[cb] : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) GC_LSS_BWD_POINT(ga[j], gb[j], pr[j], d0 + d + j);
        }
        for (; d < dn; ++d) {
          const int r = __builtin_amdgcn_readlane(rl, d);
          const float pr = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pl), d));
          const float* __restrict__ row = a.gT + (size_t)max(r, 0) * C;
          const float ga = (va && r >= 0) ? row[ca] : 0.f, gb = (vb && r >= 0) ? row[cb] : 0.f;
          GC_LSS_BWD_POINT(ga, gb, pr, d0 + d);
        }
      }
      ft[lane * kLssBwdPitch + px] = acc_a;
      ft[(64 + lane) * kLssBwdPitch + px] = acc_b;
    }
    __syncthreads();
    const int cn = min(kLssBwdCh, C - c0);
    for (int i = tid; i < cn * kLssBwdPx; i += 256) {   // stores run along hw
      const int c = i / kLssBwdPx, px = i % kLssBwdPx;
      if (px < npx) a.dfeat[((size_t)bn * C + c0 + c) * HW + hw0 + px] = ft[c * kLssBwdPitch + px];
    }
    __syncthreads();
  }
  // softmax backward: dlogit_d = prob_d (dprob_d - sum_d' prob_d' dprob_d')
  for (int px = wv; px < npx; px += 4) {
    const float* __restrict__ pp = a.prob + (size_t)bn * D * HW + hw0 + px;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(pp[(size_t)d * HW], dl[d * kLssBwdPitch + px], s);
    s = wave_total(s);
    for (int d = lane; d < D; d += 64) dl[d * kLssBwdPitch + px] = pp[(size_t)d * HW] * (dl[d * kLssBwdPitch + px] - s);
  }
  __syncthreads();
  for (int i = tid; i < D * kLssBwdPx; i += 256) {
    const int d = i / kLssBwdPx, px = i % kLssBwdPx;
    if (px < npx) a.dlogit[((size_t)bn * D + d) * HW + hw0 + px] = dl[d * kLssBwdPitch + px];
  }
}
#undef GC_LSS_BWD_POINT

// backward of maxpool3x3s2_kernel, input-driven: an input pixel lies in at most four windows; each window's arg-max is recomputed
// with the forward's rule (first element in row-major window order for which v > m || isnan(v): torch's tie rule) and the dy of the
// windows this pixel wins are summed in (oy, ox) order.  No atomics.
__global__ __launch_bounds__(256) void maxpool3x3s2_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx,
                                                               long long total, int H, int W, int Ho, int Wo) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ix = (int)(i % W), iy = (int)((i / W) % H);
  const long long nc = i / ((long long)W * H);
  const float* __restrict__ xp = x + (size_t)nc * H * W;
  const float* __restrict__ dyp = dy + (size_t)nc * Ho * Wo;
  const int self = iy * W + ix;
  float s = 0.f;
  for (int oy = iy >> 1; oy <= ((iy + 1) >> 1); ++oy) {   // windows oy with 2 oy - 1 <= iy <= 2 oy + 1
    if (oy >= Ho) continue;
    for (int ox = ix >> 1; ox <= ((ix + 1) >> 1); ++ox) {
      if (ox >= Wo) continue;
      float m = -INFINITY;
      int am = -1;
      for (int ky = 0; ky < 3; ++ky) {
        const int jy = oy * 2 - 1 + ky;
        if (jy < 0 || jy >= H) continue;
        for (int kx = 0; kx < 3; ++kx) {
          const int jx = ox * 2 - 1 + kx;
          if (jx < 0 || jx >= W) continue;
          const float v = xp[(size_t)jy * W + jx];
          if (am < 0 || v > m || isnan(v)) { m = v; am = jy * W + jx; }
        }
      }
      if (am == self) s += dyp[(size_t)oy * Wo + ox];
    }
  }
  dx[i] = s;
}

// weight gradient of the 7x7 stride-2 pad-3 stem (Cin <= 3): dw [Cout][Cin 49] = dy [Cout x P] . patches [P x Cin 49], P = N Ho Wo.
// Split over P: workgroup (s, g) sums its pixel range for output channels 64 g .. 64 g + 63 (lane = channel, wave q = taps 40 q ..
// 40 q + 39, patches read from LDS as broadcast float4) into part [S][Cout][Cin 49]; stem7x7_wgrad_reduce_kernel adds the S
// partial sums in order.  No atomics.
constexpr int kStemTaps = 160, kStemPx = 32, kStemMaxSplit = 512;
struct StemWgradArgs {
  const float *dy, *x;
  float* part;
  int N, Cin, Hi, Wi, Cout, Ho, Wo, P, per;   // per: pixels per workgroup, a multiple of 32
};
__global__ __launch_bounds__(256) void stem7x7_wgrad_kernel(const StemWgradArgs a) {
  __shared__ __attribute__((aligned(16))) float xs[kStemPx][kStemTaps];
  __shared__ float dys[kStemPx][65];
  const int tid = threadIdx.x, co = tid & 63, q = tid >> 6;
  const int ntap = a.Cin * 49, HoWo = a.Ho * a.Wo, cog = blockIdx.y * 64;
  float acc[40];
#pragma unroll
  for (int j = 0; j < 40; ++j) acc[j] = 0.f;
  const long long pbeg = (long long)blockIdx.x * a.per;
  const int pend = (int)min((long long)a.P, pbeg + a.per);
  for (long long pl = pbeg; pl < pend; pl += kStemPx) {
    const int p0 = (int)pl, pn = min(kStemPx, pend - p0);
    for (int i = tid; i < kStemPx * kStemTaps; i += 256) {
      const int px = i / kStemTaps, t = i - px * kStemTaps;
      float v = 0.f;
      if (px < pn && t < ntap) {
        const int p = p0 + px, n = p / HoWo, rem = p - n * HoWo, oy = rem / a.Wo, ox = rem - oy * a.Wo;
        const int ci = t / 49, r = t - ci * 49, ky = r / 7, kx = r - ky * 7;
        const int jy = oy * 2 - 3 + ky, jx = ox * 2 - 3 + kx;
        if (jy >= 0 && jy < a.Hi && jx >= 0 && jx < a.Wi) v = a.x[(((size_t)n * a.Cin + ci) * a.Hi + jy) * a.Wi + jx];
      }
      xs[px][t] = v;
    }
    for (int i = tid; i < kStemPx * 64; i += 256) {
      const int px = i % kStemPx, c = i / kStemPx;
      float v = 0.f;
      if (px < pn) {
        const int p = p0 + px, n = p / HoWo, rem = p - n * HoWo;
        v = a.dy[((size_t)n * a.Cout + cog + c) * HoWo + rem];
      }
      dys[px][c] = v;
    }
    __syncthreads();
    for (int px = 0; px < pn; ++px) {
      const float g = dys[px][co];
      const float4* __restrict__ xr = reinterpret_cast<const float4*>(&xs[px][q * 40]);
#pragma unroll
      for (int j = 0; j < 10; ++j) {
        const float4 v = xr[j];
        acc[4 * j] = fmaf(g, v.x, acc[4 * j]);
        acc[4 * j + 1] = fmaf(g, v.y, acc[4 * j + 1]);
        acc[4 * j + 2] = fmaf(g, v.z, acc[4 * j + 2]);
        acc[4 * j + 3] = fmaf(g, v.w, acc[4 * j + 3]);
      }
    }
    __syncthreads();
  }
  float* __restrict__ o = a.part + ((size_t)blockIdx.x * a.Cout + cog + co) * ntap;
#pragma unroll
  for (int j = 0; j < 40; ++j)
    if (q * 40 + j < ntap) o[q * 40 + j] = acc[j];
}
__global__ __launch_bounds__(256) void stem7x7_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, int S, int total) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += part[(size_t)k * total + i];
  dw[i] = s;
}
inline int stem7x7_split(long long P) { return (int)std::min<long long>(kStemMaxSplit, (P + kStemPx - 1) / kStemPx); }

#pragma clang fp contract(fast)

}  // namespace gc
