// HEAL's PyramidFusion (opencood/models/fuse_modules/pyramid_fuse.py): the three kernels the library lacked for it (gfx950, wave64,
// fp32 in / out / accumulate; sampling positions in fp64 through fuse_cell.h).
//
//   gconv3x3_kernel        act(scale * conv3x3_grouped(x) + shift): conv2 of the ResNeXt Bottleneck (sub_modules/resblock.py:67-122 with
//                          groups = 32, width_per_group = 4): C = 32 cpg channels, cpg in {4, 8, 16}, padding 1, stride 1 | 2
//   pyramid_score_kernel   the single-supervision head of one level (pyramid_fuse.py:143-162): occ = Conv2d(C, 1, 1)(x),
//                          score = (sigmoid(occ) + 1e-4) * crop mask
//   warp_weightfuse_kernel weighted_fuse (pyramid_fuse.py:17-63): warp features and scores to the ego frame, 0 -> -inf, softmax over the
//                          agents, NaN -> 0, score-weighted sum; one gather pass, the warped [N, C, H, W] maps are never written
//
// No float atomics and a fixed summation order everywhere: two runs give the same bits.
#pragma once
#include <algorithm>

#include "common.h"
#include "fuse_cell.h"

namespace gc {

// ------------------------------------------------------------------------------------------------------------------- grouped 3x3
// Workgroup = 256 threads = an 8 x 32 tile of output pixels of ONE group of one map.  The group's input halo tile goes through LDS once
// per workgroup, a few channels at a time, and every output is written once.
//
// cpg = 4 / 8 (gconv3x3_kernel): plain VALU fmaf, a thread owns one pixel and all cpg output channels of the group.  Every LDS value read
// feeds cpg FMAs whose weight operand is wave-uniform (packed [group][ci][tap][co]: one scalar load of cpg consecutive floats per
// (ci, tap), the weight rides in an SGPR), so per output element the vector pipe issues 9 cpg FMAs + 9 LDS reads and nothing else.  Not a
// block-diagonal MFMA tile: v_mfma_f32_16x16x4_f32 wants M = 16 output channels, so a tile would carry 4 (2) groups of which each K slice
// feeds one -- 3/4 (1/2) of the matrix work would multiply structural zeros, and the fp32 matrix pipe is only twice the unpacked VALU rate.
//
// cpg = 16 (gconv3x3_mfma16_kernel): the exact-fp32 v_mfma_f32_16x16x4_f32, M = the group's 16 output channels, N = 16 pixels of a row,
// K = 144 = (ci, tap) in 36 steps.  The packed weight IS the A operand in lane order (step q: packed[64 q + lane]), so a lane keeps the
// whole matrix in 36 registers; a wave owns two rows of the tile = four 16-pixel segments, and per K-step issues four LDS reads (the B
// operands: lane = pixel lane % 16 of tap k = 4 q + lane / 16) and four matrix instructions.  The VALU form of this width was slower than
// torch's grouped convolution.
//
// Stride 2: the tile's input columns are stored de-interleaved (even columns, then odd ones), so the lanes of a wave read consecutive
// LDS words for every tap instead of every other one; each input element is still read from memory once per tile (plus the halo).
constexpr int kGcTileH = 8, kGcTileW = 32;

struct GconvArgs {
  const float* x;       // [n][C][H][W]
  const float* wp;      // packed [32][cpg][9][cpg]: wp[((g cpg + ci) 9 + tap) cpg + co] = weight[g cpg + co][ci][tap]
  const float* scale;   // [C]
  const float* shift;   // [C]
  float* y;             // [n][C][Ho][Wo]
  int H, W, Ho, Wo, tiles_x, relu;
};

__global__ __launch_bounds__(256) void gconv3x3_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int cpg) {
  const int i = blockIdx.x * 256 + threadIdx.x, total = 32 * cpg * cpg * 9;
  if (i >= total) return;
  const int co = i % cpg, tap = (i / cpg) % 9, ci = (i / (cpg * 9)) % cpg, g = i / (cpg * cpg * 9);
  wp[i] = w[((size_t)(g * cpg + co) * cpg + ci) * 9 + tap];
}

template <int CPG, int S>
__global__ __launch_bounds__(256) void gconv3x3_kernel(const GconvArgs a) {
  constexpr int CK = S == 1 ? (CPG < 8 ? CPG : 8) : 4;                 // channels staged at a time
  constexpr int IH = (kGcTileH - 1) * S + 3, IW = (kGcTileW - 1) * S + 3;
  constexpr int HALF = (IW + 1) / 2;                                   // stride 2: even columns [0, HALF), odd ones behind
  constexpr int PITCH = IW + 1;
  __shared__ float s_in[CK][IH][PITCH];
  const int g = blockIdx.y, img = blockIdx.z;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int tx = threadIdx.x & (kGcTileW - 1), ty = threadIdx.x / kGcTileW;
  const int oy = tile_y * kGcTileH + ty, ox = tile_x * kGcTileW + tx;
  const int iy0 = tile_y * kGcTileH * S - 1, ix0 = tile_x * kGcTileW * S - 1;
  const int H = a.H, W = a.W;
  const float* __restrict__ xg = a.x + ((size_t)img * 32 * CPG + (size_t)g * CPG) * H * W;
  const float* __restrict__ wg = a.wp + (size_t)g * CPG * 9 * CPG;
  float acc[CPG];
#pragma unroll
  for (int co = 0; co < CPG; ++co) acc[co] = 0.f;
  for (int c0 = 0; c0 < CPG; c0 += CK) {
    if (c0) __syncthreads();
    for (int i = threadIdx.x; i < CK * IH * IW; i += 256) {
      const int c = i / (IH * IW), r = (i / IW) % IH, col = i % IW;
      const int iy = iy0 + r, ix = ix0 + col;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float v = in ? xg[((size_t)(c0 + c) * H + iy) * W + ix] : 0.f;
      s_in[c][r][S == 1 ? col : (col & 1) * HALF + (col >> 1)] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int c = 0; c < CK; ++c) {
      const float* __restrict__ wc = wg + (size_t)(c0 + c) * 9 * CPG;
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
          const int col = S == 1 ? tx + dx : (dx & 1) * HALF + tx + (dx >> 1);
          const float v = s_in[c][ty * S + dy][col];
#pragma unroll
          for (int co = 0; co < CPG; ++co) acc[co] = fmaf(v, wc[(dy * 3 + dx) * CPG + co], acc[co]);
        }
    }
  }
  if (oy >= a.Ho || ox >= a.Wo) return;
  const size_t plane = (size_t)a.Ho * a.Wo;
  float* __restrict__ yp = a.y + ((size_t)img * 32 * CPG + (size_t)g * CPG) * plane + (size_t)oy * a.Wo + ox;
#pragma unroll
  for (int co = 0; co < CPG; ++co) {   // scale / shift are wave-uniform: read them all (scalar loads) before the first store
    const float v = fmaf(a.scale[g * CPG + co], acc[co], a.shift[g * CPG + co]);
    acc[co] = a.relu ? fmaxf(v, 0.f) : v;
  }
#pragma unroll
  for (int co = 0; co < CPG; ++co) yp[co * plane] = acc[co];
}

using pyr_f32x4 = __attribute__((ext_vector_type(4))) float;

template <int S>
__global__ __launch_bounds__(256) void gconv3x3_mfma16_kernel(const GconvArgs a) {
  constexpr int CPG = 16, CK = S == 1 ? 8 : 4, QC = CK * 9 / 4;        // channels staged at a time, K-steps per staged chunk
  constexpr int IH = (kGcTileH - 1) * S + 3, IW = (kGcTileW - 1) * S + 3;
  constexpr int HALF = (IW + 1) / 2, PITCH = IW + 1;
  __shared__ float s_in[CK * IH * PITCH];
  const int g = blockIdx.y, img = blockIdx.z;
  const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
  const int iy0 = tile_y * kGcTileH * S - 1, ix0 = tile_x * kGcTileW * S - 1;
  const int H = a.H, W = a.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, r = lane >> 4;
  const float* __restrict__ xg = a.x + ((size_t)img * 32 * CPG + (size_t)g * CPG) * H * W;
  const float* __restrict__ wg = a.wp + (size_t)g * CPG * 9 * CPG;
  float aw[36];     // A: W[m = lane % 16][k = 4 q + lane / 16] = packed[(4 q + lane / 16) 16 + lane % 16]
  int koff[36];     // B: where tap k = 4 q + lane / 16 of the tile's first pixel lies in the staged chunk
#pragma unroll
  for (int q = 0; q < 36; ++q) {
    aw[q] = wg[64 * q + lane];
    const int k = 4 * q + r, ci = k / 9, tap = k - 9 * ci, dy = tap / 3, dx = tap - 3 * dy;
    koff[q] = ((ci % CK) * IH + dy) * PITCH + (S == 1 ? dx : (dx & 1) * HALF + (dx >> 1));
  }
  int base[4];      // segment s of this wave: row 2 wave + s / 2, columns 16 (s % 2) ..
#pragma unroll
  for (int s = 0; s < 4; ++s) base[s] = (2 * wave + (s >> 1)) * S * PITCH + (s & 1) * 16 + n16;
  pyr_f32x4 acc[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) acc[s] = pyr_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int cc = 0; cc < CPG / CK; ++cc) {
    if (cc) __syncthreads();
    for (int i = threadIdx.x; i < CK * IH * IW; i += 256) {
      const int c = i / (IH * IW), row = (i / IW) % IH, col = i % IW;
      const int iy = iy0 + row, ix = ix0 + col;
      const bool in = iy >= 0 && iy < H && ix >= 0 && ix < W;
      const float v = in ? xg[((size_t)(cc * CK + c) * H + iy) * W + ix] : 0.f;
      s_in[(c * IH + row) * PITCH + (S == 1 ? col : (col & 1) * HALF + (col >> 1))] = v;
    }
    __syncthreads();
#pragma unroll
    for (int qq = 0; qq < QC; ++qq) {
      const int q = cc * QC + qq;
#pragma unroll
      for (int s = 0; s < 4; ++s) acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(aw[q], s_in[base[s] + koff[q]], acc[s], 0, 0, 0);
    }
  }
  // D: lane holds channels 4 (lane / 16) + v, v = 0..3, of pixel lane % 16 of each segment
  const size_t plane = (size_t)a.Ho * a.Wo;
  float sc[4], sh[4];
#pragma unroll
  for (int v = 0; v < 4; ++v) { sc[v] = a.scale[g * CPG + 4 * r + v]; sh[v] = a.shift[g * CPG + 4 * r + v]; }
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int oy = tile_y * kGcTileH + 2 * wave + (s >> 1), ox = tile_x * kGcTileW + (s & 1) * 16 + n16;
    if (oy >= a.Ho || ox >= a.Wo) continue;
    float* __restrict__ yp = a.y + ((size_t)img * 32 * CPG + (size_t)g * CPG + 4 * r) * plane + (size_t)oy * a.Wo + ox;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float o = fmaf(sc[v], acc[s][v], sh[v]);
      yp[v * plane] = a.relu ? fmaxf(o, 0.f) : o;
    }
  }
}

template <int CPG>
inline void gconv3x3_launch_cpg(const GconvArgs& a, int stride, dim3 grid, hipStream_t st) {
  if (stride == 1) gconv3x3_kernel<CPG, 1><<<grid, 256, 0, st>>>(a);
  else gconv3x3_kernel<CPG, 2><<<grid, 256, 0, st>>>(a);
}

// the host has checked cpg in {4, 8, 16}, stride in {1, 2} and the grid limits
inline int gconv3x3_enqueue(const float* x, const float* wp, const float* scale, const float* shift, float* y, int n, int cpg, int H, int W,
                            int stride, int relu, hipStream_t st) {
  GconvArgs a{x, wp, scale, shift, y, H, W, (H - 1) / stride + 1, (W - 1) / stride + 1, 0, relu};
  a.tiles_x = (a.Wo + kGcTileW - 1) / kGcTileW;
  const dim3 grid((unsigned)(a.tiles_x * ((a.Ho + kGcTileH - 1) / kGcTileH)), 32, (unsigned)n);
  if (cpg == 4) gconv3x3_launch_cpg<4>(a, stride, grid, st);
  else if (cpg == 8) gconv3x3_launch_cpg<8>(a, stride, grid, st);
  else if (stride == 1) gconv3x3_mfma16_kernel<1><<<grid, 256, 0, st>>>(a);
  else gconv3x3_mfma16_kernel<2><<<grid, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ------------------------------------------------------------------------------------------------------------------- score head
struct PyrScoreArgs {
  const float* x;      // [n][C][H][W]
  const float* w;      // [C]   (Conv2d(C, 1, 1).weight)
  const float* bias;   // [1]
  const int* rect;     // [n][4] = (h0, h1, w0, w1), score kept inside [h0, h1) x [w0, w1) and zeroed outside; h0 < 0: no mask for
                       // this agent; null: no mask at all
  float* occ;          // [n][1][H][W]
  float* score;        // [n][1][H][W]
  int C, H, W;
};

// Workgroup = 64 pixels x 4 channel quarters (the shape of warp_attfuse_kernel); the four partial dot products of a pixel meet in LDS and
// are added in a fixed order.
__global__ __launch_bounds__(256) void pyramid_score_kernel(const PyrScoreArgs a) {
  __shared__ float s_part[4][64];
  const int HW = a.H * a.W, img = blockIdx.y;
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int pix_raw = blockIdx.x * 64 + pl;
  const bool live = pix_raw < HW;
  const int pix = live ? pix_raw : HW - 1;
  const float* __restrict__ xp = a.x + (size_t)img * a.C * HW + pix;
  float s = 0.f;
  for (int c = cq; c < a.C; c += 4) s = fmaf(xp[(size_t)c * HW], a.w[c], s);
  s_part[cq][pl] = s;
  __syncthreads();
  if (cq != 0 || !live) return;
  const float o = ((s_part[0][pl] + s_part[1][pl]) + (s_part[2][pl] + s_part[3][pl])) + a.bias[0];
  float sc = 1.0f / (1.0f + expf(-o)) + 1e-4f;
  if (a.rect != nullptr) {
    const int* __restrict__ r = a.rect + (size_t)img * 4;
    if (r[0] >= 0) {
      const int h = pix / a.W, w = pix - h * a.W;
      sc *= (h >= r[0] && h < r[1] && w >= r[2] && w < r[3]) ? 1.f : 0.f;
    }
  }
  a.occ[(size_t)img * HW + pix] = o;
  a.score[(size_t)img * HW + pix] = sc;
}

inline int pyramid_score_enqueue(const PyrScoreArgs& a, int n, hipStream_t st) {
  pyramid_score_kernel<<<dim3((unsigned)((a.H * a.W + 63) / 64), (unsigned)n), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ------------------------------------------------------------------------------------------------------------------- weighted fuse
struct WeightFuseArgs {
  const float* x;        // [n][C][H][W]
  const float* score;    // [n][1][H][W]
  const double* theta;   // [n][2][3]
  const int* scene_off;  // [B+1]
  float* out;            // [B][C][H][W]
  int C, H, W;
  int cchunk;            // channels per blockIdx.z slice (a multiple of 4)
};

// One lane per (output pixel, channel quarter), as warp_attfuse_kernel; every lane computes the N cells and the N softmax shares of its
// pixel itself (one channel: cheaper than a trip through LDS), then makes ONE pass over its channels.  A small map has few 64-pixel
// blocks and many channels (the pyramid's level 2: 32 blocks x 256 channels), so the channels are also split over blockIdx.z; every
// output element is still computed by one lane with the same arithmetic, whatever the split.
template <int N>
__device__ __forceinline__ void weightfuse_body(const WeightFuseArgs& a, int b, int off, int pix_raw, int cq) {
  const int H = a.H, W = a.W, HW = H * W;
  const bool live = pix_raw < HW;
  const int pix = live ? pix_raw : HW - 1;
  const int h = pix / W, w = pix - h * W;
  const double xb = fuse_base(w, W), yb = fuse_base(h, H);
  int idx[N][4];
  unsigned ok[N];
  float wt[N][4];
  float p[N];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    fuse_cell(a.theta + (size_t)(off + j) * 6, xb, yb, H, W, idx[j], ok[j], wt[j]);
    const float s = fuse_sample(a.score + (size_t)(off + j) * HW, idx[j], ok[j], wt[j]);
    p[j] = s == 0.f ? -INFINITY : s;                       // scores_in_ego.masked_fill_(scores_in_ego == 0, -inf)
    mx = fmaxf(mx, p[j]);
  }
  if (mx == -INFINITY) {                                   // nobody scores here: softmax gives NaN, the reference replaces it by 0
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] = 0.f;
  } else {
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) { p[j] = expf(p[j] - mx); den += p[j]; }
    const float rden = 1.0f / den;
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] *= rden;
  }
  const float* __restrict__ xs = a.x + (size_t)off * a.C * HW;
  float* __restrict__ op = a.out + (size_t)b * a.C * HW + pix;
  const int c_end = min(a.C, ((int)blockIdx.z + 1) * a.cchunk);
  for (int c = blockIdx.z * a.cchunk + cq; c < c_end; c += 4) {
    float o = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) o = fmaf(p[j], fuse_sample(xs + ((size_t)j * a.C + c) * HW, idx[j], ok[j], wt[j]), o);
    if (live) op[(size_t)c * HW] = o;
  }
}

__global__ __launch_bounds__(256) void warp_weightfuse_kernel(const WeightFuseArgs a) {
  const int b = blockIdx.y;
  const int off = a.scene_off[b], N = a.scene_off[b + 1] - off;   // block-uniform
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int pix = blockIdx.x * 64 + pl;
  switch (N) {
    case 1: weightfuse_body<1>(a, b, off, pix, cq); break;
    case 2: weightfuse_body<2>(a, b, off, pix, cq); break;
    case 3: weightfuse_body<3>(a, b, off, pix, cq); break;
    case 4: weightfuse_body<4>(a, b, off, pix, cq); break;
    case 5: weightfuse_body<5>(a, b, off, pix, cq); break;
    case 6: weightfuse_body<6>(a, b, off, pix, cq); break;
    case 7: weightfuse_body<7>(a, b, off, pix, cq); break;
    case 8: weightfuse_body<8>(a, b, off, pix, cq); break;
    default: break;  // the module validates 1 <= N <= 8; otherwise the scene is left untouched
  }
}

inline int warp_weightfuse_enqueue(WeightFuseArgs a, int B, hipStream_t st) {
  // about 1024 workgroups where the map alone gives fewer, but at least 4 channels per lane (the cells cost N fp64 affine maps)
  const long long blocks = (long long)((a.H * a.W + 63) / 64) * B;
  const int want = (int)std::min<long long>((1024 + blocks - 1) / blocks, (a.C + 15) / 16);
  a.cchunk = (((a.C + want - 1) / want) + 3) / 4 * 4;
  const int slices = (a.C + a.cchunk - 1) / a.cchunk;
  warp_weightfuse_kernel<<<dim3((unsigned)((a.H * a.W + 63) / 64), (unsigned)B, (unsigned)slices), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

}  // namespace gc
