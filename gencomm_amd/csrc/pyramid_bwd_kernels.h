// Training HEAL's PyramidFusion: the adjoints of pyramid_kernels.h (gfx950, wave64, fp32 in / out / accumulate).
//
//   gconv3x3 dgrad            the grouped 3x3's input gradient = the FORWARD tiles (gconv3x3_kernel / gconv3x3_mfma16_kernel) on dy with a
//                             transposed, tap-flipped pack (gconv3x3_pack_t_kernel), unit scale, zero shift, no ReLU; stride 2: dy is
//                             first spread onto the stride-1 grid (gconv3x3_spread_kernel), as the dense layers do
//   gconv3x3_wgrad_kernel     its weight gradient at 4 / 8 channels per group (VALU): workgroup = one group x one slab of 8 x 32 tiles
//   gconv3x3_wgrad16_kernel   the same at 16: every tap is a 16 x 16 product over a K of pixels on v_mfma_f32_16x16x4_f32
//   pyramid_score_bwd_kernel  the score head's backward (dx, per-workgroup partials of dw / db)
//   weightfuse_bwd_pixel_kernel / weightfuse_bwd_gather_kernel   the adjoint of warp_weightfuse_kernel in two passes
//   pyr_sum_rows_kernel       the ordered second pass of every parameter gradient
//
// No float atomics anywhere; every output element is written once; every parameter gradient is a sum of per-workgroup partials added in
// index order: two runs give the same bits.
#pragma once
#include <algorithm>

#include "common.h"
#include "fuse_cell.h"
#include "pyramid_kernels.h"

namespace gc {

// ------------------------------------------------------------------------------------------------------------------- ordered sums
// out[t] = sum_r part[r][t]; t < split goes to out0, the rest to out1 (the score head: dw | db).  Workgroup = 16 columns x 16 row lanes:
// lane l adds rows l, l + 16, l + 32 ... in ascending order (four independent chains of loads in flight), then the 16 lanes of a column
// meet in LDS and are added in lane order -- a fixed order whatever the grid, and 16 times shorter than one thread walking every row (the
// score head at the shipped level 0 has 2560 rows for 65 columns).
__global__ __launch_bounds__(256) void pyr_sum_rows_kernel(const float* __restrict__ part, float* __restrict__ out0, float* __restrict__ out1,
                                                           int rows, int total, int split) {
  __shared__ float s_sum[16][17];
  const int col = threadIdx.x & 15, lane = threadIdx.x >> 4;
  const int t = blockIdx.x * 16 + col;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (t < total) {
    int r = lane;
    for (; r + 48 < rows; r += 64) {
#pragma unroll
      for (int u = 0; u < 4; ++u) s[u] += part[(size_t)(r + 16 * u) * total + t];
    }
#pragma unroll
    for (int u = 0; u < 3; ++u)   // at most three rows are left for this lane
      if (r + 16 * u < rows) s[u] += part[(size_t)(r + 16 * u) * total + t];
  }
  s_sum[lane][col] = (s[0] + s[1]) + (s[2] + s[3]);
  __syncthreads();
  if (lane != 0 || t >= total) return;
  float v = 0.f;
#pragma unroll
  for (int l = 0; l < 16; ++l) v += s_sum[l][col];
  if (t < split) out0[t] = v;
  else out1[t - split] = v;
}

// ------------------------------------------------------------------------------------------------------------------- grouped 3x3: dgrad
// packed[((g cpg + co) 9 + tap) cpg + ci] = weight[g cpg + co][ci][8 - tap]: what gconv3x3_kernel needs to map dy's channels (co) to
// dx's (ci) with the taps flipped.
__global__ __launch_bounds__(256) void gconv3x3_pack_t_kernel(const float* __restrict__ w, float* __restrict__ wp, int cpg) {
  const int i = blockIdx.x * 256 + threadIdx.x, total = 32 * cpg * cpg * 9;
  if (i >= total) return;
  const int ci = i % cpg, tap = (i / cpg) % 9, co = (i / (cpg * 9)) % cpg, g = i / (cpg * cpg * 9);
  wp[i] = w[((size_t)(g * cpg + co) * cpg + ci) * 9 + (8 - tap)];
}

// up[m][2 oy][2 ox] = dy[m][oy][ox], zero elsewhere; up is [maps][H][W], dy [maps][Ho][Wo] with Ho = (H - 1) / 2 + 1.  Every element of
// up is written: no fill launch.
__global__ __launch_bounds__(256) void gconv3x3_spread_kernel(const float* __restrict__ dy, float* __restrict__ up, long long maps, int H, int W,
                                                              int Ho, int Wo) {
  const long long total = maps * H * W;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int ix = (int)(i % W), iy = (int)((i / W) % H);
    const long long m = i / ((long long)H * W);
    up[i] = ((ix | iy) & 1) ? 0.f : dy[(m * Ho + (iy >> 1)) * Wo + (ix >> 1)];
  }
}

// ------------------------------------------------------------------------------------------------------------------- grouped 3x3: wgrad
// dw[g cpg + co][ci][kh][kw] = sum_{n, oy, ox} dy[n][g cpg + co][oy][ox] x[n][g cpg + ci][s oy + kh - 1][s ox + kw - 1].
// Workgroup = one group x one slab of consecutive tiles (map-major); the x halo tile and the dy tile of the group go through LDS once per
// tile, the partial [9 cpg^2] goes to part[slab][g][.] in dw's own layout, and pyr_sum_rows_kernel adds the slabs in index order.
struct GconvWgradArgs {
  const float* x;     // [n][C][H][W]
  const float* dy;    // [n][C][Ho][Wo]
  float* part;        // [slabs][32][9 cpg cpg]
  int H, W, Ho, Wo, tiles_x, tiles_y, total_tiles, tps;   // tps: tiles per slab
};

template <int CPG, int TH, int S>
__device__ __forceinline__ void gconv_wgrad_stage(const GconvWgradArgs& a, int g, int tile, float* __restrict__ s_x, float* __restrict__ s_dy,
                                                  int dy_pitch_co, int dy_pitch_pix) {
  constexpr int TW = kGcTileW, IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3, PX = IW + 1;
  const int per_map = a.tiles_x * a.tiles_y;
  const int img = tile / per_map, t = tile - img * per_map, tile_y = t / a.tiles_x, tile_x = t - tile_y * a.tiles_x;
  const int iy0 = tile_y * TH * S - 1, ix0 = tile_x * TW * S - 1;
  const float* __restrict__ xg = a.x + ((size_t)img * 32 * CPG + (size_t)g * CPG) * a.H * a.W;
  for (int i = threadIdx.x; i < CPG * IH * IW; i += 256) {
    const int c = i / (IH * IW), r = (i / IW) % IH, col = i % IW;
    const int iy = iy0 + r, ix = ix0 + col;
    const bool in = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
    s_x[(c * IH + r) * PX + col] = in ? xg[((size_t)c * a.H + iy) * a.W + ix] : 0.f;
  }
  const float* __restrict__ dg = a.dy + ((size_t)img * 32 * CPG + (size_t)g * CPG) * a.Ho * a.Wo;
  for (int i = threadIdx.x; i < CPG * TH * TW; i += 256) {
    const int c = i / (TH * TW), pix = i % (TH * TW);
    const int oy = tile_y * TH + pix / TW, ox = tile_x * TW + pix % TW;
    const bool in = oy < a.Ho && ox < a.Wo;
    s_dy[c * dy_pitch_co + pix * dy_pitch_pix] = in ? dg[((size_t)c * a.Ho + oy) * a.Wo + ox] : 0.f;
  }
}

// cpg = 4 / 8: a thread owns one (ci, tap) and all cpg output channels for every PARTS-th pixel of the tile: one LDS read of x and one
// vector read of the pixel's cpg dy values (the same address across the (ci, tap) lanes of a pixel part: a broadcast) per cpg FMAs.
template <int CPG, int S>
__global__ __launch_bounds__(256) void gconv3x3_wgrad_kernel(const GconvWgradArgs a) {
  constexpr int TH = kGcTileH, TW = kGcTileW, IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3, PX = IW + 1;
  constexpr int PAIRS = 9 * CPG, PARTS = 256 / PAIRS, OUTS = 9 * CPG * CPG;
  __shared__ float s_x[CPG * IH * PX];
  __shared__ __attribute__((aligned(16))) float s_dy[TH * TW * CPG];   // [pixel][co]
  __shared__ float s_red[PARTS * PAIRS * CPG];
  const int slab = blockIdx.x, g = blockIdx.y;
  const int part = threadIdx.x / PAIRS, pair = threadIdx.x - part * PAIRS, ci = pair / 9, tap = pair - 9 * ci, kh = tap / 3, kw = tap - 3 * kh;
  const bool active = part < PARTS;
  float acc[CPG];
#pragma unroll
  for (int co = 0; co < CPG; ++co) acc[co] = 0.f;
  const int t_end = min(a.total_tiles, (slab + 1) * a.tps);
  for (int tile = slab * a.tps; tile < t_end; ++tile) {
    if (tile != slab * a.tps) __syncthreads();
    gconv_wgrad_stage<CPG, TH, S>(a, g, tile, s_x, s_dy, 1, CPG);
    __syncthreads();
    if (active) {
      const float* __restrict__ xr = s_x + (ci * IH + kh) * PX + kw;
      for (int pix = part; pix < TH * TW; pix += PARTS) {
        const float v = xr[(pix / TW) * S * PX + (pix % TW) * S];
#pragma unroll
        for (int co = 0; co < CPG; ++co) acc[co] = fmaf(s_dy[pix * CPG + co], v, acc[co]);
      }
    }
  }
  if (active) {
#pragma unroll
    for (int co = 0; co < CPG; ++co) s_red[(part * PAIRS + pair) * CPG + co] = acc[co];
  }
  __syncthreads();
  float* __restrict__ out = a.part + ((size_t)slab * 32 + g) * OUTS;
  for (int o = threadIdx.x; o < OUTS; o += 256) {   // o = (co cpg + ci) 9 + tap: dw's layout inside the group
    const int co = o / PAIRS, pr = o - co * PAIRS;
    float s = 0.f;
#pragma unroll
    for (int p = 0; p < PARTS; ++p) s += s_red[(p * PAIRS + pr) * CPG + co];
    out[o] = s;
  }
}

// cpg = 16: D[co][ci] += A[co][pixel] B[pixel][ci] per tap, K = 4 pixels a step.  A (dy) is read once per step and serves the nine taps;
// a wave owns TH / 4 rows of the tile and keeps the nine 16 x 16 accumulators (36 registers); the four waves meet in LDS at the end and
// are added in wave order.  Stride 2 halves the tile (4 x 32) to keep the halo tile of 16 channels inside 48 KiB.
template <int S>
__global__ __launch_bounds__(256) void gconv3x3_wgrad16_kernel(const GconvWgradArgs a) {
  constexpr int CPG = 16, TH = S == 1 ? 8 : 4, TW = kGcTileW, IH = (TH - 1) * S + 3, IW = (TW - 1) * S + 3, PX = IW + 1;
  constexpr int DYP = TH * TW + 4;                    // [co][pixel]: the pitch spreads lane (co, k) over 4 co + k banks
  constexpr int XF = CPG * IH * PX, STAGE = XF + CPG * DYP, RED = 4 * 9 * 256, OUTS = 9 * 256;
  __shared__ float smem[STAGE > RED ? STAGE : RED];
  float* s_x = smem;
  float* s_dy = smem + XF;
  const int slab = blockIdx.x, g = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n16 = lane & 15, r = lane >> 4;
  pyr_f32x4 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) acc[t] = pyr_f32x4{0.f, 0.f, 0.f, 0.f};
  const int t_end = min(a.total_tiles, (slab + 1) * a.tps);
  for (int tile = slab * a.tps; tile < t_end; ++tile) {
    if (tile != slab * a.tps) __syncthreads();
    gconv_wgrad_stage<CPG, TH, S>(a, g, tile, s_x, s_dy, DYP, 1);
    __syncthreads();
    constexpr int RPW = TH / 4;                       // rows per wave
#pragma unroll 2
    for (int ks = 0; ks < RPW * (TW / 4); ++ks) {
      const int row = wave * RPW + ks / (TW / 4), col = (ks % (TW / 4)) * 4 + r;     // this lane's pixel of the K-step
      const float av = s_dy[n16 * DYP + row * TW + col];                               // A[m = co = lane % 16][k = lane / 16]
      const float* __restrict__ xb = s_x + (n16 * IH + row * S) * PX + col * S;        // B[k = lane / 16][n = ci = lane % 16]
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, xb[(t / 3) * PX + (t % 3)], acc[t], 0, 0, 0);
    }
  }
  __syncthreads();   // the staged tiles are dead: the same LDS takes the four waves' accumulators
  // D: lane holds co = 4 (lane / 16) + v, ci = lane % 16
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) smem[wave * OUTS + ((4 * r + v) * 16 + n16) * 9 + t] = acc[t][v];
  __syncthreads();
  float* __restrict__ out = a.part + ((size_t)slab * 32 + g) * OUTS;
  for (int o = threadIdx.x; o < OUTS; o += 256) out[o] = ((smem[o] + smem[OUTS + o]) + smem[2 * OUTS + o]) + smem[3 * OUTS + o];
}

// the tiling of the weight gradient: (tile height, slabs, tiles per slab, tiles of a map in x / y)
struct GconvWgradPlan { int th, slabs, tps, tiles_x, tiles_y; long long total_tiles; };
inline GconvWgradPlan gconv3x3_wgrad_plan(int n, int cpg, int H, int W, int stride) {
  GconvWgradPlan p;
  p.th = (cpg == 16 && stride == 2) ? 4 : kGcTileH;
  const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  p.tiles_x = (Wo + kGcTileW - 1) / kGcTileW;
  p.tiles_y = (Ho + p.th - 1) / p.th;
  p.total_tiles = (long long)n * p.tiles_x * p.tiles_y;
  p.tps = (int)((p.total_tiles + 127) / 128);        // at most 128 slabs x 32 groups of workgroups
  p.slabs = (int)((p.total_tiles + p.tps - 1) / p.tps);
  return p;
}

// the host has checked cpg, stride, the sizes and the scratch
inline int gconv3x3_wgrad_enqueue(const float* x, const float* dy, float* dw, float* scratch, int n, int cpg, int H, int W, int stride, hipStream_t st) {
  const GconvWgradPlan p = gconv3x3_wgrad_plan(n, cpg, H, W, stride);
  GconvWgradArgs a{x, dy, scratch, H, W, (H - 1) / stride + 1, (W - 1) / stride + 1, p.tiles_x, p.tiles_y, (int)p.total_tiles, p.tps};
  const dim3 grid((unsigned)p.slabs, 32);
  if (cpg == 4) { if (stride == 1) gconv3x3_wgrad_kernel<4, 1><<<grid, 256, 0, st>>>(a); else gconv3x3_wgrad_kernel<4, 2><<<grid, 256, 0, st>>>(a); }
  else if (cpg == 8) { if (stride == 1) gconv3x3_wgrad_kernel<8, 1><<<grid, 256, 0, st>>>(a); else gconv3x3_wgrad_kernel<8, 2><<<grid, 256, 0, st>>>(a); }
  else if (stride == 1) gconv3x3_wgrad16_kernel<1><<<grid, 256, 0, st>>>(a);
  else gconv3x3_wgrad16_kernel<2><<<grid, 256, 0, st>>>(a);
  const int total = 32 * 9 * cpg * cpg;
  pyr_sum_rows_kernel<<<(total + 15) / 16, 256, 0, st>>>(scratch, dw, dw, p.slabs, total, total);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ------------------------------------------------------------------------------------------------------------------- score head
// d_pre = d_occ + d_score mask sg (1 - sg), sg = sigmoid(occ);  dx[c] = d_pre w[c];  dw[c] = sum d_pre x[c];  db = sum d_pre.
struct PyrScoreBwdArgs {
  const float* x;        // [n][C][H][W]
  const float* w;        // [C]
  const float* occ;      // [n][1][H][W]: the forward's output
  const int* rect;       // as the forward's (null: no mask)
  const float* d_occ;    // [n][1][H][W] or null
  const float* d_score;  // [n][1][H][W] or null
  float* dx;             // [n][C][H][W] or null
  float* part;           // [workgroups][C + 1] (dw | db) or null
  int C, H, W;
};

// The forward's workgroup: 64 pixels x 4 channel quarters, a wave = one quarter of all 64 pixels, so a channel's partial over the pixels
// is one butterfly inside the wave (a fixed order).
__global__ __launch_bounds__(256) void pyramid_score_bwd_kernel(const PyrScoreBwdArgs a) {
  const int HW = a.H * a.W, img = blockIdx.y;
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int pix_raw = blockIdx.x * 64 + pl;
  const bool live = pix_raw < HW;
  const int pix = live ? pix_raw : HW - 1;
  float dpre = 0.f;
  if (live) {
    const size_t at = (size_t)img * HW + pix;
    if (a.d_occ != nullptr) dpre = a.d_occ[at];
    if (a.d_score != nullptr) {
      float m = 1.f;
      if (a.rect != nullptr) {
        const int* __restrict__ r = a.rect + (size_t)img * 4;
        if (r[0] >= 0) {
          const int h = pix / a.W, w = pix - h * a.W;
          m = (h >= r[0] && h < r[1] && w >= r[2] && w < r[3]) ? 1.f : 0.f;
        }
      }
      const float sg = 1.0f / (1.0f + expf(-a.occ[at]));
      if (m != 0.f) dpre = fmaf(a.d_score[at], sg * (1.f - sg), dpre);
    }
  }
  const float* __restrict__ xp = a.x + (size_t)img * a.C * HW + pix;
  float* __restrict__ part = a.part != nullptr ? a.part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (a.C + 1) : nullptr;
  for (int c = cq; c < a.C; c += 4) {
    if (a.dx != nullptr && live) a.dx[((size_t)img * a.C + c) * HW + pix] = dpre * a.w[c];
    if (part != nullptr) {
      float v = live ? dpre * xp[(size_t)c * HW] : 0.f;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      if (pl == 0) part[c] = v;
    }
  }
  if (part != nullptr && cq == 0) {
    float v = dpre;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (pl == 0) part[a.C] = v;
  }
}

inline size_t pyramid_score_bwd_scratch_floats(int n, int C, int H, int W) { return (size_t)n * (((size_t)H * W + 63) / 64) * (C + 1); }

inline int pyramid_score_bwd_enqueue(PyrScoreBwdArgs a, float* dw, float* db, float* scratch, int n, hipStream_t st) {
  const unsigned bx = (unsigned)((a.H * a.W + 63) / 64);
  a.part = dw != nullptr ? scratch : nullptr;
  pyramid_score_bwd_kernel<<<dim3(bx, (unsigned)n), 256, 0, st>>>(a);
  if (dw != nullptr) pyr_sum_rows_kernel<<<(a.C + 1 + 15) / 16, 256, 0, st>>>(scratch, dw, db, (int)(bx * n), a.C + 1, a.C);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ------------------------------------------------------------------------------------------------------------------- weighted fuse
// out[b][c][p] = sum_j p_j(p) warp(x_j)[c][p], p = softmax_j of the warped scores with 0 -> -inf (warp_weightfuse_kernel).
//   pass 1 (per output pixel, the forward's cells and shares): dp_j = sum_c dout[c] warp(x_j)[c],  ds_j = p_j (dp_j - sum_k p_k dp_k)
//          -- exactly 0 where the warped score was 0 and where nobody scores -- written with p_j as two ego-frame maps [n][H][W]
//   pass 2 (per SOURCE pixel q of agent j, over the output pixels whose cell contains q):
//          dx[j][c][q] = sum wgt p_j(p) dout[b][c][p],   dscore[j][q] = sum wgt ds_j(p)
// The matches of pass 2 come from fuse_for_each_match for a tame transform (fuse_bwd_plan_kernel's test), from
// fuse_for_each_match_wide for any other, and are the pixel itself, weight 1, for an exact identity.
struct WeightFuseBwdArgs {
  const float* x;        // [n][C][H][W]
  const float* score;    // [n][1][H][W]
  const double* theta;   // [n][2][3]
  const int* scene_off;  // [B+1]
  const float* dout;     // [B][C][H][W]
  float* dx;             // [n][C][H][W]
  float* dscore;         // [n][1][H][W]
  float* pmap;           // scratch [n][H][W]
  float* dsmap;          // scratch [n][H][W]
  int C, H, W;
  int cchunk;            // pass 2: channels per blockIdx.z slice (a multiple of 8)
};

template <int N>
__device__ __forceinline__ void weightfuse_bwd_body(const WeightFuseBwdArgs& a, int b, int off, int pix_raw, int cq, int pl, float (&s_part)[8][4][64]) {
  const int H = a.H, W = a.W, HW = H * W;
  const bool live = pix_raw < HW;
  const int pix = live ? pix_raw : HW - 1;
  const int h = pix / W, w = pix - h * W;
  const double xb = fuse_base(w, W), yb = fuse_base(h, H);
  int idx[N][4];
  unsigned ok[N];
  float wt[N][4];
  float p[N];
  bool zero[N];
  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < N; ++j) {   // the forward's shares, statement for statement (weightfuse_body)
    fuse_cell(a.theta + (size_t)(off + j) * 6, xb, yb, H, W, idx[j], ok[j], wt[j]);
    const float s = fuse_sample(a.score + (size_t)(off + j) * HW, idx[j], ok[j], wt[j]);
    zero[j] = s == 0.f;
    p[j] = zero[j] ? -INFINITY : s;
    mx = fmaxf(mx, p[j]);
  }
  if (mx == -INFINITY) {
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
  float dp[N];
#pragma unroll
  for (int j = 0; j < N; ++j) dp[j] = 0.f;
  const float* __restrict__ xs = a.x + (size_t)off * a.C * HW;
  const float* __restrict__ gp = a.dout + (size_t)b * a.C * HW + pix;
  for (int c = cq; c < a.C; c += 4) {
    const float g = gp[(size_t)c * HW];
#pragma unroll
    for (int j = 0; j < N; ++j) dp[j] = fmaf(g, fuse_sample(xs + ((size_t)j * a.C + c) * HW, idx[j], ok[j], wt[j]), dp[j]);
  }
#pragma unroll
  for (int j = 0; j < N; ++j) s_part[j][cq][pl] = dp[j];
  __syncthreads();   // every thread of the workgroup gets here: dead pixels were clamped, not retired
  if (cq != 0 || !live) return;
  float sdot = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    dp[j] = (s_part[j][0][pl] + s_part[j][1][pl]) + (s_part[j][2][pl] + s_part[j][3][pl]);
    sdot = fmaf(p[j], dp[j], sdot);
  }
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const bool dead = zero[j] || mx == -INFINITY;
    a.pmap[(size_t)(off + j) * HW + pix] = dead ? 0.f : p[j];
    a.dsmap[(size_t)(off + j) * HW + pix] = dead ? 0.f : p[j] * (dp[j] - sdot);
  }
}

__global__ __launch_bounds__(256) void weightfuse_bwd_pixel_kernel(const WeightFuseBwdArgs a) {
  __shared__ float s_part[8][4][64];
  const int b = blockIdx.y;
  const int off = a.scene_off[b], N = a.scene_off[b + 1] - off;   // block-uniform
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int pix = blockIdx.x * 64 + pl;
  switch (N) {
    case 1: weightfuse_bwd_body<1>(a, b, off, pix, cq, pl, s_part); break;
    case 2: weightfuse_bwd_body<2>(a, b, off, pix, cq, pl, s_part); break;
    case 3: weightfuse_bwd_body<3>(a, b, off, pix, cq, pl, s_part); break;
    case 4: weightfuse_bwd_body<4>(a, b, off, pix, cq, pl, s_part); break;
    case 5: weightfuse_bwd_body<5>(a, b, off, pix, cq, pl, s_part); break;
    case 6: weightfuse_bwd_body<6>(a, b, off, pix, cq, pl, s_part); break;
    case 7: weightfuse_bwd_body<7>(a, b, off, pix, cq, pl, s_part); break;
    case 8: weightfuse_bwd_body<8>(a, b, off, pix, cq, pl, s_part); break;
    default: break;   // the module validates 1 <= N <= 8; the gather below then writes zeros for such a scene
  }
}

// 2: exact identity (its own pixel, weight 1: no interpolation error), 1: tame (fuse_bwd_plan_kernel's test), 0: anything else
__device__ __forceinline__ int weightfuse_match_mode(const double* __restrict__ th, int H, int W) {
  if (th[0] == 1.0 && th[1] == 0.0 && th[2] == 0.0 && th[3] == 0.0 && th[4] == 1.0 && th[5] == 0.0) return 2;
  const double m00 = th[0], m01 = th[1] * W / H, m10 = th[3] * H / W, m11 = th[4];
  const double det = m00 * m11 - m01 * m10;
  if (!(fabs(det) > 0.6)) return 0;
  const double r0 = (fabs(m11) + fabs(m01)) / fabs(det), r1 = (fabs(m10) + fabs(m00)) / fabs(det);
  return (r0 <= 1.5 && r1 <= 1.5) ? 1 : 0;
}

template <class F>
__device__ __forceinline__ void weightfuse_for_each_match(int mode, const double* __restrict__ th, int qx, int qy, int H, int W, F&& f) {
  if (mode == 2) f(qy * W + qx, 1.f);
  else if (mode == 1) fuse_for_each_match(th, qx, qy, H, W, f);
  else fuse_for_each_match_wide(th, qx, qy, H, W, f);
}

constexpr int kWfChunk = 8;   // channels accumulated at a time in pass 2

__global__ __launch_bounds__(128) void weightfuse_bwd_gather_kernel(const WeightFuseBwdArgs a, int B) {
  __shared__ int s_p[FUSE_KM][128];
  __shared__ float s_w[FUSE_KM][128];
  const int ag = blockIdx.y, tid = threadIdx.x;
  int b = 0;
  while (b + 1 < B && a.scene_off[b + 1] <= ag) ++b;
  const int scene_n = a.scene_off[b + 1] - a.scene_off[b];
  const int H = a.H, W = a.W, HW = H * W;
  const int q = blockIdx.x * 128 + tid;
  const bool live = q < HW && scene_n >= 1 && scene_n <= 8;   // a scene the pixel pass skipped: zeros
  const int qy = q < HW ? q / W : 0, qx = q < HW ? q - qy * W : 0;
  const double* __restrict__ th = a.theta + (size_t)ag * 6;
  const int mode = weightfuse_match_mode(th, H, W);
  const float* __restrict__ pm = a.pmap + (size_t)ag * HW;
  const float* __restrict__ dm = a.dsmap + (size_t)ag * HW;
  int cnt = 0;
  float dsc = 0.f;
  if (live) {
    weightfuse_for_each_match(mode, th, qx, qy, H, W, [&](int p, float wgt) {
      if (cnt < FUSE_KM) { s_p[cnt][tid] = p; s_w[cnt][tid] = wgt * pm[p]; }
      dsc = fmaf(wgt, dm[p], dsc);
      ++cnt;
    });
  }
  if (q < HW && blockIdx.z == 0) a.dscore[(size_t)ag * HW + q] = dsc;
  // More than FUSE_KM matches (a transform that shrinks the agent): the first FUSE_KM come from LDS, the rest are found again per channel
  // chunk -- slow, exact, never dropped
  const bool overflow = cnt > FUSE_KM;
  const int kept = min(cnt, FUSE_KM);
  const float* __restrict__ gp = a.dout + (size_t)b * a.C * HW;
  float* __restrict__ out = a.dx + (size_t)ag * a.C * HW + q;
  const int c_end = min(a.C, ((int)blockIdx.z + 1) * a.cchunk);
  for (int c0 = blockIdx.z * a.cchunk; c0 < c_end; c0 += kWfChunk) {
    float acc[kWfChunk];
#pragma unroll
    for (int i = 0; i < kWfChunk; ++i) acc[i] = 0.f;
    for (int k = 0; k < kept; ++k) {
      const int p = s_p[k][tid];
      const float wk = s_w[k][tid];
#pragma unroll
      for (int i = 0; i < kWfChunk; ++i)
        if (c0 + i < c_end) acc[i] = fmaf(wk, gp[(size_t)(c0 + i) * HW + p], acc[i]);
    }
    if (overflow) {
      int m = 0;
      weightfuse_for_each_match(mode, th, qx, qy, H, W, [&](int p, float wgt) {
        if (m++ >= FUSE_KM) {
          const float wk = wgt * pm[p];
#pragma unroll
          for (int i = 0; i < kWfChunk; ++i)
            if (c0 + i < c_end) acc[i] = fmaf(wk, gp[(size_t)(c0 + i) * HW + p], acc[i]);
        }
      });
    }
    if (q < HW) {
#pragma unroll
      for (int i = 0; i < kWfChunk; ++i)
        if (c0 + i < c_end) out[(size_t)(c0 + i) * HW] = acc[i];
    }
  }
}

inline size_t warp_weightfuse_bwd_scratch_floats(int n, int H, int W) { return (size_t)n * H * W * 2; }

inline int warp_weightfuse_bwd_enqueue(WeightFuseBwdArgs a, float* scratch, int B, int n, hipStream_t st) {
  const size_t HW = (size_t)a.H * a.W;
  a.pmap = scratch;
  a.dsmap = scratch + (size_t)n * HW;
  weightfuse_bwd_pixel_kernel<<<dim3((unsigned)((HW + 63) / 64), (unsigned)B), 256, 0, st>>>(a);
  // pass 2: about 1024 workgroups where the map alone gives fewer, at least 16 channels per slice
  const long long blocks = (long long)((HW + 127) / 128) * n;
  const int want = (int)std::min<long long>((1024 + blocks - 1) / blocks, (a.C + 15) / 16);
  a.cchunk = (((a.C + want - 1) / want) + kWfChunk - 1) / kWfChunk * kWfChunk;
  const int slices = (a.C + a.cchunk - 1) / a.cchunk;
  weightfuse_bwd_gather_kernel<<<dim3((unsigned)((HW + 127) / 128), (unsigned)n, (unsigned)slices), 128, 0, st>>>(a, B);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

}  // namespace gc
