// The adjoint of STAMP's ConvNeXtBlock (convnext_kernels.h), dim 64 | 128, NCHW fp32, without ever forming a [pixels, 4 C] tensor:
//   d = dw7x7(x) + b_dw, xh = (d - mean) rstd, ln = xh w_ln + b_ln, u = ln W1^T + b1, h = GELU(u), z = h W2^T + b2, y = x + gamma z.
// The tape is x alone.  At most kCnxBwdLaunches = 6 launches (3 with dx_only), no float atomics, every output element written once:
//  1 cnx_bwd_prepare_kernel   W1T [C][4 C] = W1^T and W2G [4 C][C] = (gamma (.)rows W2)^T: with them the B operand of both backward
//                             products (du W1 and dy (gamma W2)) is a 16-byte load along k again, so cnx_mma serves all five products.
//  2 cnx_bwd_pixel_kernel     one 4 x 16 tile per workgroup, the forward's grid.  Depthwise stage and two-pass LayerNorm as the forward
//                             (the same statements: cnx_dw_stage is the forward's depthwise stage verbatim); xh goes to scratch as an NCHW map (the
//                             weight pass rebuilds ln = fma(xh, w_ln, b_ln) from it with the forward's own fma).  Per hidden chunk of 64:
//                             u = ln W1[chunk]^T and dh = dy W2G[chunk]^T (both cnx_mma<C, 1>), du = dh GELU'(u + b1) into the LDS image
//                             `du`, dln += du W1T[:, chunk]^T (cnx_mma<64, NT>, 16 / 32 accumulator registers that live across the chunks).
//                             LayerNorm adjoint in LDS, 4 threads per pixel (the thread re-reads the xh it wrote itself):
//                             dd = rstd (g - mean(g) - xh mean(g xh)), g = dln w_ln, written as an NCHW map; the tile's column sums of
//                             dln xh and dln are the per-tile partials of dnorm.weight / bias.
//  3 cnx_bwd_weight_kernel    grid (pixel slab, hidden chunk).  Per tile of its slab the workgroup stages ln and dy as [64][C] images,
//                             recomputes u and dh for its 64 hidden columns, and keeps h and du IN REGISTERS: in the C/D layout a lane
//                             holds (pixel 16 rt + 4 lk + e, column lr), which is exactly the A operand (m = column, k slot lk) of a
//                             product whose K axis is the pixel axis.  S^T[j][c] += h^T dy and dW1[j][c] += du^T ln take their B operand
//                             as dwords from the two images; db1 is a register sum.  One partial per (slab, chunk), no z recomputed:
//                             dW2 = gamma (.)rows S, dgamma = rowsum(W2 (.) S) + b2 sum(dy), db2 = gamma sum(dy).
//  4 cnx_bwd_dw_kernel        grid (pixel slab, 16-channel group): dx = dy + flipped-tap 7 x 7 over dd, with the forward's halo staging;
//                             the 49 tap gradients, the bias gradient and sum(dy) are register sums over the slab, combined over the 16
//                             threads of a channel by a fixed xor butterfly: one partial per slab and channel.
//  5 cnx_bwd_reduce_kernel    every fixed-order sum over partials (16 columns x 16 partial lanes per workgroup, lane l adds partials
//                             l, l + 16, .. in order, then the 16 lane sums in order): dW1, S (-> dW2 and a scratch copy), db1,
//                             dnorm.weight / bias over tiles, the depthwise gradients and sum(dy).
//  6 cnx_bwd_final_kernel     dgamma and db2 from the reduced S and sum(dy).
// Scratch per pixel: xh and dd (2 C floats) plus 2 C / 64 of per-tile partials; the slab partials do not grow with the map (at most
// kCnxBwdAutoSlabs slabs unless the caller asks for more).
// dx may be dy itself (launch 4 reads dy only at the pixel it writes, after launches 2 and 3 are done with it); it must not overlap x.
// Resources from the gfx950 cross-compile (-Rpass-analysis=kernel-resource-usage with the library's flags), no kernel with scratch:
//   kernel                     VGPRs   LDS bytes   workgroups (256 threads) per CU
//   cnx_bwd_prepare_kernel         8           0   8
//   cnx_bwd_pixel_kernel<64>     136      55 296   2 (LDS)
//   cnx_bwd_pixel_kernel<128>    175      88 064   1 (LDS: ln, dy and du images together; a second workgroup would need 80 KB or less)
//   cnx_bwd_weight_kernel<64>    132      36 864   3 (registers)
//   cnx_bwd_weight_kernel<128>   172      69 632   2
//   cnx_bwd_dw_kernel            246      31 744   2 (registers: 49 taps, 49 tap sums and the 28 prefetched halo values; 3 would spill)
//   cnx_bwd_reduce_kernel         14       1 088   8
//   cnx_bwd_final_kernel          10       1 024   8
// LDS operand patterns: the A-operand ds_read_b128 of all cnx_mma calls runs on row strides C + 8 and 72 (8 mod 64 dwords), the
// forward's conflict-free ones; the weight pass's B dwords sit at (16 rt + 4 lk + e)(C + 8) + 16 t + lr: ds_read_b32 is served in lane
// groups {0-31}, {32-63} on 32 banks and 4 (C + 8) = 0 mod 32, so lk and lk + 1 meet on the same banks: a 2-way conflict, 2 extra LDS
// cycles per read.  Left as it is: a read feeds one MFMA (32 cycles of matrix work), and the row stride that would remove it (4 mod 8
// floats) breaks the ds_read_b128 pattern of the A operand (tests/test_stamp_adapter_train.py restates both).
#pragma once
#include "convnext_kernels.h"

namespace gc {

constexpr int kCnxBwdLaunches = 6, kCnxBwdLaunchesDxOnly = 3;
constexpr int kCnxBwdAutoSlabs = 192;  // slabs at C = 64 when the caller passes 0, a third of it at C = 128 (fewer when there are fewer tiles):
                                       // 192 x 4 and 64 x 8 hidden chunks fill the 3 / 2 resident workgroups of the weight pass on 256 CUs once
constexpr int kCnxDwVals = 51;         // per channel: 49 taps, bias, sum(dy)

struct CnxBwdArgs {
  const float *x, *dy, *dw_w, *dw_b, *ln_w, *ln_b, *w1, *b1, *w2, *b2, *gamma;
  float* dx;
  float *g_dw_w, *g_dw_b, *g_ln_w, *g_ln_b, *g_w1, *g_b1, *g_w2, *g_b2, *g_gamma;
  float *w1t, *w2g, *xh, *dd, *p_ln, *p_w, *p_dw, *s_red, *sdy;   // workspace
  int n, H, W, tx, ty, tiles, slabs, tps, dx_only, vec;
};

struct CnxBwdPlan {
  long long w1t, w2g, xh, dd, p_ln, p_w, p_dw, s_red, sdy, total;   // float offsets
  int tx, ty, tiles, slabs, tps;
};

inline CnxBwdPlan cnx_bwd_plan(int n, int C, int H, int W, int dx_only, int slabs) {
  CnxBwdPlan p{};
  p.tx = (W + kCnxTileW - 1) / kCnxTileW;
  p.ty = (H + kCnxTileH - 1) / kCnxTileH;
  const long long tiles = (long long)n * p.tx * p.ty;
  p.tiles = (int)tiles;
  long long s = slabs > 0 ? slabs : (C == 64 ? kCnxBwdAutoSlabs : kCnxBwdAutoSlabs / 3);
  if (s > tiles) s = tiles;
  p.tps = (int)((tiles + s - 1) / s);
  p.slabs = (int)((tiles + p.tps - 1) / p.tps);   // no empty slab; the last one may be short
  const long long map = (long long)n * C * H * W, cc = 4ll * C * C;
  auto up4 = [](long long v) { return (v + 3) & ~3ll; };
  long long o = 0;
  p.w1t = o; o += cc;
  p.w2g = o; o += cc;
  p.xh = o; o += up4(map);
  p.dd = o; o += up4(map);
  p.p_ln = o; o += tiles * 2 * C;
  if (!dx_only) {
    p.p_w = o; o += (long long)p.slabs * (2 * cc + 4 * C);
    p.p_dw = o; o += up4((long long)p.slabs * C * kCnxDwVals);
    p.s_red = o; o += cc;
    p.sdy = o; o += C;
  }
  p.total = o;
  return p;
}

__device__ __forceinline__ void cnx_bwd_tile(const CnxBwdArgs& a, int tile, int* nidx, int* ty0, int* tx0) {
  const int per = a.tx * a.ty, r = tile % per, row = r / a.tx;
  *nidx = tile / per;
  *ty0 = row * kCnxTileH;
  *tx0 = (r - row * a.tx) * kCnxTileW;
}

// Staging an NCHW tile as a [pixel][channel] image: element i of C x 64 -> 8 consecutive pixels of a tile row x 4 channels per 32 lanes
// (32-byte runs in memory; in LDS the 8 pixels fall on 4 banks twice, the 4 channels beside them: a 2-way ds_write_b32 conflict, which
// costs nothing, where pixel-major lanes would be 8-way).
__device__ __forceinline__ int cnx_stage_p(int i) { return 16 * ((i >> 6) & 3) + 8 * ((i >> 5) & 1) + (i & 7); }
__device__ __forceinline__ int cnx_stage_c(int i) { return 4 * (i >> 8) + ((i >> 3) & 3); }

// ---- launch 1: the two weight re-layouts
__global__ __launch_bounds__(256) void cnx_bwd_prepare_kernel(const float* __restrict__ w1, const float* __restrict__ w2, const float* __restrict__ gamma,
                                                              float* __restrict__ w1t, float* __restrict__ w2g, int C) {
  const int i = blockIdx.x * 256 + threadIdx.x, C4 = 4 * C;
  if (i >= C * C4) return;
  {   // w1t[c][j] = w1[j][c]
    const int c = i / C4, j = i - c * C4;
    w1t[i] = w1[(size_t)j * C + c];
  }
  {   // w2g[j][c] = gamma[c] w2[c][j]
    const int j = i / C, c = i - j * C;
    const float v = w2[(size_t)c * C4 + j];
    w2g[i] = gamma != nullptr ? gamma[c] * v : v;
  }
}

// ---- the forward's depthwise stage (convnext_block_kernel's, statement for statement): leaves dw7x7(x) + b_dw in ln[pixel][ch]
template <int C>
__device__ __forceinline__ void cnx_dw_stage(const float* __restrict__ xn, const float* __restrict__ dw_w, const float* __restrict__ dw_b, float* ln,
                                             float* halo, int ty0, int tx0, int H, int W) {
  constexpr int LD = C + kCnxPad;
  constexpr int SLAB = kCnxSlab * kCnxHaloH * kCnxHaloW, NS = (SLAB + 255) / 256;
  const int tid = threadIdx.x;
  const size_t HW = (size_t)H * W;
  const int c_in = tid >> 4, prow = (tid >> 2) & 3, pcol = (tid & 3) * 4;
  float pre[NS];
  auto load_slab = [&](int cs) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = tid + 256 * k;
      const int c = i / (kCnxHaloH * kCnxHaloW), rem = i - c * (kCnxHaloH * kCnxHaloW);
      const int hy = rem / kCnxHaloW, hx = rem - hy * kCnxHaloW;
      const int gy = ty0 + hy - 3, gx = tx0 + hx - 3;
      float v = 0.f;
      if (i < SLAB && gy >= 0 && gy < H && gx >= 0 && gx < W) v = xn[(size_t)(cs + c) * HW + (size_t)gy * W + gx];
      pre[k] = v;
    }
  };
  auto store_slab = [&]() {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = tid + 256 * k;
      const int c = i / (kCnxHaloH * kCnxHaloW), rem = i - c * (kCnxHaloH * kCnxHaloW);
      const int hy = rem / kCnxHaloW, hx = rem - hy * kCnxHaloW;
      if (i < SLAB) halo[c * kCnxHaloCh + hy * kCnxHaloRow + hx] = pre[k];
    }
  };
  load_slab(0);
#pragma unroll 1
  for (int cs = 0; cs < C; cs += kCnxSlab) {
    store_slab();
    const int ch = cs + c_in;
    const float* __restrict__ wch = dw_w + ch * 49;
    float wv[49];
#pragma unroll
    for (int i = 0; i < 49; ++i) wv[i] = wch[i];
    const float bias = dw_b[ch];
    __syncthreads();
    if (cs + kCnxSlab < C) load_slab(cs + kCnxSlab);
    float o[4] = {bias, bias, bias, bias};
#pragma unroll
    for (int ky = 0; ky < 7; ++ky) {
      const float* hp = halo + c_in * kCnxHaloCh + (prow + ky) * kCnxHaloRow + pcol;
      const float4 h0 = *reinterpret_cast<const float4*>(hp), h1 = *reinterpret_cast<const float4*>(hp + 4);
      const float2 h2 = *reinterpret_cast<const float2*>(hp + 8);
      const float hv[10] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y};
#pragma unroll
      for (int kx = 0; kx < 7; ++kx)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(hv[j + kx], wv[ky * 7 + kx], o[j]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) ln[(prow * kCnxTileW + pcol + j) * LD + ch] = o[j];
    __syncthreads();   // the next slab overwrites the halo; after the last one `ln` is complete
  }
}

// ---- launch 2
template <int C>
__global__ __launch_bounds__(256, 2) void cnx_bwd_pixel_kernel(const CnxBwdArgs a) {
  constexpr int LD = C + kCnxPad, LH = kCnxChunk + kCnxPad, R = kCnxRows, NT = C / 64;
  static_assert(kCnxSlab * kCnxHaloCh <= R * LH, "the halo slab must fit the du image it aliases");
  extern __shared__ __align__(16) float cnx_smem[];
  float* ln = cnx_smem;          // [64][LD]: d, then ln, then dln
  float* dyi = ln + R * LD;      // [64][LD]: dy, then dln xh
  float* du = dyi + R * LD;      // [64][LH]; the halo slab during the depthwise stage

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int H = a.H, W = a.W;
  const int tx0 = blockIdx.x * kCnxTileW, ty0 = blockIdx.y * kCnxTileH;
  const size_t HW = (size_t)H * W;
  const size_t map0 = (size_t)blockIdx.z * C * HW;

  cnx_dw_stage<C>(a.x + map0, a.dw_w, a.dw_b, ln, du, ty0, tx0, H, W);

  // ---- LayerNorm over C in place, the forward's two passes; xh goes to scratch, rstd stays in a register
  const int prow_px = tid >> 2, q = tid & 3;
  const int pgy = ty0 + (prow_px >> 4), pgx = tx0 + (prow_px & 15);
  const bool pin = pgy < H && pgx < W;
  const size_t poff = map0 + (size_t)pgy * W + pgx;   // + c HW
  float rstd;
  {
    float* row = ln + prow_px * LD;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < C / 4; ++i) s += row[q + 4 * i];
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    const float mean = s * (1.0f / C);
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < C / 4; ++i) {
      const float d = row[q + 4 * i] - mean;
      v = fmaf(d, d, v);
    }
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    rstd = 1.0f / sqrtf(v * (1.0f / C) + 1e-6f);
#pragma unroll
    for (int i = 0; i < C / 4; ++i) {
      const int c = q + 4 * i;
      const float xh = (row[c] - mean) * rstd;
      if (pin) a.xh[poff + (size_t)c * HW] = xh;
      row[c] = fmaf(xh, a.ln_w[c], a.ln_b[c]);
    }
  }
  // ---- dy tile as a [pixel][channel] image, zero outside the map
  {
    const float* __restrict__ dyn = a.dy + map0;
#pragma unroll 4
    for (int i = tid; i < C * R; i += 256) {
      const int c = cnx_stage_c(i), p = cnx_stage_p(i);
      const int gy = ty0 + (p >> 4), gx = tx0 + (p & 15);
      dyi[p * LD + c] = (gy < H && gx < W) ? dyn[(size_t)c * HW + (size_t)gy * W + gx] : 0.f;
    }
  }
  __syncthreads();

  cnx_f32x4 acc[4][NT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = cnx_f32x4{0.f, 0.f, 0.f, 0.f};
  const int col0 = wave * (C / 4);
#pragma unroll 1
  for (int chunk = 0; chunk < 4 * C / kCnxChunk; ++chunk) {
    const int hcol = chunk * kCnxChunk + 16 * wave + lr;
    cnx_f32x4 a1[4][1], a2[4][1];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) a1[rt][0] = a2[rt][0] = cnx_f32x4{0.f, 0.f, 0.f, 0.f};
    cnx_mma<C, 1, LD>(ln + lr * LD + 4 * lk, a.w1 + (size_t)hcol * C + 4 * lk, C, a1);
    cnx_mma<C, 1, LD>(dyi + lr * LD + 4 * lk, a.w2g + (size_t)hcol * C + 4 * lk, C, a2);
    const float bias1 = a.b1[hcol];
    __syncthreads();   // every wave has read the previous chunk's du
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float g, d;
        gelu_and_grad_f(a1[rt][0][e] + bias1, &g, &d);
        du[(16 * rt + 4 * lk + e) * LH + 16 * wave + lr] = a2[rt][0][e] * d;
      }
    __syncthreads();
    cnx_mma<kCnxChunk, NT, LH>(du + lr * LH + 4 * lk, a.w1t + (size_t)(col0 + lr) * (4 * C) + chunk * kCnxChunk + 4 * lk, 4 * C, acc);
  }
  // after the last chunk's second barrier nobody reads ln or dyi any more: dln takes ln's place
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) ln[(16 * rt + 4 * lk + e) * LD + col0 + 16 * t + lr] = acc[rt][t][e];
  __syncthreads();

  // ---- LayerNorm adjoint, 4 threads per pixel as the forward's LayerNorm (the thread reads back the xh it wrote)
  {
    float* row = ln + prow_px * LD;
    float* prod = dyi + prow_px * LD;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < C / 4; ++i) {
      const int c = q + 4 * i;
      const float xh = pin ? a.xh[poff + (size_t)c * HW] : 0.f;
      const float g = row[c] * a.ln_w[c];
      s1 += g;
      s2 = fmaf(g, xh, s2);
    }
    s1 += __shfl_xor(s1, 1);
    s1 += __shfl_xor(s1, 2);
    s2 += __shfl_xor(s2, 1);
    s2 += __shfl_xor(s2, 2);
    const float m1 = s1 * (1.0f / C), m2 = s2 * (1.0f / C);
#pragma unroll
    for (int i = 0; i < C / 4; ++i) {
      const int c = q + 4 * i;
      const float xh = pin ? a.xh[poff + (size_t)c * HW] : 0.f;
      const float dl = row[c];
      const float g = dl * a.ln_w[c];
      if (pin) a.dd[poff + (size_t)c * HW] = rstd * ((g - m1) - xh * m2);
      prod[c] = dl * xh;
    }
  }
  __syncthreads();
  // ---- the tile's partials of dnorm.weight (column sums of dln xh) and dnorm.bias (of dln); rows outside the map hold zeros
  if (tid < 2 * C) {
    const int which = tid / C, c = tid - which * C;
    const float* col = (which ? ln : dyi) + c;
    float s = 0.f;
#pragma unroll 8
    for (int p = 0; p < R; ++p) s += col[p * LD];
    const size_t tile = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.p_ln[tile * (2 * C) + tid] = s;
  }
}

// ---- launch 3
template <int C>
__global__ __launch_bounds__(256, 2) void cnx_bwd_weight_kernel(const CnxBwdArgs a) {
  constexpr int LD = C + kCnxPad, R = kCnxRows, NC = C / 16;
  extern __shared__ __align__(16) float cnx_smem[];
  float* ln = cnx_smem;          // [64][LD]
  float* dyi = ln + R * LD;      // [64][LD]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  const int chunk = blockIdx.y, slab = blockIdx.x;
  const int hcol = chunk * kCnxChunk + 16 * wave + lr;
  const float bias1 = a.b1[hcol];
  const int t_begin = slab * a.tps, t_end = min(t_begin + a.tps, a.tiles);

  cnx_f32x4 accS[NC], accW[NC];
#pragma unroll
  for (int t = 0; t < NC; ++t) accS[t] = accW[t] = cnx_f32x4{0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f;
#pragma unroll 1
  for (int tile = t_begin; tile < t_end; ++tile) {
    int nidx, ty0, tx0;
    cnx_bwd_tile(a, tile, &nidx, &ty0, &tx0);
    const size_t map0 = (size_t)nidx * C * HW;
    __syncthreads();   // every wave has read the previous tile's images
    {
      const float* __restrict__ xhn = a.xh + map0;
      const float* __restrict__ dyn = a.dy + map0;
#pragma unroll 4
      for (int i = tid; i < C * R; i += 256) {
        const int c = cnx_stage_c(i), p = cnx_stage_p(i);
        const int gy = ty0 + (p >> 4), gx = tx0 + (p & 15);
        const bool in = gy < H && gx < W;
        const size_t off = (size_t)c * HW + (size_t)gy * W + gx;
        ln[p * LD + c] = in ? fmaf(xhn[off], a.ln_w[c], a.ln_b[c]) : 0.f;
        dyi[p * LD + c] = in ? dyn[off] : 0.f;
      }
    }
    __syncthreads();
    cnx_f32x4 a1[4][1], a2[4][1];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) a1[rt][0] = a2[rt][0] = cnx_f32x4{0.f, 0.f, 0.f, 0.f};
    cnx_mma<C, 1, LD>(ln + lr * LD + 4 * lk, a.w1 + (size_t)hcol * C + 4 * lk, C, a1);
    cnx_mma<C, 1, LD>(dyi + lr * LD + 4 * lk, a.w2g + (size_t)hcol * C + 4 * lk, C, a2);
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float g, d;
        gelu_and_grad_f(a1[rt][0][e] + bias1, &g, &d);
        const float duv = a2[rt][0][e] * d;
        a1[rt][0][e] = g;      // h
        a2[rt][0][e] = duv;    // du
        db1 += duv;
      }
    // K = the pixel axis: the lane's own h / du value is the A operand (m = its column lr, k slot lk = pixel 16 rt + 4 lk + e)
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int prow = (16 * rt + 4 * lk + e) * LD + lr;
#pragma unroll
        for (int t = 0; t < NC; ++t) {
          accS[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[rt][0][e], dyi[prow + 16 * t], accS[t], 0, 0, 0);
          accW[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[rt][0][e], ln[prow + 16 * t], accW[t], 0, 0, 0);
        }
      }
  }
  // one partial per (slab, chunk): S^T rows [4 C][C], dW1 [4 C][C], db1 [4 C]
  float* part = a.p_w + (size_t)slab * (8 * C * C + 4 * C);
#pragma unroll
  for (int t = 0; t < NC; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const size_t o = (size_t)(chunk * kCnxChunk + 16 * wave + 4 * lk + e) * C + 16 * t + lr;
      part[o] = accS[t][e];
      part[4 * C * C + o] = accW[t][e];
    }
  db1 += __shfl_xor(db1, 16);
  db1 += __shfl_xor(db1, 32);
  if (lk == 0) part[8 * C * C + hcol] = db1;
}

// ---- launch 4
__global__ __launch_bounds__(256, 2) void cnx_bwd_dw_kernel(const CnxBwdArgs a, int C) {
  __shared__ __align__(16) float halo_d[kCnxSlab * kCnxHaloCh];
  __shared__ __align__(16) float halo_x[kCnxSlab * kCnxHaloCh];
  constexpr int SLAB = kCnxSlab * kCnxHaloH * kCnxHaloW;
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W;
  const size_t HW = (size_t)H * W;
  const int slab = blockIdx.x, cs = blockIdx.y * kCnxSlab;
  const int c_in = tid >> 4, prow = (tid >> 2) & 3, pcol = (tid & 3) * 4;
  const int ch = cs + c_in;
  const bool full = !a.dx_only;
  float wv[49], gw[49];
#pragma unroll
  for (int i = 0; i < 49; ++i) {
    wv[i] = a.dw_w[ch * 49 + i];
    gw[i] = 0.f;
  }
  float gb = 0.f, sdy = 0.f;
  const int t_begin = slab * a.tps, t_end = min(t_begin + a.tps, a.tiles);
  // the halos of tile t + 1 are loaded into registers before the arithmetic of tile t, as the forward does with its channel slabs
  constexpr int NS = (SLAB + 255) / 256;
  float pd[NS], px[NS];
  auto load_halos = [&](int tile) {
    int nidx, ty0, tx0;
    cnx_bwd_tile(a, tile, &nidx, &ty0, &tx0);
    const size_t map0 = (size_t)nidx * C * HW + (size_t)cs * HW;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = tid + 256 * k;
      const int c = i / (kCnxHaloH * kCnxHaloW), rem = i - c * (kCnxHaloH * kCnxHaloW);
      const int hy = rem / kCnxHaloW, hx = rem - hy * kCnxHaloW;
      const int gy = ty0 + hy - 3, gx = tx0 + hx - 3;
      const bool in = i < SLAB && gy >= 0 && gy < H && gx >= 0 && gx < W;
      const size_t off = map0 + (size_t)c * HW + (size_t)gy * W + gx;
      pd[k] = in ? a.dd[off] : 0.f;
      px[k] = (in && full) ? a.x[off] : 0.f;
    }
  };
  auto store_halos = [&]() {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
      const int i = tid + 256 * k;
      const int c = i / (kCnxHaloH * kCnxHaloW), rem = i - c * (kCnxHaloH * kCnxHaloW);
      const int hy = rem / kCnxHaloW, hx = rem - hy * kCnxHaloW;
      if (i < SLAB) {
        halo_d[c * kCnxHaloCh + hy * kCnxHaloRow + hx] = pd[k];
        if (full) halo_x[c * kCnxHaloCh + hy * kCnxHaloRow + hx] = px[k];
      }
    }
  };
  load_halos(t_begin);
#pragma unroll 1
  for (int tile = t_begin; tile < t_end; ++tile) {
    int nidx, ty0, tx0;
    cnx_bwd_tile(a, tile, &nidx, &ty0, &tx0);
    const size_t map0 = (size_t)nidx * C * HW + (size_t)cs * HW;
    __syncthreads();   // every thread has read the previous tile's halos
    store_halos();
    __syncthreads();
    if (tile + 1 < t_end) load_halos(tile + 1);
    // dx = dy + sum_k w[k] dd[p + 3 - k]: halo offset (hy, hx) of the window carries tap (6 - hy, 6 - hx)
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int hy = 0; hy < 7; ++hy) {
      const float* hp = halo_d + c_in * kCnxHaloCh + (prow + hy) * kCnxHaloRow + pcol;
      const float4 h0 = *reinterpret_cast<const float4*>(hp), h1 = *reinterpret_cast<const float4*>(hp + 4);
      const float2 h2 = *reinterpret_cast<const float2*>(hp + 8);
      const float hv[10] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y};
#pragma unroll
      for (int hx = 0; hx < 7; ++hx)
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(hv[j + hx], wv[(6 - hy) * 7 + (6 - hx)], o[j]);
    }
    const int gy = ty0 + prow, gx = tx0 + pcol;
    float dyv[4] = {0.f, 0.f, 0.f, 0.f};
    if (gy < H && gx < W) {
      const size_t off = map0 + (size_t)c_in * HW + (size_t)gy * W + gx;
      if (a.vec) {
        const float4 d4 = *reinterpret_cast<const float4*>(a.dy + off);
        dyv[0] = d4.x; dyv[1] = d4.y; dyv[2] = d4.z; dyv[3] = d4.w;
        float4 r;
        r.x = d4.x + o[0]; r.y = d4.y + o[1]; r.z = d4.z + o[2]; r.w = d4.w + o[3];
        *reinterpret_cast<float4*>(a.dx + off) = r;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (gx + j < W) {
            dyv[j] = a.dy[off + j];
            a.dx[off + j] = dyv[j] + o[j];
          }
      }
    }
    if (full) {
      // gw[ky][kx] += dd[p] x[p + k - 3]; dd is zero outside the map
      const float* dc = halo_d + c_in * kCnxHaloCh + (prow + 3) * kCnxHaloRow + pcol + 3;
      const float ddc[4] = {dc[0], dc[1], dc[2], dc[3]};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        gb += ddc[j];
        sdy += dyv[j];
      }
#pragma unroll
      for (int ky = 0; ky < 7; ++ky) {
        const float* hp = halo_x + c_in * kCnxHaloCh + (prow + ky) * kCnxHaloRow + pcol;
        const float4 h0 = *reinterpret_cast<const float4*>(hp), h1 = *reinterpret_cast<const float4*>(hp + 4);
        const float2 h2 = *reinterpret_cast<const float2*>(hp + 8);
        const float hv[10] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y};
#pragma unroll
        for (int kx = 0; kx < 7; ++kx)
#pragma unroll
          for (int j = 0; j < 4; ++j) gw[ky * 7 + kx] = fmaf(ddc[j], hv[j + kx], gw[ky * 7 + kx]);
      }
    }
  }
  if (!full) return;
  // the 16 threads of a channel are 16 consecutive lanes: a fixed butterfly, then lane 0 of the 16 writes
  float* part = a.p_dw + ((size_t)slab * C + ch) * kCnxDwVals;
#pragma unroll
  for (int i = 0; i < kCnxDwVals; ++i) {
    float v = i < 49 ? gw[i < 49 ? i : 0] : (i == 49 ? gb : sdy);
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    if ((tid & 15) == 0) part[i] = v;
  }
}

// ---- launch 5: fixed-order sums over partials
enum { CNX_RED_PLAIN = 0, CNX_RED_S = 1, CNX_RED_DW = 2 };
struct CnxRedJob {
  const float* src;     // [parts][stride], the job's columns at src[0 .. count)
  float* dst;
  long long stride;
  int parts, count, mode, block0;   // block0: the job's first workgroup
};
struct CnxRedArgs {
  CnxRedJob job[6];
  int jobs, C;
  const float* gamma;
  float *g_w2, *g_dw_b, *sdy;
};

__global__ __launch_bounds__(256) void cnx_bwd_reduce_kernel(const CnxRedArgs r) {
  __shared__ float s[16][17];
  int ji = 0;
#pragma unroll
  for (int k = 1; k < 6; ++k)
    if (k < r.jobs && (int)blockIdx.x >= r.job[k].block0) ji = k;
  const CnxRedJob& jb = r.job[ji];
  const int tid = threadIdx.x, cl = tid & 15, pl = tid >> 4;
  const int col = ((int)blockIdx.x - jb.block0) * 16 + cl;
  float v = 0.f;
  if (col < jb.count)
    for (int p = pl; p < jb.parts; p += 16) v += jb.src[(size_t)p * jb.stride + col];
  s[pl][cl] = v;
  __syncthreads();
  if (pl != 0 || col >= jb.count) return;
  float t = s[0][cl];
#pragma unroll
  for (int k = 1; k < 16; ++k) t += s[k][cl];
  const int C = r.C;
  if (jb.mode == CNX_RED_PLAIN) {
    jb.dst[col] = t;
  } else if (jb.mode == CNX_RED_S) {   // col = j C + c of S^T: keep S^T for dgamma, dW2[c][j] = gamma[c] S[c][j]
    jb.dst[col] = t;
    const int j = col / C, c = col - j * C;
    r.g_w2[(size_t)c * (4 * C) + j] = r.gamma != nullptr ? r.gamma[c] * t : t;
  } else {                             // col = ch * 51 + i
    const int ch = col / kCnxDwVals, i = col - ch * kCnxDwVals;
    if (i < 49) jb.dst[ch * 49 + i] = t;
    else if (i == 49) r.g_dw_b[ch] = t;
    else r.sdy[ch] = t;
  }
}

// ---- launch 6: dgamma[c] = sum_j W2[c][j] S[c][j] + b2[c] sum(dy[c]), db2[c] = gamma[c] sum(dy[c]); one workgroup per channel, a fixed tree
__global__ __launch_bounds__(256) void cnx_bwd_final_kernel(const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ gamma,
                                                            const float* __restrict__ s_red, const float* __restrict__ sdy, float* g_gamma, float* g_b2,
                                                            int C) {
  __shared__ float s[256];
  const int c = blockIdx.x, tid = threadIdx.x;
  float t = 0.f;
  for (int j = tid; j < 4 * C; j += 256) t = fmaf(w2[(size_t)c * (4 * C) + j], s_red[(size_t)j * C + c], t);
  s[tid] = t;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if (tid < w) s[tid] += s[tid + w];
    __syncthreads();
  }
  if (tid != 0) return;
  if (g_gamma != nullptr) g_gamma[c] = fmaf(b2[c], sdy[c], s[0]);
  g_b2[c] = gamma != nullptr ? gamma[c] * sdy[c] : sdy[c];
}

inline int cnx_bwd_pixel_smem(int C) { return (int)((2 * kCnxRows * (C + kCnxPad) + kCnxRows * (kCnxChunk + kCnxPad)) * sizeof(float)); }   // 54 / 86 KB
inline int cnx_bwd_weight_smem(int C) { return (int)(2 * kCnxRows * (C + kCnxPad) * sizeof(float)); }                                       // 36 / 68 KB

// every launch of one block backward; the arguments have been checked by the caller (gencomm_convnext_block_bwd)
inline int convnext_block_bwd_launch(CnxBwdArgs a, int C, hipStream_t st) {
  static LdsAttrOnce attr[4];
  const int cc4 = 4 * C * C;
  GC_KLOG("cnx_bwd_prepare_kernel");
  cnx_bwd_prepare_kernel<<<(cc4 + 255) / 256, 256, 0, st>>>(a.w1, a.w2, a.gamma, a.w1t, a.w2g, C);
  const dim3 pgrid(a.tx, a.ty, a.n);
  const int psm = cnx_bwd_pixel_smem(C), wsm = cnx_bwd_weight_smem(C);
  if (C == 64) {
    if (int rc = attr[0].set(cnx_bwd_pixel_kernel<64>, psm)) return rc;
    GC_KLOG("cnx_bwd_pixel_kernel<64>");
    cnx_bwd_pixel_kernel<64><<<pgrid, 256, psm, st>>>(a);
  } else {
    if (int rc = attr[1].set(cnx_bwd_pixel_kernel<128>, psm)) return rc;
    GC_KLOG("cnx_bwd_pixel_kernel<128>");
    cnx_bwd_pixel_kernel<128><<<pgrid, 256, psm, st>>>(a);
  }
  if (!a.dx_only) {
    const dim3 wgrid(a.slabs, 4 * C / kCnxChunk);
    if (C == 64) {
      if (int rc = attr[2].set(cnx_bwd_weight_kernel<64>, wsm)) return rc;
      GC_KLOG("cnx_bwd_weight_kernel<64>");
      cnx_bwd_weight_kernel<64><<<wgrid, 256, wsm, st>>>(a);
    } else {
      if (int rc = attr[3].set(cnx_bwd_weight_kernel<128>, wsm)) return rc;
      GC_KLOG("cnx_bwd_weight_kernel<128>");
      cnx_bwd_weight_kernel<128><<<wgrid, 256, wsm, st>>>(a);
    }
  }
  GC_KLOG("cnx_bwd_dw_kernel");
  cnx_bwd_dw_kernel<<<dim3(a.slabs, C / kCnxSlab), 256, 0, st>>>(a, C);
  if (!a.dx_only) {
    CnxRedArgs r{};
    r.C = C; r.gamma = a.gamma; r.g_w2 = a.g_w2; r.g_dw_b = a.g_dw_b; r.sdy = a.sdy;
    const long long wstride = 2ll * cc4 + 4 * C;
    int blocks = 0;
    auto add = [&](const float* src, float* dst, long long stride, int parts, int count, int mode) {
      r.job[r.jobs++] = CnxRedJob{src, dst, stride, parts, count, mode, blocks};
      blocks += (count + 15) / 16;
    };
    add(a.p_w, a.s_red, wstride, a.slabs, cc4, CNX_RED_S);
    add(a.p_w + cc4, a.g_w1, wstride, a.slabs, cc4, CNX_RED_PLAIN);
    add(a.p_w + 2 * cc4, a.g_b1, wstride, a.slabs, 4 * C, CNX_RED_PLAIN);
    add(a.p_ln, a.g_ln_w, 2 * C, a.tiles, C, CNX_RED_PLAIN);
    add(a.p_ln + C, a.g_ln_b, 2 * C, a.tiles, C, CNX_RED_PLAIN);
    add(a.p_dw, a.g_dw_w, (long long)C * kCnxDwVals, a.slabs, C * kCnxDwVals, CNX_RED_DW);
    GC_KLOG("cnx_bwd_reduce_kernel");
    cnx_bwd_reduce_kernel<<<blocks, 256, 0, st>>>(r);
    GC_KLOG("cnx_bwd_final_kernel");
    cnx_bwd_final_kernel<<<C, 256, 0, st>>>(a.w2, a.b2, a.gamma, a.s_red, a.sdy, a.g_gamma, a.g_b2, C);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

}  // namespace gc
