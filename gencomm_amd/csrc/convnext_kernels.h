// STAMP's ConvNeXtBlock (opencood/models/stamp_modules/feature_alignnet_modules.py:303-348) as ONE kernel:
//   y = x + gamma * Linear2(GELU(Linear1(LayerNorm_C(dwconv7x7(x) + b_dw)))),   NCHW fp32 in and out.
// A workgroup owns a 4 x 16 pixel tile of one map (64 pixels = the M of both matrix products) and keeps everything between x and y in
// LDS and registers: the [pixels, 4 C] hidden tensor (168 MB per block at the shipped 5 x 128 x 256 x 64) is never complete anywhere.
//
// Depthwise stage: the tile plus its 3-pixel halo (10 x 22 positions, zero outside the map) is staged in slabs of 16 channels (15.5 KB);
// a thread computes 4 horizontally adjacent outputs of one channel from 7 x 10 staged values and the channel's 49 taps, and leaves them
// in the [64][C] image `ln` (row = pixel 16 ty + tx).  The global loads of the next slab are issued before the arithmetic of the current
// one and wait in registers, the taps are requested before the barrier that publishes the slab.  LayerNorm over C (biased variance, eps
// 1e-6, two passes) runs in place, 4 threads per pixel.
// Matrix stage, on v_mfma_f32_16x16x4_f32 (exact fp32 products, a k-ordered fmaf chain per output, as codebook_kernels.h): the hidden
// dimension is walked in chunks of 64.  Per chunk, wave w computes columns 16 w .. 16 w + 15 of h = GELU(ln W1[chunk]^T + b1[chunk]) for
// all 64 pixels, writes them into the [64][64] LDS image `h` between two barriers (the first: every wave has read the previous chunk),
// and every wave accumulates acc += h W2[:, chunk]^T for its C / 4 output channels (4 row tiles x C / 64 column tiles, 16 or 32
// accumulator registers that live across the chunks).  Weights stream from L2 in nn.Linear's own layout (W1 [4 C][C], W2 [C][4 C]): the
// B operand of a lane is a 16-byte load along k in both, so there is no prepared form.  Per tile 2 x 4 C x C x 4 bytes of weights
// against 64 x 16 C^2 FLOP: 32 FLOP per L2 byte, the codec's ratio.
// LDS: ln 64 x (C + 8) floats, h 64 x 72 floats (the halo slab aliases it): 36 KB at C = 64, 52 KB at C = 128; 132 registers: three
// workgroups per CU at both widths (a second h image would save a barrier per chunk and cost the third workgroup).
// Row strides C + 8 and 72 are 8 mod 64 dwords: the A-operand ds_read_b128 of the matrix stage is conflict-free
// (tests/test_stamp_adapter.py restates the arithmetic of tests/test_lds_banks.py on these constants).
// Epilogue: in the C/D layout a lane holds 4 consecutive x of one channel of one tile row: x + gamma (acc + b2) is one 16-byte load and
// store along W (scalar when W % 4 != 0).  No atomics, no dependence on anything but the pixel's 7 x 7 neighbourhood: two runs give the
// same bits.
#pragma once
#include "common.h"

namespace gc {

constexpr int kCnxTileH = 4, kCnxTileW = 16;           // tile_h, tile_w
constexpr int kCnxRows = kCnxTileH * kCnxTileW;        // 64 pixels per workgroup
constexpr int kCnxChunk = 64;                          // hidden columns per chunk
constexpr int kCnxPad = 8;                             // row padding of the LDS images, floats
constexpr int kCnxSlab = 16;                           // channels staged per depthwise slab
constexpr int kCnxHaloH = kCnxTileH + 6, kCnxHaloW = kCnxTileW + 6;
constexpr int kCnxHaloRow = 24;                        // halo row stride, floats (22 used)
constexpr int kCnxHaloCh = kCnxHaloH * kCnxHaloRow + 8;    // halo channel stride: the slab (16 x 248 floats) must fit under the h image; the
                                                           // depthwise stage's ds_read_b128 / _b64 of a wave (4 channels x 4 rows x 4 column
                                                           // quads) then cost 84 extra LDS cycles over its 21 reads (140 at 240, 14 at 32 / 336)

struct CnxArgs {
  const float* x;
  const float* dw_w;    // [C][1][7][7]
  const float* dw_b;    // [C]
  const float* ln_w;
  const float* ln_b;
  const float* w1;      // [4 C][C]
  const float* b1;      // [4 C]
  const float* w2;      // [C][4 C]
  const float* b2;      // [C]
  const float* gamma;   // [C] or null
  float* y;
  int H, W, vec;        // vec: W % 4 == 0 and x, y 16-byte aligned
};

using cnx_f32x4 = __attribute__((ext_vector_type(4))) float;

// acc[rt][t] += A[16 rt + r][k] B[k][16 t + c] over K.  A: an LDS image, `ap` = the lane's row lr at k offset 4 lk, LDA floats between
// rows.  B[k][c] = W[c][k] as nn.Linear stores it: `wp` = row lr of the wave's first column tile at k offset 4 lk, WS floats between rows.
// Lane (lr, lk) holds k = k0 + 4 lk + s of step s for both operands (the order of the 16 k of a step is permuted alike for A and B).
// Two operand sets, one in use and one in flight, pinned as in umgm_linear (codebook_kernels.h).
template <int K, int NT, int LDA>
__device__ __forceinline__ void cnx_mma(const float* ap, const float* __restrict__ wp, int WS, cnx_f32x4 (&acc)[4][NT]) {
  float4 bq[2][NT], aq[2][4];
  auto fetch_b = [&](int set, int k0) {
    k0 = k0 < K ? k0 : K - 16;   // past the end: a valid address, loaded and not used
#pragma unroll
    for (int t = 0; t < NT; ++t) bq[set][t] = *reinterpret_cast<const float4*>(wp + (size_t)t * 16 * WS + k0);
  };
  auto fetch_a = [&](int set, int k0) {
    k0 = k0 < K ? k0 : K - 16;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) aq[set][rt] = *reinterpret_cast<const float4*>(ap + rt * 16 * LDA + k0);
  };
  auto half_step = [&](int set, int s0) {
#pragma unroll
    for (int s = s0; s < s0 + 2; ++s) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        const float4 a4 = aq[set][rt];
        const float av = s == 0 ? a4.x : s == 1 ? a4.y : s == 2 ? a4.z : a4.w;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float4 b4 = bq[set][t];
          const float bv = s == 0 ? b4.x : s == 1 ? b4.y : s == 2 ? b4.z : b4.w;
          acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[rt][t], 0, 0, 0);
        }
      }
    }
  };
  auto step = [&](int set, int k_next) {
    fetch_b(set ^ 1, k_next);
    __builtin_amdgcn_sched_barrier(0);
    half_step(set, 0);
    __builtin_amdgcn_sched_barrier(0);
    fetch_a(set ^ 1, k_next);
    __builtin_amdgcn_sched_barrier(0);
    half_step(set, 2);
    __builtin_amdgcn_sched_barrier(0);
  };
  fetch_b(0, 0);
  fetch_a(0, 0);
#pragma unroll 1
  for (int k0 = 0; k0 < K; k0 += 32) {
    step(0, k0 + 16);
    step(1, k0 + 32);
  }
}

template <int C>
__global__ __launch_bounds__(256, 3) void convnext_block_kernel(const CnxArgs a) {   // 3 waves per SIMD: at most 168 registers
  constexpr int LD = C + kCnxPad, LH = kCnxChunk + kCnxPad, R = kCnxRows, NT = C / 64;
  static_assert(kCnxSlab * kCnxHaloCh <= R * LH, "the halo slab must fit the h image it aliases");
  extern __shared__ __align__(16) float cnx_smem[];
  float* ln = cnx_smem;          // [64][LD]
  float* h = ln + R * LD;        // [64][LH]; the halo slab during the depthwise stage
  float* halo = h;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int H = a.H, W = a.W;
  const int tx0 = blockIdx.x * kCnxTileW, ty0 = blockIdx.y * kCnxTileH;
  const size_t HW = (size_t)H * W;
  const size_t map0 = (size_t)blockIdx.z * C * HW;
  const float* __restrict__ xn = a.x + map0;

  // ---- depthwise 7 x 7, 16 channels at a time: thread = (channel tid / 16 of the slab, tile row (tid / 4) % 4, columns 4 (tid % 4) ..).
  // The global loads of slab s + 1 are issued before the arithmetic of slab s and held in registers; the channel's taps are requested
  // before the barrier that publishes the slab.
  {
    constexpr int SLAB = kCnxSlab * kCnxHaloH * kCnxHaloW, NS = (SLAB + 255) / 256;
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
      const float* __restrict__ wch = a.dw_w + ch * 49;
      float wv[49];
#pragma unroll
      for (int i = 0; i < 49; ++i) wv[i] = wch[i];
      const float bias = a.dw_b[ch];
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

  // ---- LayerNorm over C in place: 4 threads per pixel, channels q, q + 4, ..
  {
    float* row = ln + (tid >> 2) * LD;
    const int q = tid & 3;
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
    const float rstd = 1.0f / sqrtf(v * (1.0f / C) + 1e-6f);
#pragma unroll
    for (int i = 0; i < C / 4; ++i) {
      const int c = q + 4 * i;
      row[c] = fmaf((row[c] - mean) * rstd, a.ln_w[c], a.ln_b[c]);
    }
  }
  __syncthreads();

  // ---- the two Linears, the hidden dimension in chunks of 64
  cnx_f32x4 acc[4][NT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = cnx_f32x4{0.f, 0.f, 0.f, 0.f};
  const int col0 = wave * (C / 4);
#pragma unroll 1
  for (int chunk = 0; chunk < 4 * C / kCnxChunk; ++chunk) {
    const int hcol = chunk * kCnxChunk + 16 * wave + lr;   // the hidden unit this lane's results belong to
    cnx_f32x4 a1[4][1];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) a1[rt][0] = cnx_f32x4{0.f, 0.f, 0.f, 0.f};
    cnx_mma<C, 1, LD>(ln + lr * LD + 4 * lk, a.w1 + (size_t)hcol * C + 4 * lk, C, a1);
    const float bias1 = a.b1[hcol];
    __syncthreads();   // every wave has read the previous chunk's h
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e)   // C/D map: col = lane & 15, row = 4 (lane >> 4) + register
        h[(16 * rt + 4 * lk + e) * LH + 16 * wave + lr] = gelu_erf_f(a1[rt][0][e] + bias1);
    __syncthreads();
    cnx_mma<kCnxChunk, NT, LH>(h + lr * LH + 4 * lk, a.w2 + (size_t)(col0 + lr) * (4 * C) + chunk * kCnxChunk + 4 * lk, 4 * C, acc);
  }

  // ---- y = x + gamma (acc + b2): row tile rt = tile row rt, the lane's 4 registers = 4 consecutive x
  float* __restrict__ yn = a.y + map0;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int ch = col0 + 16 * t + lr;
    const float b2 = a.b2[ch], g = a.gamma != nullptr ? a.gamma[ch] : 1.0f;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
      const int gy = ty0 + rt, gx = tx0 + 4 * lk;
      if (gy >= H || gx >= W) continue;
      const size_t off = (size_t)ch * HW + (size_t)gy * W + gx;
      if (a.vec) {   // W % 4 == 0: the quad is inside the row as a whole
        const float4 xi = *reinterpret_cast<const float4*>(xn + off);
        float4 o;
        o.x = fmaf(g, acc[rt][t][0] + b2, xi.x);
        o.y = fmaf(g, acc[rt][t][1] + b2, xi.y);
        o.z = fmaf(g, acc[rt][t][2] + b2, xi.z);
        o.w = fmaf(g, acc[rt][t][3] + b2, xi.w);
        *reinterpret_cast<float4*>(yn + off) = o;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (gx + e < W) yn[off + e] = fmaf(g, acc[rt][t][e] + b2, xn[off + e]);
      }
    }
  }
}

inline int cnx_smem_bytes(int C) { return (int)((kCnxRows * (C + kCnxPad) + kCnxRows * (kCnxChunk + kCnxPad)) * sizeof(float)); }   // 36 / 52 KB

inline int convnext_block_launch(CnxArgs a, int n, int C, hipStream_t st) {
  if (C != 64 && C != 128) {
    char msg[96];
    snprintf(msg, sizeof msg, "convnext block: C must be 64 or 128 (got %d)", C);
    return fail(-1, msg);   // no such instantiation
  }
  GC_CHECK_ARG(n >= 1 && n <= 65535 && a.H >= 1 && a.W >= 1, "convnext block: 1..65535 maps, positive H / W");
  const int gx = (a.W + kCnxTileW - 1) / kCnxTileW, gy = (a.H + kCnxTileH - 1) / kCnxTileH;
  GC_CHECK_ARG(gy <= 65535, "convnext block: H must be at most 262140");
  GC_CHECK_ARG(a.x && a.dw_w && a.dw_b && a.ln_w && a.ln_b && a.w1 && a.b1 && a.w2 && a.b2 && a.y, "convnext block: null pointer");
  GC_CHECK_ARG((((uintptr_t)a.w1 | (uintptr_t)a.w2) & 15) == 0, "convnext block: w1 and w2 must be 16-byte aligned");
  GC_CHECK_ARG((((uintptr_t)a.x | (uintptr_t)a.y) & 3) == 0, "convnext block: x and y must be 4-byte aligned");
  const size_t bytes = (size_t)n * C * a.H * a.W * sizeof(float);
  const uintptr_t xb = (uintptr_t)a.x, yb = (uintptr_t)a.y;
  GC_CHECK_ARG(xb + bytes <= yb || yb + bytes <= xb, "convnext block: y must not alias x (neighbouring tiles read the halo)");
  a.vec = (a.W % 4 == 0 && ((xb | yb) & 15) == 0) ? 1 : 0;
  const int smem = cnx_smem_bytes(C);
  const dim3 grid(gx, gy, n);
  static LdsAttrOnce attr[2];
  if (C == 64) {
    if (int rc = attr[0].set(convnext_block_kernel<64>, smem)) return rc;
    GC_KLOG("convnext_block_kernel<64>");
    convnext_block_kernel<64><<<grid, 256, smem, st>>>(a);
  } else {
    if (int rc = attr[1].set(convnext_block_kernel<128>, smem)) return rc;
    GC_KLOG("convnext_block_kernel<128>");
    convnext_block_kernel<128><<<grid, 256, smem, st>>>(a);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

}  // namespace gc
