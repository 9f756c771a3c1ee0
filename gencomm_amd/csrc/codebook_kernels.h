// The CodeFilling codebook codec (opencood/models/sub_modules/codebook.py, UMGMQuantizer) as ONE kernel: a workgroup owns 64 rows
// (BEV pixels), keeps every intermediate of the 1..3-level residual quantizer in LDS and registers, reads x once and writes the
// restored rows and the codes once.
//
// Per level i (encoder, _quantizerEncoder.forward): z = E_i(x), h = Q_i(z); per group g of m: logit = -(|h_g|^2 + |c|^2 - 2 h_g.c) /
// sqrt(k) * max(temperature_g, 1e-6), sampled = argmax(logit + gumbel), code = argmax(logit); q_i = the sampled codewords (the
// reference's y_hard - y_soft + y_soft is the one-hot to within 1 ulp, so its einsum is a lookup); x <- LH_i(z) - q_i on all but the
// last level.  Decoder, last level first: f <- R_i(DH_i(q_i) + S_i(f)), S_i absent on the last level.  code_loss = mean((f - x)^2).
//
// Arithmetic: the 16 Linear(C, C) layers and the h . c products of the distances run on v_mfma_f32_16x16x4_f32 (exact fp32 products, a
// k-ordered fmaf chain per output); the norms are plain fp32 FMAs.  No reduced-precision product anywhere: the argmax decisions are
// discontinuous.
// Tiling: 256 threads = 4 waves; a Linear's 64 x C output is split by columns, wave w owns columns w C/4 .. (w + 1) C/4 of all 64 rows
// (4 row tiles x C/64 column tiles of 16 x 16, 16 .. 64 accumulator registers).  Activations live in two LDS images of 64 x (C + 4)
// floats (a Linear may run in place: every wave has finished reading before any wave writes); weights stream from L2, one 16-byte
// load per lane and 16 k, prefetched one step ahead.  At C = 128 the 16 matrices (1 MB) are re-read once per 64 rows: 16 KB per row
// against 0.5 MFLOP per row, i.e. 4.9 TB/s of L2 reads at the full fp32 matrix rate (2.0 TB/s at the measured one) -- below what the
// L2s deliver, so the matrix pipe is the bound.
// A row's result depends on nothing but the row: not on its position in the tile, the tile's other rows, n or the layout.
//
// Supported envelope (anything else is an argument error naming the argument): C in {64, 128, 256}; m in {1, 2, 4}; 1..3 levels;
// k per level a power of two in 16..256; n >= 1.
#pragma once
#include "common.h"

namespace gc {

constexpr int kUmgmRows = 64;        // rows per workgroup
constexpr int kUmgmMaxLevels = 3;
constexpr int kUmgmMaxGroups = 4;
constexpr uint32_t kUmgmStream = 0x554d474du;   // counter word 3 of the codec's Philox draws ("UMGM"): apart from the sampler's fields

enum UmgmTask : int { UMGM_FORWARD = 0, UMGM_ENCODE = 1, UMGM_DECODE = 2 };
enum UmgmNoise : int { UMGM_NOISE_NONE = 0, UMGM_NOISE_UNIFORMS = 1, UMGM_NOISE_PHILOX = 2 };

// parameter blob, per level: {E, Q, LH, DH, S, R} x (weight [C][C], bias [C]), codebook [m][k][C / m], temperature [m] padded to 4.
// The LH and S slots of the last level are present and unread.
enum UmgmSlot : int { UMGM_E = 0, UMGM_Q, UMGM_LH, UMGM_DH, UMGM_S, UMGM_R, UMGM_SLOTS };
inline long long umgm_level_floats(int C, int k) { return (long long)UMGM_SLOTS * ((long long)C * C + C) + (long long)k * C + 4; }

struct UmgmArgs {
  const float* params;
  const float* x;               // rows [n][C], or NCHW [A][C][HW] when HW > 0 (n = A HW)
  const unsigned char* keep;    // NCHW only, may be null: keep[a] != 0 -> agent a's restored map is its input
  const float* uniforms;        // UMGM_NOISE_UNIFORMS: [L][n, m, k_l]
  float* out;                   // restored, layout of x
  long long* codes;             // [L][n][m]: written by FORWARD / ENCODE, read by DECODE
  long long* sampled;           // [L][n][m] or null: the sampled indices (what the decoder restores from)
  float* logits;                // [L][n, m, k_l] or null
  float* partials;              // one squared-error sum per workgroup, or null
  long long n;
  long long level_off[kUmgmMaxLevels];   // float offset of the level in params
  long long field_off[kUmgmMaxLevels];   // element offset of the level in uniforms / logits: n m (k_0 + .. + k_{l-1})
  unsigned long long seed;
  int k[kUmgmMaxLevels];
  int HW, m, L, task, noise;
};

using f32x4 = __attribute__((ext_vector_type(4))) float;

// The 4 uniforms of codewords 4 jq .. 4 jq + 3 of (level, row, group): a function of the address alone.  (2 i + 1) 2^-24, i < 2^23:
// exact in fp32, inside (0, 1).
__device__ __forceinline__ void umgm_uniform4(unsigned long long seed, int level, long long row, int g, int jq, float (&u)[4]) {
  uint32_t w[4];
  philox4x32_7((uint32_t)row, (uint32_t)((unsigned long long)row >> 32), ((uint32_t)level << 28) | ((uint32_t)g << 24) | (uint32_t)jq, kUmgmStream,
               (uint32_t)seed, (uint32_t)(seed >> 32), w);
#pragma unroll
  for (int i = 0; i < 4; ++i) u[i] = fmaf((float)(w[i] >> 9), 1.1920928955078125e-7f /* 2^-23 */, 5.9604644775390625e-8f /* 2^-24 */);
}
// the reference's gumbelSoftmax: uniforms.clamp_(eps, 1 - eps), -log(-log u), eps of float32
__device__ __forceinline__ float umgm_gumbel(float u) {
  const float eps = 1.1920928955078125e-7f;
  u = fminf(fmaxf(u, eps), 1.0f - eps);
  return -logf(-logf(u));
}

// out [64][C] = in0 W0^T + b0 (+ in1 W1^T + b1) (- the sampled codeword of each row and group); in / out: LDS images with row stride
// C + 4; W [C][C] as nn.Linear stores it.  out may alias in0 or in1.  Ends with a barrier.
template <int C>
__device__ __forceinline__ void umgm_linear(const float* in0, const float* __restrict__ W0, const float* __restrict__ b0, const float* in1,
                                            const float* __restrict__ W1, const float* __restrict__ b1, float* out,
                                            const float* __restrict__ sub_cb, const int* sub_idx, int k, int d, int m) {
  constexpr int LD = C + 4, NT = C / 64, R = kUmgmRows;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const int col0 = wave * (C / 4);
  f32x4 acc[4][NT];
#pragma unroll
  for (int rt = 0; rt < 4; ++rt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int src = 0; src < 2; ++src) {
    const float* in = src ? in1 : in0;
    const float* __restrict__ W = src ? W1 : W0;
    if (in == nullptr) break;
    // lane (lr, lk) holds k = k0 + 4 lk + s of step s for both operands: the order of the 16 k within a step is permuted alike for A and B
    const float* wp = W + (size_t)(col0 + lr) * C + 4 * lk;
    const float* ap = in + lr * LD + 4 * lk;
    // Two operand sets, one in use and one in flight: the loads of step i + 1 (weights from L2, activations from LDS) are issued during
    // the 16 NT matrix instructions of step i (a step keeps the matrix pipe busy for 512 NT cycles) and pinned there -- left to
    // itself the scheduler sinks each load to just before its first use and every step waits out an L2 round trip.
    float4 bq[2][NT], aq[2][4];
    auto fetch_b = [&](int set, int k0) {
      k0 = k0 < C ? k0 : C - 16;   // past the end: a valid address, loaded and not used
#pragma unroll
      for (int t = 0; t < NT; ++t) bq[set][t] = *reinterpret_cast<const float4*>(wp + (size_t)t * 16 * C + k0);
    };
    auto fetch_a = [&](int set, int k0) {
      k0 = k0 < C ? k0 : C - 16;
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) aq[set][rt] = *reinterpret_cast<const float4*>(ap + rt * 16 * LD + k0);
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
    auto step = [&](int set, int k_next) {   // the weights of the next step first, its activations half a step later (LDS answers sooner)
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
    for (int k0 = 0; k0 < C; k0 += 32) {
      step(0, k0 + 16);
      step(1, k0 + 32);
    }
  }
  __syncthreads();   // every wave has read its operands: `out` may be one of them
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = col0 + 16 * t + lr;
    float bias = b0[col];
    if (in1 != nullptr) bias += b1[col];
    const int g = sub_cb ? col / d : 0, cd = sub_cb ? col - g * d : 0;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * rt + 4 * lk + e;   // C/D map: col = lane & 15, row = 4 (lane >> 4) + register
        float v = acc[rt][t][e] + bias;
        if (sub_cb) v -= sub_cb[((size_t)g * k + sub_idx[row * kUmgmMaxGroups + g]) * d + cd];
        out[row * LD + col] = v;
      }
    }
  }
  (void)R; (void)m;
  __syncthreads();
}

template <int C>
__global__ __launch_bounds__(256) void umgm_kernel(const UmgmArgs a) {
  constexpr int LD = C + 4, R = kUmgmRows, G = kUmgmMaxGroups;
  extern __shared__ __align__(16) float umgm_smem[];
  float* bufA = umgm_smem;
  float* bufB = bufA + R * LD;
  int* sidx = reinterpret_cast<int*>(bufB + R * LD);                         // [L][R][G] sampled index
  __shared__ float red[4];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const long long row0 = (long long)blockIdx.x * R;
  const int m = a.m, d = C / m, L = a.L;
  const int rows_here = (int)(a.n - row0 < R ? a.n - row0 : R);

  // ---- the tile of x (rows past n: zeros, computed on and never stored)
  auto load_x = [&](float* dst) {
    if (a.HW > 0) {
      for (int i = tid; i < R * C; i += 256) {
        const int r = i % R, c = i / R;
        float v = 0.f;
        if (r < rows_here) {
          const long long gr = row0 + r, ag = gr / a.HW, hw = gr - ag * a.HW;
          v = a.x[((size_t)ag * C + c) * a.HW + hw];
        }
        dst[r * LD + c] = v;
      }
    } else {
      for (int i = tid; i < R * (C / 4); i += 256) {
        const int r = i / (C / 4), c4 = i % (C / 4);
        float4 v = float4{0.f, 0.f, 0.f, 0.f};
        if (r < rows_here) v = *reinterpret_cast<const float4*>(a.x + (size_t)(row0 + r) * C + 4 * c4);
        *reinterpret_cast<float4*>(dst + r * LD + 4 * c4) = v;
      }
    }
  };

  if (a.task != UMGM_DECODE) {
    load_x(bufA);
    __syncthreads();
    for (int l = 0; l < L; ++l) {
      const float* P = a.params + a.level_off[l];
      const size_t slot = (size_t)C * C + C;
      const int k = a.k[l];
      const float* cb = P + UMGM_SLOTS * slot;
      const float* temp = cb + (size_t)k * C;
      umgm_linear<C>(bufA, P + UMGM_E * slot, P + UMGM_E * slot + C * C, nullptr, nullptr, nullptr, bufA, nullptr, nullptr, 0, 1, m);   // z
      umgm_linear<C>(bufA, P + UMGM_Q * slot, P + UMGM_Q * slot + C * C, nullptr, nullptr, nullptr, bufB, nullptr, nullptr, 0, 1, m);   // h
      // ---- nearest codeword, on the matrix pipe too: wave w owns rows 16 w .. 16 w + 15 and walks, per group, the k / 16 tiles of 16
      // codewords: h_g . c as 16 x 16 x d products (lane (lr, lk): row / codeword lr, the k slice lk, as in umgm_linear), |c|^2 and
      // |h|^2 from the operands the lane holds.  In the result a lane holds codeword 16 ct + lr of rows 4 lk + e: the best of a row is
      // kept per lane over the tiles (ascending, strictly greater) and then taken over the 16 lanes -- no other wave is involved.
      {
        const int lr = lane & 15, lk = lane >> 4, rbase = 16 * wave, q4 = lr & 3;
        const float scale = sqrtf((float)k);
#pragma unroll 1
        for (int g = 0; g < m; ++g) {
          const float* hrow = bufB + (rbase + lr) * LD + g * d + 4 * lk;
          float hp = 0.f;
          for (int k0 = 0; k0 < d; k0 += 16) {
            const float4 h4 = *reinterpret_cast<const float4*>(hrow + k0);
            hp = fmaf(h4.x, h4.x, hp); hp = fmaf(h4.y, h4.y, hp); hp = fmaf(h4.z, h4.z, hp); hp = fmaf(h4.w, h4.w, hp);
          }
          hp += __shfl_xor(hp, 16);
          hp += __shfl_xor(hp, 32);          // |h_g|^2 of row lr, in every lane of that lr
          float h2[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) h2[e] = __shfl(hp, 4 * lk + e);
          const float tg = fmaxf(temp[g], 1e-6f);
          float vs[4], vc[4];
          int is[4], ic[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) { vs[e] = vc[e] = -INFINITY; is[e] = ic[e] = 0; }
#pragma unroll 1
          for (int ct = 0; ct < (k >> 4); ++ct) {
            const int j = 16 * ct + lr;
            const float* crow = cb + ((size_t)g * k + j) * d + 4 * lk;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            float cp = 0.f;
            for (int k0 = 0; k0 < d; k0 += 16) {
              const float4 h4 = *reinterpret_cast<const float4*>(hrow + k0);
              const float4 c4 = *reinterpret_cast<const float4*>(crow + k0);
              cp = fmaf(c4.x, c4.x, cp); cp = fmaf(c4.y, c4.y, cp); cp = fmaf(c4.z, c4.z, cp); cp = fmaf(c4.w, c4.w, cp);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h4.x, c4.x, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h4.y, c4.y, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h4.z, c4.z, acc, 0, 0, 0);
              acc = __builtin_amdgcn_mfma_f32_16x16x4f32(h4.w, c4.w, acc, 0, 0, 0);
            }
            cp += __shfl_xor(cp, 16);
            cp += __shfl_xor(cp, 32);        // |c|^2 of codeword j
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int r = rbase + 4 * lk + e;
              const long long gr = row0 + r;
              const bool valid = r < rows_here;
              const float dist = h2[e] + cp - 2.f * acc[e];
              // ENCODE is the reference's encode(): argmin of the distance, no temperature
              const float logit = a.task == UMGM_ENCODE ? -dist : -dist / scale * tg;
              const size_t fo = (size_t)a.field_off[l] + ((size_t)gr * m + g) * k + j;
              if (a.logits != nullptr && valid) a.logits[fo] = logit;
              float y = logit;
              if (a.noise == UMGM_NOISE_UNIFORMS) {
                y += umgm_gumbel(valid ? a.uniforms[fo] : 0.5f);
              } else if (a.noise == UMGM_NOISE_PHILOX) {
                float u[4];
                umgm_uniform4(a.seed, l, gr, g, j >> 2, u);
                y += umgm_gumbel(q4 == 0 ? u[0] : q4 == 1 ? u[1] : q4 == 2 ? u[2] : u[3]);
              }
              if (y > vs[e]) { vs[e] = y; is[e] = j; }          // strictly greater: the lowest index among equal maxima
              if (logit > vc[e]) { vc[e] = logit; ic[e] = j; }
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int mask = 1; mask < 16; mask <<= 1) {          // over the 16 codeword lanes: the greater value, the lower index among equals
              const float ovs = __shfl_xor(vs[e], mask), ovc = __shfl_xor(vc[e], mask);
              const int ois = __shfl_xor(is[e], mask), oic = __shfl_xor(ic[e], mask);
              if (ovs > vs[e] || (ovs == vs[e] && ois < is[e])) { vs[e] = ovs; is[e] = ois; }
              if (ovc > vc[e] || (ovc == vc[e] && oic < ic[e])) { vc[e] = ovc; ic[e] = oic; }
            }
            const int r = rbase + 4 * lk + e;
            if (lr == 0) {
              sidx[(l * R + r) * G + g] = is[e];
              if (r < rows_here) {
                a.codes[((size_t)l * a.n + row0 + r) * m + g] = ic[e];
                if (a.sampled != nullptr) a.sampled[((size_t)l * a.n + row0 + r) * m + g] = is[e];
              }
            }
          }
        }
      }
      __syncthreads();
      if (l < L - 1)   // the residual: x <- LH(z) - q
        umgm_linear<C>(bufA, P + UMGM_LH * slot, P + UMGM_LH * slot + C * C, nullptr, nullptr, nullptr, bufA, cb, sidx + l * R * G, k, d, m);
    }
    if (a.task == UMGM_ENCODE) return;
  } else {
    for (int i = tid; i < L * R * m; i += 256) {
      const int g = i % m, r = (i / m) % R, l = i / (m * R);
      long long c = 0;
      if (r < rows_here) c = a.codes[((size_t)l * a.n + row0 + r) * m + g];
      c = c < 0 ? 0 : c >= a.k[l] ? a.k[l] - 1 : c;   // a code outside the codebook must not become an address
      sidx[(l * R + r) * G + g] = (int)c;
    }
    __syncthreads();
  }

  // ---- decoder, last level first: f <- R(DH(q) + S(f)); f lives in bufA
  for (int l = L - 1; l >= 0; --l) {
    const float* P = a.params + a.level_off[l];
    const size_t slot = (size_t)C * C + C;
    const int k = a.k[l];
    const float* cb = P + UMGM_SLOTS * slot;
    for (int i = tid; i < R * (C / 4); i += 256) {
      const int r = i / (C / 4), c = 4 * (i % (C / 4)), g = c / d;   // d is a multiple of 4: a quad stays inside its group
      *reinterpret_cast<float4*>(bufB + r * LD + c) =
          *reinterpret_cast<const float4*>(cb + ((size_t)g * k + sidx[(l * R + r) * G + g]) * d + (c - g * d));
    }
    __syncthreads();
    const bool side = l < L - 1;
    umgm_linear<C>(bufB, P + UMGM_DH * slot, P + UMGM_DH * slot + C * C, side ? bufA : nullptr, P + UMGM_S * slot, P + UMGM_S * slot + C * C,
                   bufA, nullptr, nullptr, 0, 1, m);
    umgm_linear<C>(bufA, P + UMGM_R * slot, P + UMGM_R * slot + C * C, nullptr, nullptr, nullptr, bufA, nullptr, nullptr, 0, 1, m);
  }

  // ---- restored rows out, and the tile's squared error against x (before the pass-through overwrite)
  if (a.task == UMGM_FORWARD) {
    load_x(bufB);
    __syncthreads();
    float s = 0.f;
    for (int i = tid; i < R * C; i += 256) {   // one mapping for both layouts: the sum's order does not depend on the layout
      const int r = i / C, c = i % C;
      const float df = bufA[r * LD + c] - bufB[r * LD + c];
      if (r < rows_here) s = fmaf(df, df, s);
    }
    s = wave_sum(s);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0 && a.partials != nullptr) a.partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  if (a.HW > 0) {
    for (int i = tid; i < R * C; i += 256) {
      const int r = i % R, c = i / R;
      if (r < rows_here) {
        const long long gr = row0 + r, ag = gr / a.HW, hw = gr - ag * a.HW;
        const bool kept = a.task == UMGM_FORWARD && a.keep != nullptr && a.keep[ag] != 0;
        a.out[((size_t)ag * C + c) * a.HW + hw] = kept ? bufB[r * LD + c] : bufA[r * LD + c];
      }
    }
  } else {
    for (int i = tid; i < R * (C / 4); i += 256) {
      const int r = i / (C / 4), c4 = i % (C / 4);
      if (r < rows_here) *reinterpret_cast<float4*>(a.out + (size_t)(row0 + r) * C + 4 * c4) = *reinterpret_cast<const float4*>(bufA + r * LD + 4 * c4);
    }
  }
}

// code_loss = (sum of the per-workgroup partial sums, in a fixed order) / count: no atomics, two runs give the same bits
__global__ __launch_bounds__(256) void umgm_loss_kernel(const float* __restrict__ partials, int blocks, double count, float* __restrict__ loss) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < blocks; i += 256) s += (double)partials[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = (float)(part[0] / count);
}

// the uniforms UMGM_NOISE_PHILOX draws, written out as [L][n, m, k_l]: one thread per (row, group, codeword quad) of a level
__global__ __launch_bounds__(256) void umgm_noise_kernel(float* __restrict__ out, unsigned long long seed, int level, long long n, int m, int k) {
  const long long items = n * m * (k >> 2);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long long)gridDim.x * 256) {
    const int jq = (int)(i % (k >> 2));
    const long long rg = i / (k >> 2);
    float u[4];
    umgm_uniform4(seed, level, rg / m, (int)(rg % m), jq, u);
    *reinterpret_cast<float4*>(out + (size_t)rg * k + 4 * jq) = float4{u[0], u[1], u[2], u[3]};
  }
}

inline int umgm_smem_bytes(int C) {
  return (int)(2 * kUmgmRows * (C + 4) * sizeof(float) + kUmgmMaxLevels * kUmgmRows * kUmgmMaxGroups * sizeof(int));   // 37 / 69 / 133 KB
}

inline int umgm_check_shape(int C, int m, const int* k, int L) {
  GC_CHECK_ARG(C == 64 || C == 128 || C == 256, "umgm: channel must be 64, 128 or 256");
  GC_CHECK_ARG(m == 1 || m == 2 || m == 4, "umgm: m must be 1, 2 or 4");
  GC_CHECK_ARG(L >= 1 && L <= kUmgmMaxLevels, "umgm: levels (len(k)) must be 1, 2 or 3");
  GC_CHECK_ARG(k != nullptr, "umgm: null pointer (k)");
  for (int l = 0; l < L; ++l) GC_CHECK_ARG(k[l] >= 16 && k[l] <= 256 && (k[l] & (k[l] - 1)) == 0, "umgm: k must be a power of two in 16 .. 256 on every level");
  return GC_OK;
}

inline int umgm_launch(UmgmArgs a, int C, const int* k, float* loss, hipStream_t st) {
  GC_CHECK_ARG(a.n >= 1 && a.n <= (1ll << 31) * kUmgmRows - kUmgmRows, "umgm: n must be at least 1 (and at most 2^37 rows)");
  long long po = 0, fo = 0;
  for (int l = 0; l < a.L; ++l) {
    a.k[l] = k[l];
    a.level_off[l] = po;
    a.field_off[l] = fo;
    po += umgm_level_floats(C, k[l]);
    fo += a.n * a.m * k[l];
  }
  const unsigned blocks = (unsigned)((a.n + kUmgmRows - 1) / kUmgmRows);
  const int smem = umgm_smem_bytes(C);
  static LdsAttrOnce attr[3];
  if (C == 64) {
    if (int rc = attr[0].set(umgm_kernel<64>, smem)) return rc;
    GC_KLOG("umgm_kernel<64>");
    umgm_kernel<64><<<blocks, 256, smem, st>>>(a);
  } else if (C == 128) {
    if (int rc = attr[1].set(umgm_kernel<128>, smem)) return rc;
    GC_KLOG("umgm_kernel<128>");
    umgm_kernel<128><<<blocks, 256, smem, st>>>(a);
  } else {
    if (int rc = attr[2].set(umgm_kernel<256>, smem)) return rc;
    GC_KLOG("umgm_kernel<256>");
    umgm_kernel<256><<<blocks, 256, smem, st>>>(a);
  }
  GC_HIP(hipGetLastError());
  if (loss != nullptr) {
    umgm_loss_kernel<<<1, 256, 0, st>>>(a.partials, (int)blocks, (double)a.n * C, loss);
    GC_HIP(hipGetLastError());
  }
  return GC_OK;
}

}  // namespace gc
