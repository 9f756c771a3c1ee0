// Straight-through backward of the CodeFilling codec (codebook_kernels.h): the gradient of (restored, code_loss) with respect to the
// input rows, the 16 Linear heads, the tied codebooks and the temperatures.  No float atomics anywhere: two runs give the same bits.
//
// Forward of a level (see codebook_kernels.h): z = E x, h = Q z, logit = -|h_g - c|^2 / sqrt(k) * T_g, y = logit + gumbel,
// p = softmax(y), s = argmax(y), sample = onehot(s) - p.detach() + p, q = sample . codebook, x' = LH z - q; decoder t = DH q + S f',
// f = R t.  The adjoint: d sample[c] = dq . c reaches the logits only through p, dy = p (d sample - sum_c p d sample);
// d dist = -T / sqrt(k) dy; dh = sum_c d dist 2 (h - c); dT = sum dy (-dist / sqrt(k)); the codebook collects the sampled rows of dq
// (decoder's dequantizer minus the encoder's residual) and sum_n d dist 2 (c - h).
//
// umgm_bwd_kernel: a workgroup owns the forward's 64-row tile.  It recomputes the forward with the forward's own umgm_linear and the
// SAVED sampled indices (an argmax is never re-decided), then walks the adjoint: decoder first level first, encoder last level first.
// Two 64 x (C + 4) LDS images as in the forward; the backward has more live tensors per level than two images hold, so every
// intermediate goes to a global workspace of row-major [rows][C] slots -- which is also where the weight gradients read their operand
// pairs from.  Input gradients are umgm_linear on a transposed copy of the weights (umgm_transpose_kernel, once per call) with zero
// biases.  The k-sized products of the distance adjoint run on the vector pipe, 4 threads per row (they are k / C of a Linear each):
// the distances, d sample, the softmax and its adjoint in double (d sample - sum p d sample cancels, and p of a near tie multiplies
// large d sample values), dh and the codebook's distance term as fp32 FMA chains.
// Weight gradients: rows_wgrad_kernel, dW [Co][Ci] = G^T A over [rows] on v_mfma_f32_16x16x4_f32, split over row ranges whose partial
// products a second kernel adds in a fixed order.  Bias, codebook and temperature gradients: per-tile partials, added in tile order
// by umgm_bwd_small_kernel, which also applies LowerBound's gradient rule to the temperature.
#pragma once
#include "codebook_kernels.h"

namespace gc {

// workspace slots of a level, each [tiles 64][C]
enum UmgmWsSlot : int { UW_X = 0, UW_Z, UW_H, UW_Q, UW_T, UW_F, UW_DF, UW_DT, UW_DQ, UW_DH, UW_DXN, UW_DZ, UW_SLOTS };
constexpr int kRowsWgradMax = 16;       // matrices per launch
constexpr int kRowsWgradSplits = 16;    // most workgroups over the rows of a matrix (4 row ranges each)

struct UmgmBwdArgs {
  UmgmArgs f;                    // params, x, keep, uniforms, n, level_off, field_off, seed, k, HW, m, L, noise as in the forward
  const float* tparams;          // per level 6 x (W^T [C][C], zeros [C])
  const long long* sampled;      // [L][n][m], what the forward returned
  const float* d_restored;       // layout of x, or null
  const float* d_loss;           // one float on the device, or null
  float* dx;
  float* rows_ws;                // [L][UW_SLOTS][tiles 64][C]
  double* dist_ws;               // [tiles 64][m][3][kmax]
  float* small_ws;               // [tiles][small_floats]: per level 6 bias gradients [C], codebook [k C], temperature [4]
  long long rows_padded, small_floats;
  long long small_off[kUmgmMaxLevels];
  int kmax, dx_only;
};

inline long long umgm_small_level_floats(int C, int k) { return (long long)UMGM_SLOTS * C + (long long)k * C + 4; }

__global__ __launch_bounds__(256) void umgm_transpose_kernel(const float* __restrict__ params, float* __restrict__ tparams, long long off0, long long off1,
                                                             long long off2, int C, int L) {
  const long long slot = (long long)C * C + C, total = (long long)L * UMGM_SLOTS * slot;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int l = (int)(i / (UMGM_SLOTS * slot));
    const long long rem = i - (long long)l * UMGM_SLOTS * slot;
    const int s = (int)(rem / slot);
    const long long e = rem - (long long)s * slot;
    float v = 0.f;
    if (e < (long long)C * C) {
      const int r = (int)(e / C), c = (int)(e % C);
      v = params[(l == 0 ? off0 : l == 1 ? off1 : off2) + s * slot + (long long)c * C + r];
    }
    tparams[i] = v;
  }
}

template <int C>
__global__ __launch_bounds__(256) void umgm_bwd_kernel(const UmgmBwdArgs b) {
  constexpr int LD = C + 4, R = kUmgmRows, G = kUmgmMaxGroups;
  extern __shared__ __align__(16) float umgm_smem[];
  float* bufA = umgm_smem;
  float* bufB = bufA + R * LD;
  int* sidx = reinterpret_cast<int*>(bufB + R * LD);                         // [L][R][G] sampled index
  __shared__ double tred[256];

  const UmgmArgs& a = b.f;
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * R;
  const int m = a.m, d = C / m, L = a.L;
  const int rows_here = (int)(a.n - row0 < R ? a.n - row0 : R);
  const size_t slot = (size_t)C * C + C;
  const bool grads = b.dx_only == 0;
  float* small = b.small_ws + (size_t)blockIdx.x * b.small_floats;

  // a tile of a tensor in the layout of x (rows past n: zeros)
  auto load_tile = [&](const float* src, float* dst) {
    if (a.HW > 0) {
      for (int i = tid; i < R * C; i += 256) {
        const int r = i % R, c = i / R;
        float v = 0.f;
        if (r < rows_here && src != nullptr) {
          const long long gr = row0 + r, ag = gr / a.HW, hw = gr - ag * a.HW;
          v = src[((size_t)ag * C + c) * a.HW + hw];
        }
        dst[r * LD + c] = v;
      }
    } else {
      for (int i = tid; i < R * (C / 4); i += 256) {
        const int r = i / (C / 4), c4 = i % (C / 4);
        float4 v = float4{0.f, 0.f, 0.f, 0.f};
        if (r < rows_here && src != nullptr) v = *reinterpret_cast<const float4*>(src + (size_t)(row0 + r) * C + 4 * c4);
        *reinterpret_cast<float4*>(dst + r * LD + 4 * c4) = v;
      }
    }
  };
  auto ws_rows = [&](int l, int s) { return b.rows_ws + (((size_t)l * UW_SLOTS + s) * b.rows_padded + row0) * C; };
  // LDS image -> workspace slot (every thread reads the image before the next barrier; the image may be overwritten after it)
  auto spill = [&](const float* buf, int l, int s) {
    float* dst = ws_rows(l, s);
    for (int i = tid; i < R * (C / 4); i += 256) {
      const int r = i / (C / 4), c4 = i % (C / 4);
      *reinterpret_cast<float4*>(dst + (size_t)r * C + 4 * c4) = *reinterpret_cast<const float4*>(buf + r * LD + 4 * c4);
    }
  };
  // workspace slot (minus another) -> LDS image; barriers on both sides
  auto fill = [&](float* buf, int l, int s, int l_sub, int s_sub) {
    __syncthreads();
    const float* src = ws_rows(l, s);
    const float* sub = s_sub >= 0 ? ws_rows(l_sub, s_sub) : nullptr;
    for (int i = tid; i < R * (C / 4); i += 256) {
      const int r = i / (C / 4), c4 = i % (C / 4);
      float4 v = *reinterpret_cast<const float4*>(src + (size_t)r * C + 4 * c4);
      if (sub != nullptr) {
        const float4 w = *reinterpret_cast<const float4*>(sub + (size_t)r * C + 4 * c4);
        v.x -= w.x; v.y -= w.y; v.z -= w.z; v.w -= w.w;
      }
      *reinterpret_cast<float4*>(buf + r * LD + 4 * c4) = v;
    }
    __syncthreads();
  };
  // the tile's share of a bias gradient: the column sums of an image, rows in order
  auto colsum = [&](const float* buf, float* dst0, float* dst1) {
    if (grads && tid < C) {
      float s = 0.f;
      for (int r = 0; r < R; ++r) s += buf[r * LD + tid];
      dst0[tid] = s;
      if (dst1 != nullptr) dst1[tid] = s;
    }
  };

  // ---- the saved sampled indices
  for (int i = tid; i < L * R * m; i += 256) {
    const int g = i % m, r = (i / m) % R, l = i / (m * R);
    long long c = 0;
    if (r < rows_here) c = b.sampled[((size_t)l * a.n + row0 + r) * m + g];
    c = c < 0 ? 0 : c >= a.k[l] ? a.k[l] - 1 : c;   // an index outside the codebook must not become an address
    sidx[(l * R + r) * G + g] = (int)c;
  }
  load_tile(a.x, bufA);
  __syncthreads();

  // ---- the forward again, with the forward's own Linear: encoder
  for (int l = 0; l < L; ++l) {
    const float* P = a.params + a.level_off[l];
    const int k = a.k[l];
    const float* cb = P + UMGM_SLOTS * slot;
    if (grads) spill(bufA, l, UW_X);
    umgm_linear<C>(bufA, P + UMGM_E * slot, P + UMGM_E * slot + C * C, nullptr, nullptr, nullptr, bufA, nullptr, nullptr, 0, 1, m);   // z
    if (grads) spill(bufA, l, UW_Z);
    umgm_linear<C>(bufA, P + UMGM_Q * slot, P + UMGM_Q * slot + C * C, nullptr, nullptr, nullptr, bufB, nullptr, nullptr, 0, 1, m);   // h
    spill(bufB, l, UW_H);
    if (l < L - 1)
      umgm_linear<C>(bufA, P + UMGM_LH * slot, P + UMGM_LH * slot + C * C, nullptr, nullptr, nullptr, bufA, cb, sidx + l * R * G, k, d, m);
  }
  __syncthreads();
  // ---- decoder, last level first; f lives in bufA
  for (int l = L - 1; l >= 0; --l) {
    const float* P = a.params + a.level_off[l];
    const int k = a.k[l];
    const float* cb = P + UMGM_SLOTS * slot;
    for (int i = tid; i < R * (C / 4); i += 256) {
      const int r = i / (C / 4), c = 4 * (i % (C / 4)), g = c / d;
      *reinterpret_cast<float4*>(bufB + r * LD + c) =
          *reinterpret_cast<const float4*>(cb + ((size_t)g * k + sidx[(l * R + r) * G + g]) * d + (c - g * d));
    }
    __syncthreads();
    if (grads) spill(bufB, l, UW_Q);
    const bool side = l < L - 1;
    umgm_linear<C>(bufB, P + UMGM_DH * slot, P + UMGM_DH * slot + C * C, side ? bufA : nullptr, P + UMGM_S * slot, P + UMGM_S * slot + C * C,
                   bufA, nullptr, nullptr, 0, 1, m);
    if (grads) spill(bufA, l, UW_T);
    umgm_linear<C>(bufA, P + UMGM_R * slot, P + UMGM_R * slot + C * C, nullptr, nullptr, nullptr, bufA, nullptr, nullptr, 0, 1, m);
    if (grads && l > 0) spill(bufA, l, UW_F);
  }

  // ---- d f_0 = g_restored (not of a kept agent: its restored map is its input) + g_loss 2 (f_0 - x) / (n C); zero past n
  {
    const float gl = b.d_loss != nullptr ? *b.d_loss : 0.f;
    const float ls = (float)(2.0 / ((double)a.n * C)) * gl;
    load_tile(a.x, bufB);
    __syncthreads();
    for (int i = tid; i < R * C; i += 256) {
      const int r = a.HW > 0 ? i % R : i / C, c = a.HW > 0 ? i / R : i % C;   // along the contiguous axis of d_restored
      float v = 0.f;
      if (r < rows_here) {
        v = ls * (bufA[r * LD + c] - bufB[r * LD + c]);
        if (b.d_restored != nullptr) {
          if (a.HW > 0) {
            const long long gr = row0 + r, ag = gr / a.HW, hw = gr - ag * a.HW;
            if (!(a.keep != nullptr && a.keep[ag] != 0)) v += b.d_restored[((size_t)ag * C + c) * a.HW + hw];
          } else {
            v += b.d_restored[(size_t)(row0 + r) * C + c];
          }
        }
      }
      bufA[r * LD + c] = v;
    }
    __syncthreads();
  }

  // ---- adjoint of the decoder, first level first: bufA = d f_l
  for (int l = 0; l < L; ++l) {
    const float* TP = b.tparams + (size_t)l * UMGM_SLOTS * slot;
    float* sm = small + b.small_off[l];
    if (grads) spill(bufA, l, UW_DF);
    colsum(bufA, sm + UMGM_R * C, nullptr);
    umgm_linear<C>(bufA, TP + UMGM_R * slot, TP + UMGM_R * slot + C * C, nullptr, nullptr, nullptr, bufA, nullptr, nullptr, 0, 1, m);      // d t
    if (grads) spill(bufA, l, UW_DT);
    colsum(bufA, sm + UMGM_DH * C, l < L - 1 ? sm + UMGM_S * C : nullptr);
    umgm_linear<C>(bufA, TP + UMGM_DH * slot, TP + UMGM_DH * slot + C * C, nullptr, nullptr, nullptr, bufB, nullptr, nullptr, 0, 1, m);    // d q (decoder)
    spill(bufB, l, UW_DQ);
    if (l < L - 1)
      umgm_linear<C>(bufA, TP + UMGM_S * slot, TP + UMGM_S * slot + C * C, nullptr, nullptr, nullptr, bufA, nullptr, nullptr, 0, 1, m);    // d f_{l+1}
  }

  // ---- adjoint of the encoder, last level first: bufA = d x_{l+1} (the residual's gradient) below the last level
  for (int l = L - 1; l >= 0; --l) {
    const float* P = a.params + a.level_off[l];
    const float* TP = b.tparams + (size_t)l * UMGM_SLOTS * slot;
    float* sm = small + b.small_off[l];
    const int k = a.k[l];
    const float* cb = P + UMGM_SLOTS * slot;
    const float* temp = cb + (size_t)k * C;
    const bool res = l < L - 1;
    if (res) {
      __syncthreads();
      spill(bufA, l, UW_DXN);
      colsum(bufA, sm + UMGM_LH * C, nullptr);
    }
    fill(bufA, l, UW_H, 0, -1);                                   // h
    fill(bufB, l, UW_DQ, l, res ? (int)UW_DXN : -1);              // d q = decoder's - residual's
    // -- distances: thread (row, group, sub) of 64 x m x (4 / m)
    const int S = 4 / m, row = tid >> 2, part = tid & 3, g = part / S, sub = part - g * S;
    const long long gr = row0 + row;
    const bool valid = row < rows_here;
    const float scale = sqrtf((float)k), tg = fmaxf(temp[g], 1e-6f);
    // double from here to d dist: p of a near tie multiplies large d sample values, and d sample - sum p d sample cancels
    double* sc_y = b.dist_ws + (((size_t)blockIdx.x * R + row) * m + g) * 3 * b.kmax;   // y, then d dist
    double* sc_ds = sc_y + b.kmax;
    double* sc_di = sc_ds + b.kmax;
    const float* hrow = bufA + row * LD + g * d;
    const float* qrow = bufB + row * LD + g * d;
    const int kc = k / S, c_lo = sub * kc;
    double mx = -INFINITY;
    for (int cq = c_lo; cq < c_lo + kc; cq += 4) {
      float u[4] = {0.5f, 0.5f, 0.5f, 0.5f};
      if (a.noise == UMGM_NOISE_PHILOX) {
        umgm_uniform4(a.seed, l, gr, g, cq >> 2, u);
      } else if (a.noise == UMGM_NOISE_UNIFORMS && valid) {
        const float4 u4 = *reinterpret_cast<const float4*>(a.uniforms + (size_t)a.field_off[l] + ((size_t)gr * m + g) * k + cq);
        u[0] = u4.x; u[1] = u4.y; u[2] = u4.z; u[3] = u4.w;
      }
#pragma unroll
      for (int ci = 0; ci < 4; ++ci) {
        const int c = cq + ci;
        const float* crow = cb + ((size_t)g * k + c) * d;
        double dist = 0.0, ds = 0.0;
        for (int j = 0; j < d; j += 4) {
          const float4 h4 = *reinterpret_cast<const float4*>(hrow + j);
          const float4 q4 = *reinterpret_cast<const float4*>(qrow + j);
          const float4 c4 = *reinterpret_cast<const float4*>(crow + j);
          double t;
          t = (double)h4.x - c4.x; dist = fma(t, t, dist); ds = fma((double)q4.x, (double)c4.x, ds);
          t = (double)h4.y - c4.y; dist = fma(t, t, dist); ds = fma((double)q4.y, (double)c4.y, ds);
          t = (double)h4.z - c4.z; dist = fma(t, t, dist); ds = fma((double)q4.z, (double)c4.z, ds);
          t = (double)h4.w - c4.w; dist = fma(t, t, dist); ds = fma((double)q4.w, (double)c4.w, ds);
        }
        double y = -dist / scale * tg;
        if (a.noise != UMGM_NOISE_NONE) {   // the forward's clamp, then -log(-log u)
          const double uc = fmin(fmax((double)u[ci], 1.1920928955078125e-7), 1.0 - 1.1920928955078125e-7);
          y -= log(-log(uc));
        }
        sc_y[c] = y; sc_ds[c] = ds; sc_di[c] = dist;
        mx = fmax(mx, y);
      }
    }
    for (int mask = 1; mask < S; mask <<= 1) mx = fmax(mx, __shfl_xor(mx, mask));
    double Z = 0.0, Wd = 0.0;
    for (int c = c_lo; c < c_lo + kc; ++c) {
      const double e = exp(sc_y[c] - mx);
      Z += e;
      Wd = fma(e, sc_ds[c], Wd);
    }
    for (int mask = 1; mask < S; mask <<= 1) { Z += __shfl_xor(Z, mask); Wd += __shfl_xor(Wd, mask); }
    const double mean = Wd / Z;
    double dT = 0.0, sdd = 0.0;
    for (int c = c_lo; c < c_lo + kc; ++c) {
      const double p = exp(sc_y[c] - mx) / Z;
      const double dy = p * (sc_ds[c] - mean);
      dT = fma(dy, -sc_di[c] / scale, dT);
      const double dd = -(double)tg / scale * dy;
      sc_y[c] = dd;
      sdd += dd;
    }
    for (int mask = 1; mask < S; mask <<= 1) sdd += __shfl_xor(sdd, mask);
    tred[tid] = dT;
    __syncthreads();                       // d dist of the tile is in the workspace, the temperature terms in tred
    if (grads) {
      if (tid < m) {
        double s = 0.0;
        for (int r = 0; r < R; ++r)
          for (int q = 0; q < S; ++q) s += tred[r * 4 + tid * S + q];
        sm[UMGM_SLOTS * C + (size_t)k * C + tid] = (float)s;
      }
      // the codebook: the sampled rows of d q, and sum_n d dist 2 (c - h); rows in order
      const double* ddt = b.dist_ws + (size_t)blockIdx.x * R * m * 3 * b.kmax;
      for (int o = tid; o < k * C; o += 256) {
        const int j = o % d, c = (o / d) % k, gg = o / (d * k);
        const float cv = cb[o];
        float acc = 0.f;
        for (int r = 0; r < R; ++r) {
          const float dd = (float)ddt[((size_t)r * m + gg) * 3 * b.kmax + c];
          acc = fmaf(2.f * dd, cv - bufA[r * LD + gg * d + j], acc);
          if (sidx[(l * R + r) * G + gg] == c) acc += bufB[r * LD + gg * d + j];
        }
        sm[UMGM_SLOTS * C + o] = acc;
      }
    }
    __syncthreads();
    // d h = 2 h sum_c d dist - 2 sum_c d dist c, over bufB; thread (row, group, sub) owns C / 4 columns of its group
    {
      const int dj = d / S, j_lo = sub * dj;
      for (int j0 = j_lo; j0 < j_lo + dj; j0 += 16) {
        float acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int c = 0; c < k; ++c) {
          const float dd2 = (float)(-2.0 * sc_y[c]);
          const float* crow = cb + ((size_t)g * k + c) * d + j0;
#pragma unroll
          for (int i4 = 0; i4 < 4; ++i4) {
            const float4 c4 = *reinterpret_cast<const float4*>(crow + 4 * i4);
            acc[4 * i4 + 0] = fmaf(dd2, c4.x, acc[4 * i4 + 0]);
            acc[4 * i4 + 1] = fmaf(dd2, c4.y, acc[4 * i4 + 1]);
            acc[4 * i4 + 2] = fmaf(dd2, c4.z, acc[4 * i4 + 2]);
            acc[4 * i4 + 3] = fmaf(dd2, c4.w, acc[4 * i4 + 3]);
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) bufB[row * LD + g * d + j0 + i] = fmaf((float)(2.0 * sdd), hrow[j0 + i], acc[i]);
      }
    }
    __syncthreads();
    if (grads) spill(bufB, l, UW_DH);
    colsum(bufB, sm + UMGM_Q * C, nullptr);
    if (res) fill(bufA, l, UW_DXN, 0, -1);
    umgm_linear<C>(bufB, TP + UMGM_Q * slot, TP + UMGM_Q * slot + C * C, res ? bufA : nullptr, TP + UMGM_LH * slot, TP + UMGM_LH * slot + C * C,
                   bufA, nullptr, nullptr, 0, 1, m);                                                                                   // d z
    if (grads) spill(bufA, l, UW_DZ);
    colsum(bufA, sm + UMGM_E * C, nullptr);
    umgm_linear<C>(bufA, TP + UMGM_E * slot, TP + UMGM_E * slot + C * C, nullptr, nullptr, nullptr, bufA, nullptr, nullptr, 0, 1, m);      // d x_l
  }

  // ---- dx, every element once; a kept agent's g_restored goes straight through
  if (a.HW > 0) {
    for (int i = tid; i < R * C; i += 256) {
      const int r = i % R, c = i / R;
      if (r < rows_here) {
        const long long gr = row0 + r, ag = gr / a.HW, hw = gr - ag * a.HW;
        const size_t at = ((size_t)ag * C + c) * a.HW + hw;
        float v = bufA[r * LD + c];
        if (b.d_restored != nullptr && a.keep != nullptr && a.keep[ag] != 0) v += b.d_restored[at];
        b.dx[at] = v;
      }
    }
  } else {
    for (int i = tid; i < R * (C / 4); i += 256) {
      const int r = i / (C / 4), c4 = i % (C / 4);
      if (r < rows_here) *reinterpret_cast<float4*>(b.dx + (size_t)(row0 + r) * C + 4 * c4) = *reinterpret_cast<const float4*>(bufA + r * LD + 4 * c4);
    }
  }
}

// bias, codebook and temperature gradients: the per-tile partials added in tile order, written to their places in the gradient blob.
// The temperature goes through LowerBound's rule (codebook_utils.py:28-31): the gradient passes where temperature >= bound or the
// gradient is negative.  The bias slots of the last level's unread LH / S heads and the temperature padding are zeroed.
struct UmgmSmallArgs {
  const float* small_ws;
  const float* params;
  float* dparams;
  long long small_floats, tiles;
  long long small_off[kUmgmMaxLevels], level_off[kUmgmMaxLevels];
  int k[kUmgmMaxLevels];
  int C, m, L;
};
__global__ __launch_bounds__(256) void umgm_bwd_small_kernel(const UmgmSmallArgs a) {
  // 32 elements per workgroup; thread (q, element) adds tiles q, q + 8, .. in order, then the 8 sums are added in order
  __shared__ double part[8][32];
  const int q = threadIdx.x >> 5;
  const long long e = (long long)blockIdx.x * 32 + (threadIdx.x & 31);
  double s = 0.0;
  if (e < a.small_floats)
    for (long long t = q; t < a.tiles; t += 8) s += (double)a.small_ws[t * a.small_floats + e];
  part[q][threadIdx.x & 31] = s;
  __syncthreads();
  if (q != 0 || e >= a.small_floats) return;
  for (int i = 1; i < 8; ++i) s += part[i][threadIdx.x & 31];
  int l = 0;
  while (l + 1 < a.L && e >= a.small_off[l + 1]) ++l;
  const long long el = e - a.small_off[l];
  const int C = a.C;
  const long long slot = (long long)C * C + C;
  float v = (float)s;
  long long at;
  if (el < (long long)UMGM_SLOTS * C) {
    const int sl = (int)(el / C);
    at = a.level_off[l] + sl * slot + (long long)C * C + el % C;
    if (l == a.L - 1 && (sl == UMGM_LH || sl == UMGM_S)) v = 0.f;
  } else if (el < (long long)UMGM_SLOTS * C + (long long)a.k[l] * C) {
    at = a.level_off[l] + UMGM_SLOTS * slot + (el - (long long)UMGM_SLOTS * C);
  } else {
    const int g = (int)(el - (long long)UMGM_SLOTS * C - (long long)a.k[l] * C);
    at = a.level_off[l] + UMGM_SLOTS * slot + (long long)a.k[l] * C + g;
    if (g >= a.m) v = 0.f;
    else if (!(a.params[at] >= 1e-6f || v < 0.f)) v = 0.f;
  }
  a.dparams[at] = v;
}

// ---- dW [Co][Ci] = G^T A over rows, G [rows][Co], A [rows][Ci]: grid (splits, Co / 64 x Ci / 64, matrices); a workgroup owns a 64 x 64
// tile of dW over one row range, and each of its 4 waves the whole tile over a quarter of that range (8 operand loads per 16 matrix
// instructions).  Partial products go to part [matrix][4 split + wave][Co][Ci].
struct RowsWgradArgs {
  const float* G[kRowsWgradMax];
  const float* A[kRowsWgradMax];
  float* out[kRowsWgradMax];
  float* part;
  long long rows, per;
  int Co, Ci, splits, count;
};
__global__ __launch_bounds__(256) void rows_wgrad_kernel(const RowsWgradArgs a) {
  const int bz = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const float* __restrict__ Gp = a.G[bz];
  const float* __restrict__ Ap = a.A[bz];
  const int nti = a.Ci / 64, to = blockIdx.y / nti, ti = blockIdx.y - to * nti;
  const int o0 = to * 64 + lr, i0 = ti * 64 + lr;
  const long long r0 = ((long long)blockIdx.x * 4 + wave) * a.per;   // may lie past the last row: the wave then writes zeros
  const long long r1 = r0 + a.per < a.rows ? r0 + a.per : a.rows;
  f32x4 acc[4][4];
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[s][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
  for (long long r = r0; r < r1; r += 4) {
    const long long rr = r + lk;
    const bool ok = rr < r1;
    float av[4], bv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) av[s] = ok ? Gp[(size_t)rr * a.Co + o0 + 16 * s] : 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) bv[t] = ok ? Ap[(size_t)rr * a.Ci + i0 + 16 * t] : 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[s][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[t], acc[s][t], 0, 0, 0);
  }
  float* part = a.part + ((size_t)bz * 4 * a.splits + 4 * blockIdx.x + wave) * a.Co * a.Ci;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e)   // C/D map: col = lane & 15, row = 4 (lane >> 4) + register
        part[(size_t)(to * 64 + 16 * s + 4 * lk + e) * a.Ci + ti * 64 + 16 * t + lr] = acc[s][t][e];
}
__global__ __launch_bounds__(256) void rows_wgrad_reduce_kernel(const RowsWgradArgs a) {
  const long long per = (long long)a.Co * a.Ci;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= per * a.count) return;
  const int bz = (int)(e / per);
  const long long idx = e - bz * per;
  double s = 0.0;
  for (int sp = 0; sp < 4 * a.splits; ++sp) s += (double)a.part[((size_t)bz * 4 * a.splits + sp) * per + idx];
  a.out[bz][idx] = (float)s;
}

// splits workgroups of 4 waves over the rows; per: rows of a wave, a multiple of 4
inline void rows_wgrad_plan(long long rows, int* splits, long long* per) {
  long long s = (rows + 255) / 256;
  s = s < 1 ? 1 : s > kRowsWgradSplits ? kRowsWgradSplits : s;
  *splits = (int)s;
  *per = ((rows + 4 * s - 1) / (4 * s) + 3) / 4 * 4;
}
inline long long rows_wgrad_scratch_floats(long long rows, int Co, int Ci, int count) {
  int splits;
  long long per;
  rows_wgrad_plan(rows, &splits, &per);
  return (long long)count * 4 * splits * Co * Ci;
}
inline int rows_wgrad_launch(RowsWgradArgs a, hipStream_t st) {
  rows_wgrad_plan(a.rows, &a.splits, &a.per);
  GC_KLOG("rows_wgrad_kernel");
  rows_wgrad_kernel<<<dim3(a.splits, (a.Co / 64) * (a.Ci / 64), a.count), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  const long long total = (long long)a.Co * a.Ci * a.count;
  rows_wgrad_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- workspace of the backward, in floats: transposed weights | row slots | distance scratch | small partials | weight-gradient partials
struct UmgmBwdPlan {
  long long tiles, rows_padded, t_floats, rows_floats, dist_floats, small_floats, small_off[kUmgmMaxLevels], wgrad_floats, total;
  int kmax;
};
inline UmgmBwdPlan umgm_bwd_plan(long long rows, int C, int m, const int* k, int L) {
  UmgmBwdPlan p{};
  p.tiles = (rows + kUmgmRows - 1) / kUmgmRows;
  p.rows_padded = p.tiles * kUmgmRows;
  p.t_floats = (long long)L * UMGM_SLOTS * ((long long)C * C + C);
  p.rows_floats = (long long)L * UW_SLOTS * p.rows_padded * C;
  for (int l = 0; l < L; ++l) {
    p.kmax = k[l] > p.kmax ? k[l] : p.kmax;
    p.small_off[l] = p.small_floats;
    p.small_floats += umgm_small_level_floats(C, k[l]);
  }
  p.dist_floats = 2 * p.rows_padded * m * 3 * p.kmax;   // doubles
  p.wgrad_floats = rows_wgrad_scratch_floats(rows, C, C, 6 * L - 2);
  p.total = p.t_floats + p.rows_floats + p.dist_floats + p.tiles * p.small_floats + p.wgrad_floats;
  return p;
}

inline int umgm_bwd_launch(UmgmBwdArgs b, int C, const int* k, float* dparams, float* workspace, hipStream_t st) {
  UmgmArgs& a = b.f;
  GC_CHECK_ARG(a.n >= 1 && a.n <= (1ll << 31) * kUmgmRows - kUmgmRows, "umgm backward: n must be at least 1 (and at most 2^37 rows)");
  const int L = a.L;
  const UmgmBwdPlan p = umgm_bwd_plan(a.n, C, a.m, k, L);
  long long po = 0, fo = 0;
  for (int l = 0; l < L; ++l) {
    a.k[l] = k[l];
    a.level_off[l] = po;
    a.field_off[l] = fo;
    b.small_off[l] = p.small_off[l];
    po += umgm_level_floats(C, k[l]);
    fo += a.n * a.m * k[l];
  }
  float* tparams = workspace;
  b.tparams = tparams;
  b.rows_ws = tparams + p.t_floats;
  b.dist_ws = reinterpret_cast<double*>(b.rows_ws + p.rows_floats);
  b.small_ws = b.rows_ws + p.rows_floats + p.dist_floats;
  float* wpart = b.small_ws + p.tiles * p.small_floats;
  b.rows_padded = p.rows_padded;
  b.small_floats = p.small_floats;
  b.kmax = p.kmax;

  GC_KLOG("umgm_transpose_kernel");
  umgm_transpose_kernel<<<(unsigned)std::min<long long>((p.t_floats + 255) / 256, 1 << 16), 256, 0, st>>>(a.params, tparams, a.level_off[0], a.level_off[1],
                                                                                                        a.level_off[2], C, L);
  GC_HIP(hipGetLastError());
  const unsigned blocks = (unsigned)p.tiles;
  const int smem = umgm_smem_bytes(C);
  static LdsAttrOnce attr[3];
  if (C == 64) {
    if (int rc = attr[0].set(umgm_bwd_kernel<64>, smem)) return rc;
    GC_KLOG("umgm_bwd_kernel<64>");
    umgm_bwd_kernel<64><<<blocks, 256, smem, st>>>(b);
  } else if (C == 128) {
    if (int rc = attr[1].set(umgm_bwd_kernel<128>, smem)) return rc;
    GC_KLOG("umgm_bwd_kernel<128>");
    umgm_bwd_kernel<128><<<blocks, 256, smem, st>>>(b);
  } else {
    if (int rc = attr[2].set(umgm_bwd_kernel<256>, smem)) return rc;
    GC_KLOG("umgm_bwd_kernel<256>");
    umgm_bwd_kernel<256><<<blocks, 256, smem, st>>>(b);
  }
  GC_HIP(hipGetLastError());
  if (b.dx_only) return GC_OK;

  const size_t slot = (size_t)C * C + C;
  UmgmSmallArgs s{};
  s.small_ws = b.small_ws; s.params = a.params; s.dparams = dparams; s.small_floats = p.small_floats; s.tiles = p.tiles; s.C = C; s.m = a.m; s.L = L;
  for (int l = 0; l < L; ++l) { s.small_off[l] = p.small_off[l]; s.level_off[l] = a.level_off[l]; s.k[l] = k[l]; }
  GC_KLOG("umgm_bwd_small_kernel");
  umgm_bwd_small_kernel<<<(unsigned)((p.small_floats + 31) / 32), 256, 0, st>>>(s);
  GC_HIP(hipGetLastError());

  RowsWgradArgs w{};
  w.part = wpart; w.rows = a.n; w.Co = C; w.Ci = C;
  auto rows_at = [&](int l, int sl) { return b.rows_ws + ((size_t)l * UW_SLOTS + sl) * p.rows_padded * C; };
  auto pair = [&](int l, int head, int gs, int al, int as) {
    w.G[w.count] = rows_at(l, gs); w.A[w.count] = rows_at(al, as); w.out[w.count] = dparams + a.level_off[l] + head * slot; ++w.count;
  };
  for (int l = 0; l < L; ++l) {
    pair(l, UMGM_E, UW_DZ, l, UW_X);
    pair(l, UMGM_Q, UW_DH, l, UW_Z);
    pair(l, UMGM_DH, UW_DT, l, UW_Q);
    pair(l, UMGM_R, UW_DF, l, UW_T);
    if (l < L - 1) {
      pair(l, UMGM_LH, UW_DXN, l, UW_Z);
      pair(l, UMGM_S, UW_DT, l + 1, UW_F);
    } else {   // the unread heads of the last level
      GC_HIP(hipMemsetAsync(dparams + a.level_off[l] + UMGM_LH * slot, 0, (size_t)C * C * sizeof(float), st));
      GC_HIP(hipMemsetAsync(dparams + a.level_off[l] + UMGM_S * slot, 0, (size_t)C * C * sizeof(float), st));
    }
  }
  return rows_wgrad_launch(w, st);
}

}  // namespace gc
