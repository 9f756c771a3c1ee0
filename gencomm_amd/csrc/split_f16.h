// The exact fp16 split: fp32-grade products on the f16 matrix pipe.  One home for the operand splits, the power-of-two scales and the
// prepared weight-table entry of every kernel that uses them: conv8h_kernels.h, conv8h8_kernels.h, latenth_kernels.h, conv_h3_kernels.h,
// wgrad_h3_kernels.h, conv_kernels.h, enhancer_kernels.h, sparse_kernels.h.
//
// Arithmetic (three terms: every operand carries all 24 bits of its fp32 value).  An activation x is split EXACTLY into three
// terms x = hi + lo + t: hi = fp16(x), lo = fp16(x - hi), t = x - hi - lo (each difference is exact in fp32; t is 0 or
// +-1 unit in the last place of x, i.e. a power of two, because two 11-bit terms and the sign of lo cover 23 of the 24
// bits).  hi and lo are fp16 operands, t -- scaled by 2^20 (HC_TSCALE) -- a bf8 (e5m2) one, where a power of two is exact.  A weight w
// (pre-scaled by a power of two so that the largest lies in [2^13, 2^14): block_weight_scale) is split the same way
// into three fp16 terms w1 + w2 + w3 (exact) and additionally rounded once to bf8, wb = bf8(w 2^-20).  A product block is
// SIX matrix instructions into fp32 accumulators:
//     hi w1 + lo w1 + hi w2 + lo w2 + hi w3        (five fp16 MFMAs: every fp16 x fp16 product exact)
//   + t  wb                                        (one bf8 MFMA: the 2^-23-sized term to 3 bits)
// The terms left out are lo w3, t w2, t w3 (<= 2^-33 |x w|) and the bf8 rounding of w in the last one
// (2^-23 * 2^-3 = 2^-26 |x w|): a product is accurate to 2^-26 -- finer than the 2^-24 rounding of the fp32 accumulation
// that the reference's own arithmetic has.  The two-term form (split_pair / split8, mfma_split3: hi w1 + hi w2 + lo w1) leaves
// 2^-22 |x w| per product: "22-bit products".  t is carried for |x| >= 2^-12 (below: absolute error <= 2^-36 per product), w3 for
// |w| >= 2^-14 max|w|.
//
// Range guard.  A split x = hi + lo needs |x| < 65504:
//  * kernels whose operands are RAW tensors (conv_in's x_t / message channels, the Upsample conv's input, the unit-test
//    entry) scale them by an exact power of two 2^-k chosen from a device-side bound on max|x| (act_scale, common.h: k = 0, i.e. no
//    change at all, while the bound is below 2^14) and undo it in the epilogue -- the result is the fp32 one at any
//    input magnitude a float can hold; the general convolutions carry a RUNNING scale instead (RunScale below);
//  * operands that are GroupNorm / LayerNorm outputs are bounded by |gamma| sqrt(group size) + |beta| whatever the
//    input; every split kernel additionally runs with MODE.FP16_OVFL = 1 (fp16_ovfl_clamp, common.h), under which an overflowing
//    f32 -> f16 conversion saturates to +-65504 instead of producing inf: a pathological gamma degrades accuracy, it cannot
//    create inf / NaN out of finite inputs.
//
// Contraction: this header is compiled under the build's default (fast).  A `#pragma clang fp contract` governs the function an
// expression is WRITTEN in, so a caller pinned to `off` (sparse_kernels.h) multiplies by its scale itself and hands the products in.
#pragma once
#include "common.h"

namespace gc {

constexpr float HC_TSCALE = 1048576.0f;      // 2^20: t is stored as bf8(t 2^20), the bf8 weight as bf8(w 2^-20)

// exact two-term fp16 split of a pair of floats: hi = rne16(x), lo = rne16(x - hi)
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {
  const half2_t h = __builtin_convertvector((float2_t){a, b}, half2_t);
  const float ra = a - (float)h[0], rb = b - (float)h[1];
  const half2_t l = __builtin_convertvector((float2_t){ra, rb}, half2_t);
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ void split_one(float a, uint16_t& hi, uint16_t& lo) {
  const _Float16 h = (_Float16)a;
  const _Float16 l = (_Float16)(a - (float)h);
  hi = __builtin_bit_cast(uint16_t, h);
  lo = __builtin_bit_cast(uint16_t, l);
}
// the same of eight floats times `mul`: four packed pairs per term (one 16-byte LDS record piece each).  Under this header's contraction
// the product and the first subtraction fuse: a caller pinned to `off` (sparse_kernels.h) forms the products itself, pair by pair.
__device__ __forceinline__ void split8(const float (&v)[8], float mul, uint4& hi, uint4& lo) {
  split_pair(v[0] * mul, v[1] * mul, hi.x, lo.x);
  split_pair(v[2] * mul, v[3] * mul, hi.y, lo.y);
  split_pair(v[4] * mul, v[5] * mul, hi.z, lo.z);
  split_pair(v[6] * mul, v[7] * mul, hi.w, lo.w);
}

// 1.0f the optimiser cannot see through: fma(x, one, -fp16) stays a fused multiply-add and is selected as ONE v_fma_mix_f32 (an fp16
// operand read in place); written as x - (float)h it becomes v_cvt_f32_f16 + v_sub_f32.  One s_mov per kernel (the asm is pure: CSE'd).
__device__ __forceinline__ float hc_one() {
  float o;
  asm("s_mov_b32 %0, 1.0" : "=s"(o));
  return o;
}
// exact three-term split of a pair: hi / lo packed fp16 pairs, ta / tb = the third terms, UNSCALED: the 2^20 rides inside the
// conversion to bf8 (bf8x2s / bf8x4s: v_cvt_scalef32_pk_bf8_f32 divides by its scale operand 2^-20 -- one multiply per element less)
// 7 vector instructions per pair: 2 packed conversions + 4 v_fma_mix_f32 (+ the bf8 conversion at the caller).
__device__ __forceinline__ void split3_pair(float a, float b, uint32_t& hi, uint32_t& lo, float& ta, float& tb) {
  const float one = hc_one();
  const half2_t h = __builtin_convertvector((float2_t){a, b}, half2_t);
  const float ra = fmaf(a, one, -(float)h[0]), rb = fmaf(b, one, -(float)h[1]);
  const half2_t l = __builtin_convertvector((float2_t){ra, rb}, half2_t);
  ta = fmaf(ra, one, -(float)l[0]);
  tb = fmaf(rb, one, -(float)l[1]);
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}
// The same for PRODUCTS za ra, zb rb (the GroupNorm + SiLU staging of conv8h_kernels.h forms its activation as such a product): hi =
// fp16 of the rounded product, first residual = fma(z, r, -hi) -- the exact product minus hi, rounded once -- and on from there as above.
__device__ __forceinline__ void split3_prod_pair(float za, float ra, float zb, float rb, uint32_t& hi, uint32_t& lo, float& ta, float& tb) {
  const float one = hc_one();
  const half2_t h = __builtin_convertvector((float2_t){za * ra, zb * rb}, half2_t);
  const float qa = fmaf(za, ra, -(float)h[0]), qb = fmaf(zb, rb, -(float)h[1]);
  const half2_t l = __builtin_convertvector((float2_t){qa, qb}, half2_t);
  ta = fmaf(qa, one, -(float)l[0]);
  tb = fmaf(qb, one, -(float)l[1]);
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}
// The three-term split with plain subtractions (no hc_one: weight preparation and the Enhancer's staging, whose schedules were taken on
// this form).  split3_sub_pair leaves the third terms as floats, split3w_pair rounds them to the third fp16 term of a weight.
__device__ __forceinline__ void split3_sub_pair(float a, float b, uint32_t& hi, uint32_t& lo, float& ta, float& tb) {
  const half2_t h = __builtin_convertvector((float2_t){a, b}, half2_t);
  const float ra = a - (float)h[0], rb = b - (float)h[1];
  const half2_t l = __builtin_convertvector((float2_t){ra, rb}, half2_t);
  ta = ra - (float)l[0];
  tb = rb - (float)l[1];
  hi = __builtin_bit_cast(uint32_t, h);
  lo = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ void split3w_pair(float a, float b, uint32_t& w1, uint32_t& w2, uint32_t& w3) {
  float ta, tb;
  split3_sub_pair(a, b, w1, w2, ta, tb);
  w3 = __builtin_bit_cast(uint32_t, __builtin_convertvector((float2_t){ta, tb}, half2_t));
}

// two / four scaled third terms -> bf8 bytes (v_cvt_pk_bf8_f32: OCP e5m2, round to nearest even; powers of two are exact)
__device__ __forceinline__ uint32_t bf8x2(float a, float b) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false) & 0xffffu;
}
__device__ __forceinline__ uint32_t bf8x4(float a, float b, float c, float d) {
  int v = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
  v = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, v, true);
  return (uint32_t)v;
}

// the same for UNSCALED third terms: bf8(t 2^20) through the scaled conversion of gfx950 (value / scale, scale = 2^-20; checked
// bit for bit against multiply + convert on hardware)
__device__ __forceinline__ uint32_t bf8x2s(float a, float b) {
  const short2_t v = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32((short2_t){0, 0}, a, b, 1.0f / HC_TSCALE, false);
  return (uint32_t)(uint16_t)v[0];
}
__device__ __forceinline__ uint32_t bf8x4s(float a, float b, float c, float d) {
  // (an undefined "old" operand instead of the zero fill -- an empty volatile asm -- saves two v_mov per pixel and was measured 3.5 %
  // SLOWER in latent_step_h_kernel, where the volatile statements pin the schedule: profiles/r5_conv8h_valu_diet.txt)
  short2_t u = {0, 0};
  short2_t v = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(u, a, b, 1.0f / HC_TSCALE, false);
  v = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(v, c, d, 1.0f / HC_TSCALE, true);
  return __builtin_bit_cast(uint32_t, v);
}

// ---- prepared weight table of a tap group: [term 3][lane 64][4 dwords] fp16 (channels 2d, 2d + 1 in dword d), then [lane 64][2 dwords]
// bf8 of w 2^-20 (channel k in byte k) = 896 dwords.  wtab_entry = dword q of it, from the eight SCALED weights of (group, wtab_lane(q));
// wtab_pair / wtab_bf8 are its two halves for callers that store from both branches (merged into one store their code changes).
__device__ __forceinline__ int wtab_lane(int q) { return q < 768 ? (q >> 2) & 63 : (q - 768) >> 1; }
__device__ __forceinline__ uint32_t wtab_pair(int q, const float (&wv)[8]) {   // q < 768: the term-selected fp16 pair
  const int d = q & 3, term = q >> 8;
  uint16_t v[2];
  for (int e = 0; e < 2; ++e) {
    const float x = wv[2 * d + e];
    const _Float16 w1 = (_Float16)x;
    const float r1 = x - (float)w1;
    const _Float16 w2 = (_Float16)r1;
    const _Float16 w3 = (_Float16)(r1 - (float)w2);
    v[e] = __builtin_bit_cast(uint16_t, term == 0 ? w1 : term == 1 ? w2 : w3);
  }
  return (uint32_t)v[0] | ((uint32_t)v[1] << 16);
}
__device__ __forceinline__ uint32_t wtab_bf8(int q, const float (&wv)[8]) {    // q >= 768: the bf8 quad
  const int d = (q - 768) & 1;
  const float k = 1.0f / HC_TSCALE;
  return bf8x4(wv[4 * d] * k, wv[4 * d + 1] * k, wv[4 * d + 2] * k, wv[4 * d + 3] * k);
}
__device__ __forceinline__ uint32_t wtab_entry(int q, const float (&wv)[8]) { return q < 768 ? wtab_pair(q, wv) : wtab_bf8(q, wv); }

// ---- scales ----
// the power of two that puts `mx` (> 0, finite) into [2^13, 2^14), its exponent clamped to [lo, hi]
__device__ __forceinline__ float pow2_scale(float mx, int hi, int lo) {
  int e;
  (void)frexpf(mx, &e);  // mx = f * 2^e, f in [0.5, 1)
  return ldexpf(1.0f, max(min(14 - e, hi), lo));
}
// max over a workgroup of 256 threads (1 KB of LDS of its own: handed in by reference the caller's array would arrive as a generic pointer)
__device__ __forceinline__ float block_max256(float m) {
  __shared__ float s_max[256];
  const int tid = threadIdx.x;
  s_max[tid] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) s_max[tid] = fmaxf(s_max[tid], s_max[tid + s]);
    __syncthreads();
  }
  return s_max[0];
}
// Weight scale of a prepared table: the power of two that puts the largest weight in [2^13, 2^14): the third terms of weights down to
// 2^-14 of the largest stay on fp16's 2^-24 grid (exact), the bf8 copies (x 2^-20) of weights down to 2^-7 of it stay normal;
// all-zero weights -> scale 1.  m = this thread's max |w|.
__device__ __forceinline__ float block_weight_scale(float m) {
  const float wmax = block_max256(m);
  int ex = 0;
  if (wmax > 0.f) (void)frexpf(wmax, &ex);  // wmax = f * 2^ex, f in [0.5, 1)
  return wmax > 0.f ? ldexpf(1.0f, 14 - ex) : 1.0f;
}
// Running activation scale of a K loop: the power of two that puts the largest |x| seen so far into [2^13, 2^14) (fp16 max 65504; small
// inputs -- gradients -- are scaled UP so that their low parts stay normal fp16 numbers), workgroup-uniform.  `row` = the four waves'
// maxima of the next chunk.  When the scale moves -- the exponent grew, or this is the first non-zero chunk -- the caller multiplies what
// it has accumulated by new / old (exact).  The compare and the rescale stay in the caller: behind a function boundary either one costs the
// chunk loop an instruction (a select for "unchanged", a second test of the returned ratio).
struct RunScale {
  float xs = 1.0f, run_max = 0.f;   // xs: the scale the caller's accumulators are in
  __device__ __forceinline__ float fold(const float (&row)[4]) {
    run_max = fmaxf(run_max, fmaxf(fmaxf(row[0], row[1]), fmaxf(row[2], row[3])));
    return run_max;
  }
  // the scale after `row`; `prev` while everything seen is zero
  __device__ __forceinline__ float next(const float (&row)[4], float prev, int hi, int lo) {
    if (!(fold(row) > 0.f)) return prev;
    return pow2_scale(run_max, hi, lo);
  }
};

// ---- the two-term product block: hi hi + hi lo + lo hi on v_mfma_f32_32x32x16_f16 ----
template <class Acc>
__device__ __forceinline__ void mfma_split3(half8_t ah, half8_t al, half8_t bh, half8_t bl, Acc& acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
}

}  // namespace gc
