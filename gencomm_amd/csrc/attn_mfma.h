// The fp32 matrix-core attention tile (v_mfma_f32_32x32x2_f32: exact fp32 products, an fmaf chain), written once: a wave owns 32
// columns (queries; keys in the key pass of the backward) and walks the other side in blocks of 32 staged as LDS rows,
//   S^T[row][col] = R C^T      A = the rows from LDS, B = the lane's column operand from registers; the 32 x 32 block comes out with a
//                              lane owning ONE column (lane & 31) and 16 of the 32 rows (the others in lane ^ 32), so softmax statistics
//                              are register-local plus one exchange;
//   O^T[d][col] += R'^T P      A = value rows from LDS in the row order the P registers already have, B = P straight from the registers.
// Used by win_attn_mfma_kernel (v2xvit_kernels.h), swap_attn_kernel (swap_attn_kernels.h), swap_attn_bwd_q_kernel and
// swap_attn_bwd_k_kernel (swap_attn_bwd_kernels.h) and attn_flash_mfma_kernel (attn_kernels.h), which live in different translation
// units: device functions only, no kernel is defined here.  Staging, masks, biases and what a kernel does with the result stay with it.
//   mfma_row            which row of the block accumulator register r holds
//   mfma_scores[2]      the score chain over DH / 2 steps; two interleaved accumulators in the backward
//   mfma_softmax_step   one block of the running softmax: max, exchange, exp, denominator, rescale of O
//   mfma_apply[2]       the apply chain over the 16 P registers and DV / 32 accumulators; the dV / dK pair in the key pass
//   mfma_store_t        O^T to channel-strided memory, channels beyond DH masked
// The softmax arithmetic is a template parameter: swap_attn_kernel uses expf, the window and UNet kernels __expf (mfma_softmax_step);
// one flavour for all would change output bits.
// The score and probability blocks travel BY VALUE (returned, or passed as f32x16): a block whose address is handed to a helper inside
// the key loop costs swap_attn_bwd_q_kernel<16, 4> two VGPRs and with them a wave per SIMD.
#pragma once
#include "common.h"

namespace gc {

using f32x16 = __attribute__((ext_vector_type(16))) float;   // one 32 x 32 block: 16 rows of one column per lane
struct f32x16x2 { f32x16 a, b; };

// Row of the 32 x 32 block in accumulator register r of lane half h = lane >> 5 (its column is lane & 31), counted from the block's first
// row row0.  The sum is grouped as (row0 + 4 h) + a constant per register ON PURPOSE: the callers divide it by window sizes, and this
// grouping lets the compiler fold those divisions per register (with row0 added last the ws 4 swap kernels need up to 30 more VGPRs;
// with the register's two terms apart, swap_attn_kernel<16, 8> loses a wave per SIMD).
__device__ __forceinline__ constexpr int mfma_row(int r, int h, int row0 = 0) { return row0 + 4 * h + (8 * (r >> 2) + (r & 3)); }

__device__ __forceinline__ f32x16 mfma_zero() { return f32x16{}; }

// R C^T over DH channels: row = the lane's LDS row (lane & 31) + h, b[s] = channel 2 s + h of the lane's column.
template <int DH>
__device__ __forceinline__ f32x16 mfma_scores(const float* row, const float (&b)[DH / 2]) {
  f32x16 acc = mfma_zero();
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(row[2 * s], b[s], acc, 0, 0, 0);
  return acc;
}

// Two score chains at once (S and dP of the backward): the two independent accumulators alternate.
template <int DH>
__device__ __forceinline__ f32x16x2 mfma_scores2(const float* row0, const float (&b0)[DH / 2], const float* row1, const float (&b1)[DH / 2]) {
  f32x16x2 acc = {mfma_zero(), mfma_zero()};
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) {
    acc.a = __builtin_amdgcn_mfma_f32_32x32x2f32(row0[2 * s], b0[s], acc.a, 0, 0, 0);
    acc.b = __builtin_amdgcn_mfma_f32_32x32x2f32(row1[2 * s], b1[s], acc.b, 0, 0, 0);
  }
  return acc;
}

// One block of the running softmax.  The caller has filled sc with the block's scores (bias added, masked rows -inf; at least one row
// of the block finite); sc becomes P = exp(sc - new max), and the denominator and O are rescaled to the new max.
// FAST = the arithmetic of the window and UNet kernels: __expf, and the denominator update as one fma.  !FAST = that of the swap
// kernels: expf, and the product rounded on its own (those kernels are compiled with contraction off, swap_attn_kernels.h).  The choice
// is spelled out here so that it does not follow from where this header happens to be included.
template <bool FAST, int NB>
__device__ __forceinline__ void mfma_softmax_step(f32x16& sc, float& mrun, float& den, f32x16 (&o)[NB]) {
#pragma clang fp contract(off)
  auto ex = [](float x) { return FAST ? __expf(x) : expf(x); };
  float bm = -INFINITY;
#pragma unroll
  for (int r = 0; r < 16; ++r) bm = fmaxf(bm, sc[r]);
  bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
  const float nm = fmaxf(mrun, bm), corr = ex(mrun - nm);
  float ps = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) { sc[r] = ex(sc[r] - nm); ps += sc[r]; }
  den = FAST ? fmaf(den, corr, ps) : den * corr + ps;
  mrun = nm;
#pragma unroll
  for (int db = 0; db < NB; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[db][i] *= corr;
}

// o[db] += R'^T P over the block's 32 rows: rows = row 0 of the staged tile + (lane & 31), LD its stride, row0 the block's first row,
// channels 32 db .. 32 db + 31.
// The 32-wide halves alternate: consecutive MFMAs never share an accumulator when NB > 1.
template <int NB, int LD>
__device__ __forceinline__ void mfma_apply(const float* rows, int row0, int h, f32x16 p, f32x16 (&o)[NB]) {
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int db = 0; db < NB; ++db) o[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(rows[mfma_row(t, h, row0) * LD + 32 * db], p[t], o[db], 0, 0, 0);
}

// Two apply chains at once (dV and dK of the key pass), alternating.
template <int NB, int LD>
__device__ __forceinline__ void mfma_apply2(const float* rows0, const float* rows1, int row0, int h, f32x16 p0, f32x16 p1, f32x16 (&o0)[NB],
                                            f32x16 (&o1)[NB]) {
#pragma unroll
  for (int t = 0; t < 16; ++t)
#pragma unroll
    for (int db = 0; db < NB; ++db) {
      o0[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(rows0[mfma_row(t, h, row0) * LD + 32 * db], p0[t], o0[db], 0, 0, 0);
      o1[db] = __builtin_amdgcn_mfma_f32_32x32x2f32(rows1[mfma_row(t, h, row0) * LD + 32 * db], p1[t], o1[db], 0, 0, 0);
    }
}

// p[ch * stride] = f(O^T[ch][the lane's column]) for the channels ch < DH (DH = 16: rows 16 .. 31 of the block are padding).
template <int DH, int NB, class F>
__device__ __forceinline__ void mfma_store_t(float* p, size_t stride, int h, const f32x16 (&o)[NB], F f) {
#pragma unroll
  for (int db = 0; db < NB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (DH >= 32 || (r >> 2) < DH / 8) p[(size_t)(32 * db + mfma_row(r, h)) * stride] = f(o[db][r]);
}

}  // namespace gc
