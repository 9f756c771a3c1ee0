// Backward of swap_attn_kernel (swap_attn_kernels.h): the adjoint of the joint softmax over agent x window tokens with masked keys,
// of the 3-D relative position bias table and of q, k and v.  With P_ij = exp(s_ij - lse_i) (s = q k^T scale + bias, lse from the
// TRAIN instantiation of the forward):
//   D_i = sum_d dO_id O_id    dP_ij = dO_i . v_j    dS_ij = P_ij (dP_ij - D_i)
//   dQ_i = scale sum_j dS_ij k_j    dK_j = scale sum_i dS_ij q_i    dV_j = sum_i P_ij dO_i    dtable[rel(i, j)][head] += dS_ij
// Two passes, no T x T matrix in memory (320 x 320 per group and head at L 5, ws 8): each pass recomputes S on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32) on the tile of attn_mfma.h, a wave owning 32 columns and a lane one column and 16 of the 32 rows:
//   swap_attn_bwd_q_kernel   wave = 32 queries; K and V staged in tiles of 64 keys, the key loop ends at the last valid agent.
//                            S^T = K Q^T and dP^T = V dO^T (A = rows from LDS, B = the wave's q / dO from registers), then
//                            dQ^T[d][query] += K^T dS (A = K rows in the key order the dS registers have).  dS is also added into the
//                            workgroup's copy of the table gradient in LDS (LDS float atomics), flushed with global float atomics:
//                            dtable is ACCUMULATED and its summation order is NOT fixed.
//   swap_attn_bwd_k_kernel   wave = 32 keys; Q (scaled), dO, lse and D staged in tiles of 64 queries (D is summed by the thread that
//                            stages the dO row, from dO and O).  S = Q K^T and dP = dO V^T (A = Q / dO rows, B = the wave's k / v),
//                            dV^T[d][key] += dO^T P, dK^T[d][key] += (scale Q)^T dS.  Key blocks of masked agents skip the
//                            arithmetic and store exact zeros; ALL L agents' queries are walked (padded agents are queries too).
// Every element of dqkv is stored exactly once (q rows by the first kernel, k and v rows by the second), nothing is read from it.
// Workgroups, the split of groups of more than 256 tokens and the LDS row stride (odd: DV + 1) are the forward's; the order in which
// the groups are dealt to the workgroup ids is not (SwapBwdArgs::xcd, swap_attn_bwd_launch).
#pragma once
#include "swap_attn_kernels.h"

namespace gc {

#pragma clang fp contract(off)   // as in swap_attn_kernels.h

struct SwapBwdArgs {
  const float* qkv;     // [B * L][3 * inner][H][W]
  const float* table;   // [(2 L - 1)(2 WS - 1)^2][heads]
  const int* nvalid;    // [B]
  const float* out;     // [B * L][inner][H][W], the forward's output
  const float* lse;     // [B * L][heads][H][W]
  const float* dout;    // [B * L][inner][H][W]
  float* dqkv;          // [B * L][3 * inner][H][W]
  float* dtable;        // accumulated
  int L, heads, H, W, grid_mode;
  int nblk, wpc;        // blocks of 32 tokens per group; blocks (= waves) per workgroup
  int xcd;              // != 0: workgroup ids are dealt so that neighbouring groups run on the same XCD (they share cache lines)
  float scale;
};

// The group a workgroup id is dealt (SwapBwdArgs::xcd): XCD k = blockIdx.x & 7 walks the k-th eighth of the groups.
__device__ __forceinline__ int swap_bwd_bx(const SwapBwdArgs& a) {
  return a.xcd ? (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3) : blockIdx.x;
}

template <int DH, int WS>
__global__ __launch_bounds__(512) void swap_attn_bwd_q_kernel(const SwapBwdArgs a) {
  constexpr int T1 = WS * WS, KT = 64, DV = DH < 32 ? 32 : DH, LD = DV + 1, PW = 2 * WS - 1, PW2 = PW * PW;
  extern __shared__ float swb_smem[];  // K [KT][LD], V [KT][LD] (columns DH .. 31 zero when DH < 32), bias and its gradient [(2 L - 1) PW2] each
  const SwapGroup<DH, WS> g(a, a.nblk, swap_bwd_bx(a));
  const int m = g.m, b = g.b, L = g.L, T = g.T, TV = g.TV, inner = g.inner, HW = g.HW, NP = (2 * L - 1) * PW2;
  float* sK = swb_smem;
  float* sV = sK + KT * LD;
  float* sP = sV + KT * LD;
  float* sD = sP + NP;
  const int tid = threadIdx.x, nthr = blockDim.x;

  for (int i = tid; i < NP; i += nthr) {
    sP[i] = a.table[(size_t)i * a.heads + m];
    sD[i] = 0.f;
  }
  if (DV != DH)
    for (int i = tid; i < 2 * KT * LD; i += nthr) sK[i] = 0.f;   // K and V: the columns beyond DH are never written again

  const int wave = tid >> 6, lane = tid & 63, qi = lane & 31, h = lane >> 5;
  const int qb = g.chunk * a.wpc + wave;
  const bool wave_live = wave < a.wpc && qb < a.nblk;
  const int qtok = qb * 32 + qi;
  const bool qok = wave_live && qtok < T;
  const int qt = qok ? qtok : 0;
  const int ql = qt / T1, qh = (qt % T1) / WS, qw = qt % WS;
  const int qpix = g.pixel(qh, qw);
  const size_t orow = ((size_t)(b * L + ql) * inner + m * DH) * HW + qpix;
  float qv[DH / 2], gv[DH / 2];
  float D = 0.f;
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) {
    qv[s] = qok ? g.base[ql * g.agent + (size_t)(m * DH + 2 * s + h) * HW + qpix] * a.scale : 0.f;
    gv[s] = qok ? a.dout[orow + (size_t)(2 * s + h) * HW] : 0.f;
    D = fmaf(gv[s], qok ? a.out[orow + (size_t)(2 * s + h) * HW] : 0.f, D);
  }
  D += __shfl_xor(D, 32, 64);
  const float lse = qok ? a.lse[((size_t)(b * L + ql) * a.heads + m) * HW + qpix] : 0.f;
  f32x16 dq[DV / 32];
#pragma unroll
  for (int db = 0; db < DV / 32; ++db) dq[db] = mfma_zero();
  const int pbase = (ql + L - 1) * PW2 + (qh + WS - 1) * PW + (qw + WS - 1);

  for (int k0 = 0; k0 < TV; k0 += KT) {
    __syncthreads();
    swap_fill_kv<DH, WS, LD, LD>(g, k0, sK, sV);
    __syncthreads();
    if (!wave_live) continue;
    const int nkb = (min(KT, TV - k0) + 31) >> 5;
#pragma unroll 1
    for (int kb = 0; kb < nkb; ++kb) {
      const f32x16x2 sd = mfma_scores2<DH>(sK + (32 * kb + qi) * LD + h, qv, sV + (32 * kb + qi) * LD + h, gv);
      f32x16 sc = sd.a, dp = sd.b;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = mfma_row(r, h, k0 + 32 * kb);
        const bool kok = qok && key < TV;
        const int pi = kok ? pbase - g.rel_off(key) : 0;
        const float p = kok ? expf(sc[r] + sP[pi] - lse) : 0.f;
        const float ds = p * (dp[r] - D);
        sc[r] = ds;
        if (kok) atomicAdd(&sD[pi], ds);
      }
      mfma_apply<DV / 32, LD>(sK + qi, 32 * kb, h, sc, dq);
    }
  }
  if (qok)
    mfma_store_t<DH>(a.dqkv + (size_t)(b * L + ql) * g.agent + (size_t)(m * DH) * HW + qpix, HW, h, dq, [&](float x) { return x * a.scale; });
  __syncthreads();
  for (int i = tid; i < NP; i += nthr)
    if (sD[i] != 0.f) atomicAdd(&a.dtable[(size_t)i * a.heads + m], sD[i]);
}

template <int DH, int WS>
__global__ __launch_bounds__(512) void swap_attn_bwd_k_kernel(const SwapBwdArgs a) {
  constexpr int T1 = WS * WS, QT = 64, DV = DH < 32 ? 32 : DH, LD = DV + 1, PW = 2 * WS - 1, PW2 = PW * PW;
  constexpr int CH = DH < 32 ? DH : 32;
  extern __shared__ float swb_smem[];  // Q scaled [QT][LD], dO [QT][LD] (columns DH .. 31 zero when DH < 32), lse [QT], D [QT], bias [(2 L - 1) PW2]
  const SwapGroup<DH, WS> g(a, a.nblk, swap_bwd_bx(a));
  const int m = g.m, b = g.b, L = g.L, T = g.T, TV = g.TV, inner = g.inner, HW = g.HW, NP = (2 * L - 1) * PW2;
  float* sQ = swb_smem;
  float* sG = sQ + QT * LD;
  float* sL = sG + QT * LD;
  float* sDd = sL + QT;
  float* sP = sDd + QT;
  const int tid = threadIdx.x, nthr = blockDim.x;

  for (int i = tid; i < NP; i += nthr) sP[i] = a.table[(size_t)i * a.heads + m];
  if (DV != DH)
    for (int i = tid; i < 2 * QT * LD; i += nthr) sQ[i] = 0.f;

  // wave = one block of 32 keys (lanes l and l + 32 share a key)
  const int wave = tid >> 6, lane = tid & 63, qi = lane & 31, h = lane >> 5;
  const int kb = g.chunk * a.wpc + wave;
  const bool wave_live = wave < a.wpc && kb < a.nblk;
  const int ktok = kb * 32 + qi;
  const bool kok = wave_live && ktok < T;          // a key of the group: its dK and dV rows are stored here
  const bool kvalid = kok && ktok < TV;            // ... and of an agent that is present
  const bool wave_work = wave_live && kb * 32 < TV;   // wave-uniform: the block's first key is valid
  const int kt = kok ? ktok : 0;
  const int kl = kt / T1, kh = (kt % T1) / WS, kw = kt % WS;
  const int kpix = g.pixel(kh, kw);
  float kv[DH / 2], vv[DH / 2];
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) {
    kv[s] = kvalid ? g.base[kl * g.agent + (size_t)(inner + m * DH + 2 * s + h) * HW + kpix] : 0.f;
    vv[s] = kvalid ? g.base[kl * g.agent + (size_t)(2 * inner + m * DH + 2 * s + h) * HW + kpix] : 0.f;
  }
  f32x16 dk[DV / 32], dv[DV / 32];
#pragma unroll
  for (int db = 0; db < DV / 32; ++db) {
    dk[db] = mfma_zero();
    dv[db] = mfma_zero();
  }
  // rel(query, key) = off(query) + pk with pk = (L - 1 - kl) PW2 + (WS - 1 - kh) PW + (WS - 1 - kw)
  const int pk = (L - 1 - kl) * PW2 + (WS - 1 - kh) * PW + (WS - 1 - kw);
  const int qend = g.chunk * a.wpc * 32 < TV ? T : 0;   // a workgroup whose keys are all masked stages nothing

  for (int q0 = 0; q0 < qend; q0 += QT) {
    __syncthreads();
    for (int e = tid; e < 2 * QT; e += nthr) {   // one (query, Q or dO) row per pass; rows beyond the group's tokens become zero rows
      const int row = e & (QT - 1), isg = e / QT, tok = q0 + row;
      const bool live = tok < T;
      const int t = live ? tok : 0;
      const int tl = t / T1, pix = g.pixel((t % T1) / WS, t % WS);
      if (!isg) {
        const float* __restrict__ src = g.base + tl * g.agent + (size_t)(m * DH) * HW + pix;
        swap_fill_row<DH>(sQ + row * LD, live, [&](int c) { return src[(size_t)c * HW] * a.scale; });
        sL[row] = live ? a.lse[((size_t)(b * L + tl) * a.heads + m) * HW + pix] : 0.f;
      } else {   // the dO row also sums D = dO . O, channel by channel as it is staged
        const size_t off = ((size_t)(b * L + tl) * inner + m * DH) * HW + pix;
        float* __restrict__ dst = sG + row * LD;
        float dsum = 0.f;
#pragma unroll
        for (int c0 = 0; c0 < DH; c0 += CH) {
          float v[CH], o[CH];
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            v[c] = live ? a.dout[off + (size_t)(c0 + c) * HW] : 0.f;
            o[c] = live ? a.out[off + (size_t)(c0 + c) * HW] : 0.f;
          }
#pragma unroll
          for (int c = 0; c < CH; ++c) {
            dst[c0 + c] = v[c];
            dsum = fmaf(v[c], o[c], dsum);
          }
        }
        sDd[row] = dsum;
      }
    }
    __syncthreads();
    if (!wave_work) continue;
    const int nqb = (min(QT, T - q0) + 31) >> 5;
#pragma unroll 1
    for (int qb = 0; qb < nqb; ++qb) {
      // S[query][key] and dP: a lane owns one key column
      const f32x16x2 sd = mfma_scores2<DH>(sQ + (32 * qb + qi) * LD + h, kv, sG + (32 * qb + qi) * LD + h, vv);
      f32x16 sc = sd.a, dp = sd.b;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rowl = mfma_row(r, h, 32 * qb), tok = q0 + rowl;
        const bool ok = kvalid && tok < T;
        const float p = ok ? expf(sc[r] + sP[ok ? g.rel_off(tok) + pk : 0] - sL[rowl]) : 0.f;
        sc[r] = p;
        dp[r] = p * (dp[r] - sDd[rowl]);
      }
      mfma_apply2<DV / 32, LD>(sG + qi, sQ + qi, 32 * qb, h, sc, dp, dv, dk);
    }
  }
  if (!kok) return;   // no barrier follows
  float* __restrict__ dkp = a.dqkv + (size_t)(b * L + kl) * g.agent + (size_t)(inner + m * DH) * HW + kpix;
  auto keep = [&](float x) { return kvalid ? x : 0.f; };   // exact zeros for the keys of masked agents
  mfma_store_t<DH>(dkp, HW, h, dk, keep);
  mfma_store_t<DH>(dkp + (size_t)inner * HW, HW, h, dv, keep);
}

template <int DH, int WS>
inline int swap_attn_bwd_launch(SwapBwdArgs a, int B, hipStream_t st) {
  constexpr int DV = DH < 32 ? 32 : DH, PW = 2 * WS - 1;
  int nchunk;
  swap_split(a.L, WS, a.nblk, a.wpc, nchunk);
  const size_t np = (size_t)(2 * a.L - 1) * PW * PW;
  const size_t shm_q = ((size_t)2 * 64 * (DV + 1) + 2 * np) * sizeof(float);
  const size_t shm_k = ((size_t)2 * 64 * (DV + 1) + 2 * 64 + np) * sizeof(float);
  if (shm_q > 48 * 1024)
    GC_HIP(hipFuncSetAttribute((const void*)swap_attn_bwd_q_kernel<DH, WS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm_q));
  if (shm_k > 48 * 1024)
    GC_HIP(hipFuncSetAttribute((const void*)swap_attn_bwd_k_kernel<DH, WS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm_k));
  const long long groups = (long long)(a.H / WS) * (a.W / WS) * nchunk;
  GC_CHECK_ARG(groups < (1LL << 31), "swap attention backward: too many groups for one launch");
  const dim3 grid((unsigned)groups, a.heads, B);
  // Consecutive workgroup ids are dealt round-robin to the 8 XCDs, each with an L2 of its own, while the groups that share cache lines are
  // neighbours (8 windows, or all Y grid cells of a row, per 128-byte line): hand XCD k the k-th eighth of the groups instead. It pays
  // wherever a group's tokens are short runs (ws 4: both partitions; ws 8: the window partition); the 8 x 8 grid partition gains nothing.
  a.xcd = groups % 8 == 0 && (WS == 4 || !a.grid_mode);
  swap_attn_klog(DH, WS, "swap_attn_bwd_q_kernel");
  swap_attn_bwd_q_kernel<DH, WS><<<grid, 64 * a.wpc, shm_q, st>>>(a);
  GC_HIP(hipGetLastError());
  swap_attn_klog(DH, WS, "swap_attn_bwd_k_kernel");
  swap_attn_bwd_k_kernel<DH, WS><<<grid, 64 * a.wpc, shm_k, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

#pragma clang fp contract(fast)

}  // namespace gc
