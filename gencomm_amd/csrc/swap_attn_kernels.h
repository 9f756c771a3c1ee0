// CoBEVT fusion (reference: opencood/models/fuse_modules/fusion_in_one.py:409-464 + fuse_modules/swap_fusion_modules.py) -- the
// attention core of SwapFusionBlockMask's `Attention` (swap_fusion_modules.py:87-128).  Everything around it runs on kernels the
// library already has (warp_affine_kernel, the LayerNorm and the 1x1 implicit-GEMM convolution for every Linear).
//   swap_attn_kernel   per scene, head and GROUP (one ws x ws window or one grid cell of the map): attention over the group's
//                      L * ws * ws tokens (agent l, w1, w2) JOINTLY, softmax(q k^T dim_head^-0.5 + bias[rel(i, j)], keys of agents
//                      l >= N_b masked) v, with the 3-D relative position bias
//                        rel = (li - lj + L - 1)(2 ws - 1)^2 + (hi - hj + ws - 1)(2 ws - 1) + (wi - wj + ws - 1)
//                      (= the module's relative_position_index buffer, :63-85) computed in the kernel.
//   agent_mean_kernel  the head's mean over the L agent rows of a scene (mlp_head's Reduce, :275).
// Partitions are index arithmetic on the NCHW maps, nothing is rearranged in memory (X = H / ws, Y = W / ws):
//   window  token (l, w1, w2) of group (x, y) = pixel (x ws + w1, y ws + w2) of agent l       '(x w1) (y w2)', :173-176
//   grid    token (l, w1, w2) of group (x, y) = pixel (w1 X + x, w2 Y + y) of agent l         '(w1 x) (w2 y)', :184-187
// QUERIES of padded agents (l >= N_b) are computed like any other: their rows are zero only before the first residual and enter the
// final mean over all L agents; only their KEYS are masked.  The ego (agent 0) is always valid, so no row is fully masked.
//
// fp32 in, out and accumulation on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, an fmaf chain), in the
// tile of attn_mfma.h: a wave owns one block of 32 queries and walks the keys in blocks of 32, S^T[key][query] = K Q^T, O^T += V^T P.
// 320 tokens (L 5, ws 8) x dim_head 64 of K and V are 166 KB: the keys are staged in tiles of 64 ([key][DH + 1] rows: odd stride,
// conflict-free fills and operand reads) with a running softmax.  64 keys are four agents of a 4 x 4 group or one agent of an 8 x 8
// group, so the key loop ends at the last VALID agent: masked agents cost nothing at ws 8 and at most part of one tile at ws 4.
// A workgroup = up to 8 query blocks of one (group, head, scene); a group of more than 256 tokens is split evenly over several
// workgroups, each staging the group's keys for itself.
// swap_attn_kernel<DH, WS, true> (gencomm_swap_attn_train_fwd) is the same body with one more store per query, lse = running max +
// log(running denominator), which swap_attn_bwd_kernels.h turns back into the probabilities; `out` is computed by the same instructions.
#pragma once
#include "attn_mfma.h"

namespace gc {

// Contraction is off for everything in this header and in swap_attn_bwd_kernels.h: a product and the sum it feeds are rounded one after
// the other, wherever the header is included.
#pragma clang fp contract(off)

constexpr int kSwapMaxAgents = 8;  // MAX_AGENTS_PER_SCENE of the Python package

struct SwapArgs {
  const float* qkv;     // [B * L][3 * inner][H][W] (q | k | v blocks of inner = heads * DH channels, head-major)
  const float* table;   // relative_position_bias_table [(2 L - 1)(2 WS - 1)^2][heads]
  const int* nvalid;    // [B] agents present in each scene (clamped to 1 .. L here: the host never reads it)
  float* out;           // [B * L][inner][H][W]
  int L, heads, H, W, grid_mode;
  int nqb, wpc;         // query blocks of 32 per group; query blocks (= waves) per workgroup
  float scale;
  float* lse;           // [B * L][heads][H][W], written by the TRAIN instantiation only: running max + log(running denominator)
};

// The (group, head, scene) of a workgroup and where its tokens live, for the forward and both backward kernels (Args = SwapArgs or
// SwapBwdArgs).  bx = blockIdx.x, or the backward's remap of it (swap_bwd_bx); nblk = blocks of 32 tokens per group.
template <int DH, int WS>
struct SwapGroup {
  static constexpr int T1 = WS * WS, PW = 2 * WS - 1, PW2 = PW * PW;
  int chunk, m, b, L, T, TV, inner, HW, W, X, Y, gx, gy, grid_mode;
  size_t agent;                     // floats of one agent's q | k | v
  const float* __restrict__ base;   // the scene's qkv
  template <class Args>
  __device__ __forceinline__ SwapGroup(const Args& a, int nblk, int bx) {
    const int nchunk = (nblk + a.wpc - 1) / a.wpc, grp = bx / nchunk;
    chunk = bx - grp * nchunk;
    m = blockIdx.y, b = blockIdx.z, L = a.L, W = a.W, grid_mode = a.grid_mode;
    X = a.H / WS, Y = a.W / WS;
    gx = grp / Y, gy = grp - gx * Y;
    T = L * T1;                                       // tokens = queries of the group
    TV = min(max(a.nvalid[b], 1), L) * T1;            // its valid keys: the agents present come first
    inner = a.heads * DH, HW = a.H * a.W;
    agent = (size_t)3 * inner * HW;
    base = a.qkv + (size_t)b * L * agent;
  }
  // pixel of the token's (w1, w2) inside this group
  __device__ __forceinline__ int pixel(int w1, int w2) const {
    return grid_mode ? (w1 * X + gx) * W + w2 * Y + gy : (gx * WS + w1) * W + gy * WS + w2;
  }
  // offset of token (l, w1, w2) in the relative position table: rel(query, key) = off(query) - off(key) + the centre
  // (L - 1) PW2 + (WS - 1) PW + WS - 1
  static __device__ __forceinline__ int rel_off(int tok) { return (tok / T1) * PW2 + ((tok % T1) / WS) * PW + tok % WS; }
};

// One row of a staged tile: DH channels through registers, up to 32 loads in flight before the first LDS store; a dead row becomes zeros.
template <int DH, class Load>
__device__ __forceinline__ void swap_fill_row(float* dst, bool live, Load load) {
  constexpr int CH = DH < 32 ? DH : 32;   // channels a fill thread has in flight
#pragma unroll
  for (int c0 = 0; c0 < DH; c0 += CH) {
    float v[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] = live ? load(c0 + c) : 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c) dst[c0 + c] = v[c];
  }
}

// The K | V tile of keys k0 .. k0 + 63 of head g.m: one (key, K or V) row per thread and pass; keys beyond the valid ones become zero rows.
template <int DH, int WS, int LDK, int LDV>
__device__ __forceinline__ void swap_fill_kv(const SwapGroup<DH, WS>& g, int k0, float* sK, float* sV) {
  constexpr int KT = 64, T1 = WS * WS;
  for (int e = threadIdx.x; e < 2 * KT; e += blockDim.x) {
    const int row = e & (KT - 1), isv = e / KT, key = k0 + row;
    const bool live = key < g.TV;
    const int kt = live ? key : 0;
    const float* __restrict__ src = g.base + (kt / T1) * g.agent + (size_t)((1 + isv) * g.inner + g.m * DH) * g.HW + g.pixel((kt % T1) / WS, kt % WS);
    swap_fill_row<DH>(isv ? sV + row * LDV : sK + row * LDK, live, [&](int c) { return src[(size_t)c * g.HW]; });
  }
}

template <int DH, int WS, bool TRAIN = false>
__global__ __launch_bounds__(512) void swap_attn_kernel(const SwapArgs a) {
  constexpr int T1 = WS * WS, KT = 64, LDK = DH + 1, DV = DH < 32 ? 32 : DH, LDV = DV + 1, PW = 2 * WS - 1, PW2 = PW * PW;
  static_assert(KT % T1 == 0 && DH % 16 == 0 && DH <= 64, "4 x 4 or 8 x 8 groups, head width 16, 32 or 64");
  extern __shared__ float sw_smem[];  // K [KT][LDK], V [KT][LDV] (columns DH .. 31 zero when DH < 32), bias of this head [(2 L - 1) PW2]
  float* sK = sw_smem;
  float* sV = sK + KT * LDK;
  float* sP = sV + KT * LDV;
  const int tid = threadIdx.x, nthr = blockDim.x;
  const SwapGroup<DH, WS> g(a, a.nqb, blockIdx.x);
  const int m = g.m, b = g.b, L = g.L, T = g.T, TV = g.TV, inner = g.inner, HW = g.HW;

  for (int i = tid; i < (2 * L - 1) * PW2; i += nthr) sP[i] = a.table[(size_t)i * a.heads + m];
  if (DV != DH)
    for (int i = tid; i < KT * LDV; i += nthr) sV[i] = 0.f;   // the columns beyond DH are never written again

  // wave = one block of 32 queries (lanes l and l + 32 share a query)
  const int wave = tid >> 6, lane = tid & 63, qi = lane & 31, h = lane >> 5;
  const int qb = g.chunk * a.wpc + wave;
  const bool wave_live = wave < a.wpc && qb < a.nqb;      // wave-uniform; a wave without queries still fills and meets the barriers
  const int qtok = qb * 32 + qi;
  const bool qok = wave_live && qtok < T;
  const int qt = qok ? qtok : 0;
  const int ql = qt / T1, qh = (qt % T1) / WS, qw = qt % WS;
  const int qpix = g.pixel(qh, qw);
  float qv[DH / 2];
#pragma unroll
  for (int s = 0; s < DH / 2; ++s) qv[s] = qok ? g.base[ql * g.agent + (size_t)(m * DH + 2 * s + h) * HW + qpix] * a.scale : 0.f;
  f32x16 o[DV / 32];
#pragma unroll
  for (int db = 0; db < DV / 32; ++db) o[db] = mfma_zero();
  float mrun = -INFINITY, den = 0.f;
  const int pbase = (ql + L - 1) * PW2 + (qh + WS - 1) * PW + (qw + WS - 1);

  for (int k0 = 0; k0 < TV; k0 += KT) {
    __syncthreads();   // the previous tile is no longer read (first pass: the bias and the zero fill are complete after the next one)
    swap_fill_kv<DH, WS, LDK, LDV>(g, k0, sK, sV);
    __syncthreads();
    if (!wave_live) continue;
    const int nkb = (min(KT, TV - k0) + 31) >> 5;   // every walked block of 32 begins with a valid key
#pragma unroll 1
    for (int kb = 0; kb < nkb; ++kb) {
      f32x16 sc = mfma_scores<DH>(sK + (32 * kb + qi) * LDK + h, qv);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = mfma_row(r, h, k0 + 32 * kb);
        const bool kok = key < TV;
        const float bias = sP[kok ? pbase - g.rel_off(key) : 0];   // rel(query, key) = pbase - off(key)
        sc[r] = kok ? sc[r] + bias : -INFINITY;
      }
      mfma_softmax_step<false>(sc, mrun, den, o);   // finite: the block's first key is valid
      mfma_apply<DV / 32, LDV>(sV + qi, 32 * kb, h, sc, o);
    }
  }
  if (!qok) return;   // no barrier follows
  den += __shfl_xor(den, 32, 64);   // the partner lane holds the same query: it is live too
  const float rden = 1.0f / den;
  mfma_store_t<DH>(a.out + ((size_t)(b * L + ql) * inner + m * DH) * HW + qpix, HW, h, o, [&](float x) { return x * rden; });
  if (TRAIN && h == 0) a.lse[((size_t)(b * L + ql) * a.heads + m) * HW + qpix] = mrun + logf(den);
}

// The split of a group's blocks of 32 tokens over workgroups: at most 8 blocks (= waves) each, evenly.
inline void swap_split(int L, int ws, int& nblk, int& wpc, int& nchunk) {
  nblk = (L * ws * ws + 31) / 32;
  const int split = (nblk + 7) / 8;
  wpc = (nblk + split - 1) / split;
  nchunk = (nblk + wpc - 1) / wpc;
}

inline void swap_attn_klog(int dh, int ws, const char* kernel = "swap_attn_kernel", const char* tail = "") {
  if (!klog_armed()) return;
  char name[64];
  snprintf(name, sizeof name, "%s<%d,%d%s>", kernel, dh, ws, tail);
  klog_note(name);
}

template <int DH, int WS, bool TRAIN = false>
inline int swap_attn_launch(SwapArgs a, int B, hipStream_t st) {
  constexpr int DV = DH < 32 ? 32 : DH, PW = 2 * WS - 1;
  int nchunk;
  swap_split(a.L, WS, a.nqb, a.wpc, nchunk);
  const size_t shm = ((size_t)64 * (DH + 1) + 64 * (DV + 1) + (2 * a.L - 1) * PW * PW) * sizeof(float);
  if (shm > 48 * 1024)
    GC_HIP(hipFuncSetAttribute((const void*)swap_attn_kernel<DH, WS, TRAIN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));
  const long long groups = (long long)(a.H / WS) * (a.W / WS) * nchunk;
  GC_CHECK_ARG(groups < (1LL << 31), "swap attention: too many groups for one launch");
  swap_attn_klog(DH, WS, "swap_attn_kernel", TRAIN ? ",train" : "");
  swap_attn_kernel<DH, WS, TRAIN><<<dim3((unsigned)groups, a.heads, B), 64 * a.wpc, shm, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

template <bool TRAIN>
inline int swap_attn_dispatch(const SwapArgs& a, int B, int dim_head, int window, hipStream_t st) {
  if (window == 4 && dim_head == 16) return swap_attn_launch<16, 4, TRAIN>(a, B, st);
  if (window == 4 && dim_head == 32) return swap_attn_launch<32, 4, TRAIN>(a, B, st);
  if (window == 4 && dim_head == 64) return swap_attn_launch<64, 4, TRAIN>(a, B, st);
  if (window == 8 && dim_head == 16) return swap_attn_launch<16, 8, TRAIN>(a, B, st);
  if (window == 8 && dim_head == 32) return swap_attn_launch<32, 8, TRAIN>(a, B, st);
  return swap_attn_launch<64, 8, TRAIN>(a, B, st);
}

// out [B][count] = mean over the L rows of x [B][L][count], summed in agent order (count = C * H * W)
__global__ __launch_bounds__(256) void agent_mean_kernel(const float* __restrict__ x, float* __restrict__ out, int L, long long count) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const float* __restrict__ p = x + (size_t)blockIdx.y * L * count + i;
  float s = 0.f;
  for (int l = 0; l < L; ++l) s += p[(size_t)l * count];
  out[(size_t)blockIdx.y * count + i] = s / (float)L;
}

#pragma clang fp contract(fast)

}  // namespace gc
