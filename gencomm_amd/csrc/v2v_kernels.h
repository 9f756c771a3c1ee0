// V2VNet message passing (gfx950, wave64, fp32; grid maths in fp64).
//
// Reference: V2VNetFusion.forward (opencood/models/fuse_modules/fusion_in_one.py:238-353) with ConvGRU
// (opencood/models/sub_modules/convgru.py).  Per iteration, node i of a scene with N agents receives from every agent j
//   message_ij = msg_cnn(cat[warp_ij(h_j), h_i]) * warp_ij(ones)
// which is averaged or maxed over j and fed, next to h_i, to a ConvGRU that starts from a zero hidden state.  The convolutions run on
// the library's implicit-GEMM kernel (msg_cnn split into its source half and its node half, gencomm_amd/v2vnet.py); the three kernels
// here are what is left around them:
//   v2v_warp_pairs_kernel   out[p] = warp_affine_simple(x[src_row[p]], theta[p]) for P (target, source) pairs: the source map is read
//                           in place for each of its targets.  Cell and taps are fuse_cell / fuse_sample (fuse_cell.h), the workgroup is
//                           fuse_body's: 64 pixels x 4 channel quarters.  A pair whose theta is exactly the identity (i == j) is a copy.
//   v2v_aggregate_kernel    m_p = (y[p] + e[k]) * mask_p over the pairs p of node k, mean (divisor N_k) or max over p, written as
//                           [h_k | agg] (the ConvGRU's input) or h_k + agg.  mask_p = warp of a map of ones = the sum of the in-range tap
//                           weights, in fuse_sample's fma order; it is computed here, once per (pixel, pair) of a workgroup, shared
//                           through LDS, and never stored.  Streaming: 128-bit accesses when H W is a multiple of 4.
//   gru_gate_kernel         h = sigmoid(beta) * tanh(candidate): what ConvGRUCell.forward leaves of a cell whose h_cur is zero.
// No atomics, every output element has one writer: two runs are bit-identical.
//
// Training (gencomm_amd/v2vnet.py, trainable=True) adds their adjoints:
//   v2v_aggregate_kernel<V, true>   the same body, which for max also writes the index (within the node's pair list) of the winning message:
//                           torch.max's rule -- a strictly greater value replaces the current one, so the lowest index wins among equal
//                           maxima, and a NaN replaces anything but an earlier NaN.  `out` is computed by the same instructions as before.
//   v2v_aggregate_bwd_kernel  d m_p = d agg / N_k (mean) or d agg [winner == p] (max); d y[p] = d m_p mask_p, d e[k] = sum_p d m_p mask_p,
//                           the masks recomputed as in the forward (once per (pixel, pair) of a workgroup, through LDS).
//   gru_gate_bwd_kernel     d beta = d h tanh(c) s (1 - s), d candidate = d h s (1 - tanh(c)^2), s and tanh recomputed from g.
//   v2v_warp_bwd_*          d x[r] (+)= sum over the pairs p that read row r of warp^T(d warped[p]; theta[p]).  v2v_warp_bwd_plan_kernel
//                           sorts the pairs on the device: 2 = exactly the identity (the forward copied: the adjoint adds), 1 = tame
//                           (fuse_bwd_plan_kernel's test: gathered per SOURCE pixel with fuse_for_each_match), 0 = anything else
//                           (scattered with float atomics by v2v_warp_bwd_scatter_kernel, after the gather).  The gather's workgroup is
//                           64 source pixels x 4 channel quarters: per batch of four pairs, wave j builds the match lists of pair j in
//                           LDS, then all four quarters consume them over their channels; more channel slices sit in blockIdx.z.  With
//                           identity and tame pairs only, every element of d x has one writer and sums in a fixed order.
#pragma once
#include "common.h"
#include "fuse_cell.h"

namespace gc {

constexpr int kV2vMaxPairs = 8;   // pairs per node = agents per scene

struct V2vWarpArgs {
  const float* x;        // [rows][C][H][W]
  const double* theta;   // [P][2][3]
  const int* src_row;    // [P]
  float* out;            // [P][C][H][W]
  int C, H, W;
};

__global__ __launch_bounds__(256) void v2v_warp_pairs_kernel(const V2vWarpArgs a) {
  const int H = a.H, W = a.W, HW = H * W;
  const int p = blockIdx.y;
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int pix_raw = blockIdx.x * 64 + pl;
  const bool live = pix_raw < HW;
  const int pix = live ? pix_raw : HW - 1;   // dead pixels are clamped, not retired: their loads stay in the map
  const double* __restrict__ th = a.theta + (size_t)p * 6;
  const float* __restrict__ xs = a.x + (size_t)a.src_row[p] * a.C * HW;
  float* __restrict__ op = a.out + (size_t)p * a.C * HW + pix;
  if (th[0] == 1.0 && th[1] == 0.0 && th[2] == 0.0 && th[3] == 0.0 && th[4] == 1.0 && th[5] == 0.0) {   // block-uniform: i == j
    for (int c = cq; c < a.C; c += 4) {
      const float v = xs[(size_t)c * HW + pix];
      if (live) op[(size_t)c * HW] = v;
    }
    return;
  }
  const int h = pix / W, w = pix - h * W;
  const double xb = fuse_base(w, W), yb = fuse_base(h, H);
  int idx[4];
  unsigned ok;
  float wt[4];
  fuse_cell(th, xb, yb, H, W, idx, ok, wt);
  for (int c = cq; c < a.C; c += 4) {
    const float v = fuse_sample(xs + (size_t)c * HW, idx, ok, wt);
    if (live) op[(size_t)c * HW] = v;
  }
}

struct V2vAggArgs {
  const float* y;         // [P][C][H][W]      conv(warp_ij(h_j); W[:, :C])
  const float* e;         // [n_nodes][C][H][W] conv(h_i; W[:, C:]) + bias
  const float* h;         // [rows][C][H][W]   node states; node k reads row node_row[k]
  const double* theta;    // [P][2][3]
  const int* node_row;    // [n_nodes]
  const int* pair_off;    // [n_nodes + 1]
  float* out;             // out_mode 0: [n_nodes][2C][H][W] = [h | agg];  1: [n_nodes][C][H][W] = h + agg
  int C, H, W;
  int op;                 // 0 mean, 1 max
  int out_mode;
  int c_per_block;        // channels per blockIdx.z slice, a multiple of 4
  unsigned char* winner;  // training entry, op 1: [n_nodes][C][H][W] index of the winning message within the node's pairs; else null
};

// The warp of a map of ones: fuse_sample on a plane whose every tap is 1 (same fma order, so the same bits as warping such a plane).
__device__ __forceinline__ float v2v_mask(unsigned ok, const float (&wt)[4]) {
  float v = 0.f;
#pragma unroll
  for (int k = 0; k < 4; ++k) v = fmaf((ok >> k) & 1u ? 1.f : 0.f, wt[k], v);
  return v;
}

template <int V> struct V2vVec;
template <> struct V2vVec<1> {
  float v[1];
  __device__ __forceinline__ void load(const float* p) { v[0] = p[0]; }
  __device__ __forceinline__ void store(float* p) const { p[0] = v[0]; }
};
template <> struct V2vVec<4> {
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
  __device__ __forceinline__ void store(float* p) const { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};

// Workgroup = 64 pixel groups of V pixels x 4 channel quarters, one node (blockIdx.y), one channel slice (blockIdx.z).  Quarter cq
// computes the masks of pairs cq and cq + 4 for its V pixels; the four quarters meet in LDS, so a workgroup evaluates fuse_cell once per
// (pixel, pair).  V = 4 needs H W % 4 == 0 (every plane then starts 16-byte aligned relative to the base pointers).
// TRAIN (launched for the max only): the winner map is written next to `out`.  With the mean the message's product and the running sum
// contract into one fma where the product has no other use, so an instantiation that also compares the message would round differently:
// the training entry launches the TRAIN = false instantiation for the mean.
template <int V, bool TRAIN>
__global__ __launch_bounds__(256) void v2v_aggregate_kernel(const V2vAggArgs a) {
  __shared__ __attribute__((aligned(16))) float s_mask[kV2vMaxPairs][64 * V];
  const int H = a.H, W = a.W, HW = H * W, C = a.C;
  const int k = blockIdx.y;
  const int p0 = a.pair_off[k], N = a.pair_off[k + 1] - p0;   // block-uniform
  if (N < 1 || N > kV2vMaxPairs) return;                      // the caller checks the scene sizes; such a node is left untouched
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int g_raw = blockIdx.x * 64 + pl;                      // pixel group
  const int ngroups = HW / V;                                  // V == 4: exact
  const bool live = g_raw < ngroups;
  const int pix0 = (live ? g_raw : ngroups - 1) * V;
  for (int j = cq; j < N; j += 4) {
    const double* __restrict__ th = a.theta + (size_t)(p0 + j) * 6;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int pix = pix0 + i;
      const int hh = pix / W, ww = pix - hh * W;
      const double xb = fuse_base(ww, W), yb = fuse_base(hh, H);
      int idx[4];
      unsigned ok;
      float wt[4];
      fuse_cell(th, xb, yb, H, W, idx, ok, wt);
      s_mask[j][pl * V + i] = v2v_mask(ok, wt);
    }
  }
  __syncthreads();   // every thread of the workgroup gets here: dead pixel groups were clamped, not retired
  const float* __restrict__ hs = a.h + (size_t)a.node_row[k] * C * HW + pix0;
  const float* __restrict__ es = a.e + (size_t)k * C * HW + pix0;
  const float* __restrict__ ys = a.y + (size_t)p0 * C * HW + pix0;
  float* __restrict__ os = a.out + (size_t)k * (a.out_mode == 0 ? 2 * C : C) * HW + pix0;
  const float fn = (float)N;            // torch.mean's divisor: agents whose mask is zero count
  const int c_end = min(C, (int)(blockIdx.z + 1) * a.c_per_block);
  for (int c = blockIdx.z * a.c_per_block + cq; c < c_end; c += 4) {
    V2vVec<V> ev, hv, agg;
    ev.load(es + (size_t)c * HW);
    hv.load(hs + (size_t)c * HW);
    float best[V];             // TRAIN: torch.max's running maximum and its index
    unsigned char win[V];
    for (int j = 0; j < N; ++j) {
      V2vVec<V> yv, mk;
      yv.load(ys + ((size_t)j * C + c) * HW);
      mk.load(&s_mask[j][pl * V]);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float m = (yv.v[i] + ev.v[i]) * mk.v[i];
        agg.v[i] = j == 0 ? m : (a.op == 0 ? agg.v[i] + m : fmaxf(agg.v[i], m));
        if (TRAIN) {
          if (j == 0 || m > best[i] || (m != m && best[i] == best[i])) { best[i] = m; win[i] = (unsigned char)j; }
        }
      }
    }
    if (a.op == 0) {
#pragma unroll
      for (int i = 0; i < V; ++i) agg.v[i] = agg.v[i] / fn;
    }
    if (!live) continue;
    if (TRAIN && a.op == 1) {
      unsigned char* __restrict__ wp = a.winner + ((size_t)k * C + c) * HW + pix0;
      if constexpr (V == 4) *reinterpret_cast<uchar4*>(wp) = make_uchar4(win[0], win[1], win[2], win[3]);
      else wp[0] = win[0];
    }
    if (a.out_mode == 0) {
      hv.store(os + (size_t)c * HW);
      agg.store(os + (size_t)(C + c) * HW);
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) agg.v[i] = hv.v[i] + agg.v[i];
      agg.store(os + (size_t)c * HW);
    }
  }
}

// h[n][i] = sigmoid(g[n][i]) * tanh(g[n][C HW + i]) for i < C HW = `count`; blockIdx.y = n.  expf / tanhf are the accurate library forms.
template <int V>
__global__ __launch_bounds__(256) void gru_gate_kernel(const float* __restrict__ g, float* __restrict__ h, long long count) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (i >= count) return;
  const float* __restrict__ gb = g + (size_t)blockIdx.y * 2 * count + i;
  V2vVec<V> beta, cand, o;
  beta.load(gb);
  cand.load(gb + count);
#pragma unroll
  for (int k = 0; k < V; ++k) o.v[k] = (1.0f / (1.0f + expf(-beta.v[k]))) * tanhf(cand.v[k]);
  o.store(h + (size_t)blockIdx.y * count + i);
}


// ---- training: the adjoints ------------------------------------------------------------------------------------------------------
struct V2vAggBwdArgs {
  const float* dagg;            // d agg of node k at dagg + k * node_stride: the second channel half of d [h | agg], or d (h + agg) itself
  size_t node_stride;
  const double* theta;          // [P][2][3]
  const int* pair_off;          // [n_nodes + 1]
  const unsigned char* winner;  // [n_nodes][C][H][W] (op 1)
  float* dy;                    // [P][C][H][W]
  float* de;                    // [n_nodes][C][H][W]
  int C, H, W;
  int op;
  int c_per_block;
};

// The forward's workgroup: 64 pixel groups of V pixels x 4 channel quarters, one node, one channel slice; the masks as there.
template <int V>
__global__ __launch_bounds__(256) void v2v_aggregate_bwd_kernel(const V2vAggBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float s_mask[kV2vMaxPairs][64 * V];
  const int H = a.H, W = a.W, HW = H * W, C = a.C;
  const int k = blockIdx.y;
  const int p0 = a.pair_off[k], N = a.pair_off[k + 1] - p0;   // block-uniform
  if (N < 1 || N > kV2vMaxPairs) return;                      // as in the forward: such a node is left untouched
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int g_raw = blockIdx.x * 64 + pl;
  const int ngroups = HW / V;
  const bool live = g_raw < ngroups;
  const int pix0 = (live ? g_raw : ngroups - 1) * V;
  for (int j = cq; j < N; j += 4) {
    const double* __restrict__ th = a.theta + (size_t)(p0 + j) * 6;
#pragma unroll
    for (int i = 0; i < V; ++i) {
      const int pix = pix0 + i;
      const int hh = pix / W, ww = pix - hh * W;
      const double xb = fuse_base(ww, W), yb = fuse_base(hh, H);
      int idx[4];
      unsigned ok;
      float wt[4];
      fuse_cell(th, xb, yb, H, W, idx, ok, wt);
      s_mask[j][pl * V + i] = v2v_mask(ok, wt);
    }
  }
  __syncthreads();   // every thread gets here: dead pixel groups were clamped, not retired
  const float* __restrict__ ds = a.dagg + (size_t)k * a.node_stride + pix0;
  const unsigned char* __restrict__ ws = a.op == 1 ? a.winner + (size_t)k * C * HW + pix0 : nullptr;
  float* __restrict__ dys = a.dy + (size_t)p0 * C * HW + pix0;
  float* __restrict__ des = a.de + (size_t)k * C * HW + pix0;
  const float fn = (float)N;
  const int c_end = min(C, (int)(blockIdx.z + 1) * a.c_per_block);
  for (int c = blockIdx.z * a.c_per_block + cq; c < c_end; c += 4) {
    V2vVec<V> dg, dev;
    dg.load(ds + (size_t)c * HW);
    int win[V];
#pragma unroll
    for (int i = 0; i < V; ++i) win[i] = -1;
    if (a.op == 1) {
      if constexpr (V == 4) {
        const uchar4 t = *reinterpret_cast<const uchar4*>(ws + (size_t)c * HW);
        win[0] = t.x; win[1] = t.y; win[2] = t.z; win[3] = t.w;
      } else {
        win[0] = ws[(size_t)c * HW];
      }
    } else {
#pragma unroll
      for (int i = 0; i < V; ++i) dg.v[i] = dg.v[i] / fn;   // torch.mean's backward: the gradient divided by the number of pairs
    }
#pragma unroll
    for (int i = 0; i < V; ++i) dev.v[i] = 0.f;
    for (int j = 0; j < N; ++j) {
      V2vVec<V> mk, o;
      mk.load(&s_mask[j][pl * V]);
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float dm = (a.op == 0 || win[i] == j) ? dg.v[i] : 0.f;
        o.v[i] = dm * mk.v[i];
        dev.v[i] += o.v[i];
      }
      if (live) o.store(dys + ((size_t)j * C + c) * HW);
    }
    if (live) dev.store(des + (size_t)c * HW);
  }
}

// dg[n][i] = dh s(1 - s) tanh(c), dg[n][count + i] = dh s (1 - tanh(c)^2) with s = sigmoid(g[n][i]), c = g[n][count + i]; blockIdx.y = n.
template <int V>
__global__ __launch_bounds__(256) void gru_gate_bwd_kernel(const float* __restrict__ g, const float* __restrict__ dh, float* __restrict__ dg,
                                                           long long count) {
  const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
  if (i >= count) return;
  const float* __restrict__ gb = g + (size_t)blockIdx.y * 2 * count + i;
  float* __restrict__ ob = dg + (size_t)blockIdx.y * 2 * count + i;
  V2vVec<V> beta, cand, d, ob_, oc_;
  beta.load(gb);
  cand.load(gb + count);
  d.load(dh + (size_t)blockIdx.y * count + i);
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float s = 1.0f / (1.0f + expf(-beta.v[k])), t = tanhf(cand.v[k]);
    ob_.v[k] = d.v[k] * t * (s * (1.0f - s));
    oc_.v[k] = d.v[k] * s * (1.0f - t * t);
  }
  ob_.store(ob);
  oc_.store(ob + count);
}

struct V2vWarpBwdArgs {
  const float* dwarped;      // [P][C][H][W]
  const double* theta;       // [P][2][3]
  const int* src_row;        // [P]
  const int* row_pair_off;   // [rows + 1]: the pairs that read row r are row_pairs[row_pair_off[r] .. row_pair_off[r + 1])
  const int* row_pairs;      // [P]
  float* dx;                 // [rows][C][H][W]
  int* plan;                 // [P]: 2 identity, 1 tame (gathered), 0 scattered
  int P, C, H, W;
  int accumulate;
  int c_per_block;           // channels per blockIdx.z slice, a multiple of 4
};

__global__ __launch_bounds__(64) void v2v_warp_bwd_plan_kernel(const V2vWarpBwdArgs a) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= a.P) return;
  const double* th = a.theta + (size_t)p * 6;
  int kind = 0;
  if (th[0] == 1.0 && th[1] == 0.0 && th[2] == 0.0 && th[3] == 0.0 && th[4] == 1.0 && th[5] == 0.0) {
    kind = 2;
  } else {
    // fuse_bwd_plan_kernel's test: in pixel units every row of the inverse map's matrix has an L1 norm <= 1.5 and |det| > 0.6
    const double m00 = th[0], m01 = th[1] * a.W / a.H, m10 = th[3] * a.H / a.W, m11 = th[4];
    const double det = m00 * m11 - m01 * m10;
    if (fabs(det) > 0.25) {
      const double r0 = (fabs(m11) + fabs(m01)) / fabs(det), r1 = (fabs(m10) + fabs(m00)) / fabs(det);
      kind = (r0 <= 1.5 && r1 <= 1.5 && fabs(det) > 0.6) ? 1 : 0;
    }
  }
  a.plan[p] = kind;
}

constexpr int kV2vBwdBatch = 4;   // pairs whose match lists are in LDS at a time: one per wave

// Workgroup = 64 source pixels x 4 channel quarters, one source row (blockIdx.y), one channel slice (blockIdx.z).
__global__ __launch_bounds__(256) void v2v_warp_bwd_gather_kernel(const V2vWarpBwdArgs a) {
  __shared__ int s_p[kV2vBwdBatch][FUSE_KM][64];
  __shared__ float s_w[kV2vBwdBatch][FUSE_KM][64];
  __shared__ int s_cnt[kV2vBwdBatch][64];
  const int H = a.H, W = a.W, HW = H * W, C = a.C;
  const int r = blockIdx.y;
  const int o0 = a.row_pair_off[r], npairs = a.row_pair_off[r + 1] - o0;   // block-uniform
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int q_raw = blockIdx.x * 64 + pl;
  const bool live = q_raw < HW;
  const int q = live ? q_raw : HW - 1;       // dead pixels are clamped, not retired: every thread meets every barrier
  const int qy = q / W, qx = q - qy * W;
  float* __restrict__ dxp = a.dx + (size_t)r * C * HW + q;
  const int c_begin = blockIdx.z * a.c_per_block + cq, c_end = min(C, (int)(blockIdx.z + 1) * a.c_per_block);
  int b0 = 0;
  do {                                       // at least once: a row that no pair reads is still written (zeros, or left as it is)
    const int nb = min(max(npairs - b0, 0), kV2vBwdBatch);
    if (cq < nb) {                           // wave cq builds the list of pair b0 + cq
      const int p = a.row_pairs[o0 + b0 + cq];
      int cnt = 0;
      if (a.plan[p] == 1) {
        fuse_for_each_match(a.theta + (size_t)p * 6, qx, qy, H, W, [&](int pp, float wgt) {
          if (cnt < FUSE_KM) { s_p[cq][cnt][pl] = pp; s_w[cq][cnt][pl] = wgt; }
          ++cnt;
        });
      }
      s_cnt[cq][pl] = cnt;
    }
    __syncthreads();
    const bool init = a.accumulate != 0 || b0 > 0;
    for (int c = c_begin; c < c_end; c += 4) {
      float acc = init ? dxp[(size_t)c * HW] : 0.f;
      for (int j = 0; j < nb; ++j) {
        const int p = a.row_pairs[o0 + b0 + j];
        const int kind = a.plan[p];
        const float* __restrict__ gp = a.dwarped + ((size_t)p * C + c) * HW;
        if (kind == 2) {
          acc += gp[q];
        } else if (kind == 1) {
          const int cnt = s_cnt[j][pl], kept = min(cnt, FUSE_KM);
          for (int m = 0; m < kept; ++m) acc = fmaf(s_w[j][m][pl], gp[s_p[j][m][pl]], acc);
          if (cnt > FUSE_KM) {               // as in fuse_bwd_gather_kernel: the rest is found again per channel, never dropped
            int m = 0;
            fuse_for_each_match(a.theta + (size_t)p * 6, qx, qy, H, W, [&](int pp, float wgt) {
              if (m++ >= FUSE_KM) acc = fmaf(wgt, gp[pp], acc);
            });
          }
        }
      }
      if (live) dxp[(size_t)c * HW] = acc;
    }
    __syncthreads();                         // the lists are rebuilt by the next batch
    b0 += kV2vBwdBatch;
  } while (b0 < npairs);
}

// The pairs the plan left over (plan 0): thread = one OUTPUT pixel of the pair, its four taps added with float atomics.
__global__ __launch_bounds__(256) void v2v_warp_bwd_scatter_kernel(const V2vWarpBwdArgs a) {
  const int p = blockIdx.y;
  if (a.plan[p] != 0) return;                // block-uniform
  const int H = a.H, W = a.W, HW = H * W;
  const int pl = threadIdx.x & 63, cq = threadIdx.x >> 6;
  const int pix = blockIdx.x * 64 + pl;
  if (pix >= HW) return;
  const int h = pix / W, w = pix - h * W;
  const double xb = fuse_base(w, W), yb = fuse_base(h, H);
  int idx[4];
  unsigned ok;
  float wt[4];
  fuse_cell(a.theta + (size_t)p * 6, xb, yb, H, W, idx, ok, wt);
  const float* __restrict__ gp = a.dwarped + (size_t)p * a.C * HW + pix;
  float* __restrict__ dxr = a.dx + (size_t)a.src_row[p] * a.C * HW;
  for (int c = cq; c < a.C; c += 4) {
    const float g = gp[(size_t)c * HW];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (((ok >> k) & 1u) && wt[k] != 0.f) atomicAdd(dxr + (size_t)c * HW + idx[k], wt[k] * g);
  }
}

}  // namespace gc
