// The terms that the HEAL and MPDA training criteria add to the detection-head loss (loss_kernels.h), each with its gradient:
//
//   * the multi-level occupancy focal loss of PointPillarPyramidLoss (opencood/loss/point_pillar_pyramid_loss.py:69-103, calc_occ_loss),
//     every pyramid level in two launches;
//   * the domain BCE of PointPillarMPDALoss (opencood/loss/point_pillar_mpda_loss.py:124-150), two launches.
//
// The reference writes the occupancy term as two max_pool2d, four permutes, a normaliser and a focal loss PER LEVEL, on maps of a few
// thousand cells, and autograd doubles that: dozens of launches for microseconds of arithmetic.  Here the level labels are formed from
// pos_equal_one / neg_equal_one inside the kernels and never stored.
//
// No atomics anywhere in this header: every value is a sum over a fixed index order (per thread a strided walk, per wave a butterfly,
// per workgroup the waves in order, across workgroups a second launch that walks the partial sums in order), so two runs give the same
// bits, and nothing has to be zeroed by the caller.
#pragma once
#include "common.h"

namespace gc {

// Contraction is off in this header so that focal_term below rounds exactly as the classification block of head_loss_kernel
// (loss_kernels.h, compiled with contraction off) does: the occupancy heads and the detection heads see one focal loss.
#pragma clang fp contract(off)

constexpr int kOccMaxLevels = 4;
constexpr int kOccValueThreads = 1024;
constexpr int kBceMaxAgents = 1024;        // bits of the source mask
constexpr int kBceBlocksPerAgent = 32;     // workgroup partial sums per agent map

// Sigmoid focal loss of one logit x against the target t in {0, 1} (point_pillar_loss.py:230-245), without the anchor weight:
// val = (1 - p_t)^gamma * alpha_t * ce, dval = d val / d x.  The operator sequence of head_loss_kernel's classification block.
__device__ __forceinline__ void focal_term(float x, float t, float gamma, float alpha, float& val, float& dval) {
  const float ex = expf(-fabsf(x));
  const float ce = fmaxf(x, 0.f) - x * t + log1pf(ex);
  const float p = 1.0f / (1.0f + expf(-x));
  const float pt = t * p + (1.f - t) * (1.f - p), q = 1.f - pt;
  const float mod = gamma == 2.0f ? q * q : powf(q, gamma);
  const float dmod = gamma == 2.0f ? 2.0f * q : (q > 0.f ? gamma * powf(q, gamma - 1.0f) : 0.f);   // d mod / d q
  const float aw = t * alpha + (1.f - t) * (1.f - alpha);
  const float dce = (x >= 0.f ? 1.f : 0.f) - t - (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)) * ex / (1.f + ex);   // clamp(min = 0) passes the gradient at 0, |x| does not
  const float dq = -(2.f * t - 1.f) * p * (1.f - p);   // d q / d x
  val = mod * aw * ce;
  dval = (dmod * dq * ce + mod * dce) * aw;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// Sum of one double per thread over a workgroup of NW waves, waves added in order; valid in thread 0.  `s` holds NW doubles.
template <int NW>
__device__ __forceinline__ double block_sum_f64(double v, double* s) {
  v = wave_sum_f64(v);
  __syncthreads();   // a previous use of `s` has been read
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  double tot = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < NW; ++w) tot += s[w];
  return tot;
}

// -------------------------------------------------------------------------------------------------------------------------------------
// Occupancy term.  pos / neg [B][H][W][A] (anchors 0 and 1 are read, as in the reference), level i: logits occ_i [B][1][H_i][W_i] with
// H_i = H / k_i, W_i = W / k_i (max_pool2d floors: the remainder rows and columns belong to no window).  Per level cell
//   pos_l = any cell of its k x k window has pos[..,0] != 0 or pos[..,1] != 0
//   neg_l = every cell of its window has neg[..,0] != 0 and neg[..,1] != 0          (1 - maxpool(1 - occ_neg))
// and per (sample, level) norm = max(sum pos_l, 1), cell weight w = (pos_l * pos_cls_weight + neg_l) / norm, focal loss with target
// pos_l; the level's loss is the sum over samples and cells / B * weight_i.
//
// Launch 1, occ_value_kernel, one workgroup per (level, sample): counts the positives and sums the unnormalised focal terms in float64
// (norm is one number per workgroup, so it leaves the sum), writes norm and sum / norm to `part`.  Launch 2, occ_grad_kernel, one thread per
// level cell of all levels (the levels of a sample laid end to end, so a workgroup may span two): the gradient, written once; its first
// workgroup also adds the (sample, level) values in order into the per-level losses and the total.
// -------------------------------------------------------------------------------------------------------------------------------------
struct OccLossArgs {
  const float *pos, *neg;
  const float* occ[kOccMaxLevels];
  float* grad[kOccMaxLevels];          // d total / d occ_i, the layout of occ_i
  double* sums;                        // [5] total, level 0..3 (0 for a level that does not exist); then `part`
  double* part;                        // [B][4][2]: norm, value of (sample, level) -- sums + 5
  int B, H, W, A, levels;
  int k[kOccMaxLevels], Hl[kOccMaxLevels], Wl[kOccMaxLevels];
  int cell_start[kOccMaxLevels + 1];   // first cell of level i in a sample's end-to-end order; [levels] = cells per sample
  float weight[kOccMaxLevels];
  float pos_cls_weight, alpha, gamma, inv_bs;
};

// the labels of level cell (y, x) of sample b at window size k: every read is inside [0, H) x [0, W) because y < H / k and x < W / k
__device__ __forceinline__ void occ_labels(const OccLossArgs& a, int b, int k, int y, int x, bool& pos_l, bool& neg_l) {
  pos_l = false;
  neg_l = true;
  for (int r = y * k; r < y * k + k; ++r) {
    const size_t row = ((size_t)b * a.H + r) * a.W;
    for (int c = x * k; c < x * k + k; ++c) {
      const size_t e = (row + c) * a.A;
      pos_l = pos_l || a.pos[e] != 0.f || a.pos[e + 1] != 0.f;
      neg_l = neg_l && a.neg[e] != 0.f && a.neg[e + 1] != 0.f;
    }
  }
}

__global__ __launch_bounds__(kOccValueThreads) void occ_value_kernel(const OccLossArgs a) {
  __shared__ double s_red[kOccValueThreads / 64];
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;   // l is uniform: the table reads below are scalar loads
  const int k = a.k[l], Wl = a.Wl[l], n = a.Hl[l] * Wl;
  const float* __restrict__ occ = a.occ[l] + (size_t)b * n;
  double cnt = 0.0, sum = 0.0;
  for (int j = tid; j < n; j += kOccValueThreads) {
    const int y = j / Wl, x = j - y * Wl;
    bool pos_l, neg_l;
    occ_labels(a, b, k, y, x, pos_l, neg_l);
    float val, dval;
    focal_term(occ[j], pos_l ? 1.f : 0.f, a.gamma, a.alpha, val, dval);
    cnt += pos_l ? 1.0 : 0.0;
    sum += (double)(val * ((pos_l ? a.pos_cls_weight : 0.f) + (neg_l ? 1.f : 0.f)));
  }
  cnt = block_sum_f64<kOccValueThreads / 64>(cnt, s_red);
  sum = block_sum_f64<kOccValueThreads / 64>(sum, s_red);
  if (tid == 0) {
    const double norm = cnt > 1.0 ? cnt : 1.0;   // clamp(min = 1)
    double* p = a.part + ((size_t)b * kOccMaxLevels + l) * 2;
    p[0] = norm;
    p[1] = sum / norm;
  }
}

__global__ __launch_bounds__(256) void occ_grad_kernel(const OccLossArgs a) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;   // cell of sample b, levels end to end
  if (i < a.cell_start[a.levels]) {
    // the level of the cell and its table row, selected without a dynamically indexed copy of the tables
    int l = 0, k = a.k[0], Hl = a.Hl[0], Wl = a.Wl[0], start = 0;
    float wl = a.weight[0];
    const float* occ = a.occ[0];
    float* grad = a.grad[0];
#pragma unroll
    for (int q = 1; q < kOccMaxLevels; ++q)
      if (q < a.levels && i >= a.cell_start[q]) {
        l = q; k = a.k[q]; Hl = a.Hl[q]; Wl = a.Wl[q]; start = a.cell_start[q]; wl = a.weight[q]; occ = a.occ[q]; grad = a.grad[q];
      }
    const int j = i - start, y = j / Wl, x = j - y * Wl;
    const size_t e = (size_t)b * Hl * Wl + j;
    bool pos_l, neg_l;
    occ_labels(a, b, k, y, x, pos_l, neg_l);
    const float norm = (float)a.part[((size_t)b * kOccMaxLevels + l) * 2];   // a count: exact in float32 below 2^24 cells
    const float w = ((pos_l ? a.pos_cls_weight : 0.f) + (neg_l ? 1.f : 0.f)) / norm;
    float val, dval;
    focal_term(occ[e], pos_l ? 1.f : 0.f, a.gamma, a.alpha, val, dval);
    grad[e] = dval * w * wl * a.inv_bs;
  }
  if (blockIdx.x == 0 && b == 0 && tid == 0) {   // the values of launch 1, samples in order, then levels in order
    double total = 0.0;
    for (int l = 0; l < kOccMaxLevels; ++l) {
      double s = 0.0;
      if (l < a.levels) {
        for (int bb = 0; bb < a.B; ++bb) s += a.part[((size_t)bb * kOccMaxLevels + l) * 2 + 1];
        s = s * (double)a.inv_bs * (double)a.weight[l];
      }
      a.sums[1 + l] = s;
      total += s;
    }
    a.sums[0] = total;
  }
}

inline int occ_loss_enqueue(const OccLossArgs& a, hipStream_t st) {
  occ_value_kernel<<<dim3(a.levels, a.B), kOccValueThreads, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  occ_grad_kernel<<<dim3((a.cell_start[a.levels] + 255) / 256, a.B), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}


// -------------------------------------------------------------------------------------------------------------------------------------
// Domain term.  x [N][C][H][W] logits of the domain classifier, target 1 on every element of a source agent (the first agent of a
// scene: bit n of `source`) and 0 elsewhere; value = mean over all N C H W elements of max(x, 0) - x t + log1p(exp(-|x|)), gradient
// (sigmoid(x) - t) / numel.  Launch 1: gradient (written once) and one float64 partial sum per workgroup (kBceBlocksPerAgent strided
// workgroups per agent, so a workgroup's target is one number); launch 2: the partial sums in order, / numel.
// -------------------------------------------------------------------------------------------------------------------------------------
struct DomainBceArgs {
  const float* x;
  float* grad;
  double* sums;   // [0] the mean; [1 + n * kBceBlocksPerAgent + block] partial sums
  int N, CHW, blocks;
  float inv_numel;
  unsigned long long source[kBceMaxAgents / 64];
};

__global__ __launch_bounds__(256) void domain_bce_kernel(const DomainBceArgs a) {
  __shared__ double s_red[4];
  const int n = blockIdx.y, tid = threadIdx.x;
  const float t = (a.source[n >> 6] >> (n & 63)) & 1ull ? 1.f : 0.f;
  const float* __restrict__ x = a.x + (size_t)n * a.CHW;
  float* __restrict__ g = a.grad + (size_t)n * a.CHW;
  double sum = 0.0;
  for (int i = blockIdx.x * 256 + tid; i < a.CHW; i += a.blocks * 256) {
    const float v = x[i];
    sum += (double)(fmaxf(v, 0.f) - v * t + log1pf(expf(-fabsf(v))));
    g[i] = (1.0f / (1.0f + expf(-v)) - t) * a.inv_numel;
  }
  sum = block_sum_f64<4>(sum, s_red);
  if (tid == 0) a.sums[1 + n * kBceBlocksPerAgent + blockIdx.x] = sum;
}

__global__ __launch_bounds__(256) void domain_bce_reduce_kernel(const DomainBceArgs a) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x, total = a.N * a.blocks;
  double sum = 0.0;
  for (int i = tid; i < total; i += 256) sum += a.sums[1 + (i / a.blocks) * kBceBlocksPerAgent + i % a.blocks];
  sum = block_sum_f64<4>(sum, s_red);
  if (tid == 0) a.sums[0] = sum / ((double)a.N * (double)a.CHW);
}

inline int domain_bce_enqueue(const DomainBceArgs& a, hipStream_t st) {
  domain_bce_kernel<<<dim3(a.blocks, a.N), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  domain_bce_reduce_kernel<<<1, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

#pragma clang fp contract(fast)

}  // namespace gc
