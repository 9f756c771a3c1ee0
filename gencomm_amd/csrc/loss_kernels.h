// Detection-head part of the GenComm training criterion in ONE launch: classification (sigmoid focal), regression (smooth-L1 on the
// sin-difference encoding) and direction (softmax cross entropy over the heading bins) of PointPillarLoss
// (opencood/loss/point_pillar_loss.py:36-126, helpers :129-170, :216-245), forward AND the gradients of the three weighted sums with
// respect to the head maps.  The reference writes the criterion as ~70 framework elementwise operators on kilobyte-sized maps and
// autograd adds ~90 more in the backward: ~150 launches of a 1 150-launch training step for microseconds of arithmetic.
//
// Layouts as the heads and the collate produce them: cls [B][A][H][W], reg [B][7A][H][W], dir [B][A*A][H][W] (the reference's
// `view(-1, anchor_num)` groups the direction channels by anchor: logits of anchor a = channels a*A .. a*A+A-1);
// pos / neg [B][H][W][A], targets [B][H][W][7A].  Anchor k of a sample = (pixel hw, anchor a), k = hw * A + a.
// One thread per (sample, anchor a, pixel): consecutive threads walk the pixels of one channel (coalesced in the NCHW maps).
#pragma once
#include "common.h"

namespace gc {

// Contraction is off in this header for a historical reason, not a numerical one: since it was written it has been compiled behind
// iou3d_kernels.h, which used to leave `off` in force for every later include of its translation unit.  Its float64 comparisons and
// golden fixtures were taken on these bits, so the mode is pinned here rather than inherited; nothing in the arithmetic below is
// known to need it.
#pragma clang fp contract(off)

constexpr int kLossMaxAnchors = 8;

struct HeadLossArgs {
  const float *cls, *reg, *dir;
  const float *pos, *neg, *tgt;
  float *gcls, *greg, *gdir;   // d (cls_loss + reg_loss + dir_loss) / d map, same layouts as cls / reg / dir
  double* sums;                // [4] += cls_loss, reg_loss, dir_loss (weighted, / batch size), their sum; the caller zeroes it
  int B, A, HW;
  int has_dir, num_bins;
  float pos_cls_weight, gamma, alpha, cls_weight, sigma, reg_weight, dir_weight, inv_bs;
  double dir_offset;
  double anchor_yaw[kLossMaxAnchors];   // radians, float64 like the reference's numpy table
};

__global__ __launch_bounds__(256) void head_loss_kernel(const HeadLossArgs a) {
  __shared__ float s_red[4][4];
  const int b = blockIdx.y, tid = threadIdx.x, A = a.A, HW = a.HW, NA = HW * A;
  // number of positive anchors of the sample (point_pillar_loss.py:72-74: clamp(min = 1)): every workgroup of the sample counts them
  // itself -- NA values, cache hits after the first workgroup -- instead of a launch of its own
  float cnt = 0.f;
  for (int k = tid; k < NA; k += 256) cnt += a.pos[(size_t)b * NA + k] > 0.f ? 1.f : 0.f;
  cnt = wave_sum(cnt);
  if ((tid & 63) == 0) s_red[tid >> 6][3] = cnt;
  __syncthreads();
  const float pos_norm = fmaxf(s_red[0][3] + s_red[1][3] + s_red[2][3] + s_red[3][3], 1.0f);

  float l_cls = 0.f, l_reg = 0.f, l_dir = 0.f;
  const int i = blockIdx.x * 256 + tid;   // (anchor a, pixel hw) of sample b
  if (i < NA) {
    const int an = i / HW, hw = i - an * HW, k = hw * A + an;
    const float t = a.pos[(size_t)b * NA + k];
    const bool positive = t > 0.f, negative = a.neg[(size_t)b * NA + k] > 0.f;
    // ---- classification: sigmoid focal loss (point_pillar_loss.py:230-245)
    {
      const size_t e = ((size_t)b * A + an) * HW + hw;
      const float x = a.cls[e];
      const float w = ((positive ? a.pos_cls_weight : 0.f) + (negative ? 1.f : 0.f)) / pos_norm;
      const float ex = expf(-fabsf(x));
      const float ce = fmaxf(x, 0.f) - x * t + log1pf(ex);
      const float p = 1.0f / (1.0f + expf(-x));
      const float pt = t * p + (1.f - t) * (1.f - p), q = 1.f - pt;
      const float mod = a.gamma == 2.0f ? q * q : powf(q, a.gamma);
      const float dmod = a.gamma == 2.0f ? 2.0f * q : (q > 0.f ? a.gamma * powf(q, a.gamma - 1.0f) : 0.f);   // d mod / d q
      const float aw = t * a.alpha + (1.f - t) * (1.f - a.alpha);
      l_cls = mod * aw * ce * w;
      const float dce = (x >= 0.f ? 1.f : 0.f) - t - (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)) * ex / (1.f + ex);   // clamp(min = 0) passes the gradient at 0, |x| does not
      const float dq = -(2.f * t - 1.f) * p * (1.f - p);   // d q / d x
      a.gcls[e] = (dmod * dq * ce + mod * dce) * aw * w * a.cls_weight * a.inv_bs;
    }
    // ---- regression: smooth-L1 on (x, y, z, h, w, l, sin-difference of the yaw), positives only (:129-140, :216-226)
    const float rw = (positive ? 1.f : 0.f) / pos_norm;
    const float s2 = a.sigma * a.sigma, thr = 1.0f / s2;
    float t6 = 0.f;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      const size_t e = ((size_t)b * 7 * A + an * 7 + j) * HW + hw;
      const float pv = a.reg[e], tv = a.tgt[((size_t)b * NA + k) * 7 + j];
      float d, dd = 1.0f;   // d = encoded prediction - encoded target, dd = d d / d prediction
      if (j == 6) {
        float sp, cp, st, ct;
        sincosf(pv, &sp, &cp);
        sincosf(tv, &st, &ct);
        d = sp * ct - cp * st;
        dd = cp * ct + sp * st;
        t6 = tv;
      } else {
        d = pv - tv;
      }
      const float ad = fabsf(d);
      const bool lt = ad <= thr;
      const float as = ad * a.sigma;
      l_reg += (lt ? 0.5f * as * as : ad - 0.5f / s2) * rw;
      const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
      a.greg[e] = (lt ? s2 * ad : 1.0f) * sgn * dd * rw * a.reg_weight * a.inv_bs;
    }
    // ---- direction: bin of the ground-truth heading (:142-170, float64 like the reference), softmax cross entropy, positives only
    if (a.has_dir) {
      const double two_pi = 6.283185307179586476925286766559;
      const double v = ((double)t6 + a.anchor_yaw[an]) - a.dir_offset;
      const double off = v - floor(v / two_pi) * two_pi;
      long long bin = (long long)floor(off / (two_pi / a.num_bins));
      bin = bin < 0 ? 0 : (bin > a.num_bins - 1 ? a.num_bins - 1 : bin);
      float lg[kLossMaxAnchors], mx = -INFINITY;
      for (int c = 0; c < A; ++c) {
        lg[c] = a.dir[((size_t)b * A * A + an * A + c) * HW + hw];
        mx = fmaxf(mx, lg[c]);
      }
      float se = 0.f, lt = 0.f;   // lt: the target bin's logit (selected in the loop: no dynamically indexed register array)
      for (int c = 0; c < A; ++c) {
        se += expf(lg[c] - mx);
        lt = c == (int)bin ? lg[c] : lt;
      }
      const float lse = mx + logf(se);
      l_dir = (lse - lt) * rw;
      for (int c = 0; c < A; ++c)
        a.gdir[((size_t)b * A * A + an * A + c) * HW + hw] = (expf(lg[c] - lse) - (c == (int)bin ? 1.f : 0.f)) * rw * a.dir_weight * a.inv_bs;
    }
  }
  l_cls = wave_sum(l_cls);
  l_reg = wave_sum(l_reg);
  l_dir = wave_sum(l_dir);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = l_cls; s_red[tid >> 6][1] = l_reg; s_red[tid >> 6][2] = l_dir; }
  __syncthreads();
  if (tid < 3 && (tid < 2 || a.has_dir)) {
    const float wsel = tid == 0 ? a.cls_weight : (tid == 1 ? a.reg_weight : a.dir_weight);
    const double v = ((double)s_red[0][tid] + (double)s_red[1][tid] + (double)s_red[2][tid] + (double)s_red[3][tid]) * (double)wsel * (double)a.inv_bs;
    atomicAdd(&a.sums[tid], v);
    atomicAdd(&a.sums[3], v);   // their sum: the differentiable output of the host-side Function
  }
}

inline int head_loss_enqueue(const HeadLossArgs& a, hipStream_t st) {
  const int NA = a.HW * a.A;
  head_loss_kernel<<<dim3((NA + 255) / 256, a.B), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}


// -------------------------------------------------------------------------------------------------------------------------------------
// Multi-class detection-head terms of the V2X-Real criteria (opencood/loss/point_pillar_v2xreal_loss.py and its GenComm twin
// point_pillar_v2xreal_gencomm_loss.py: forward :88-160, WeightedSmoothL1Loss :12-70, cls_loss_func :168-199, add_sin_difference
// :221-233), forward values AND the gradients of conf_loss + reg_loss with respect to the head maps, in two launches: a per-sample count
// of the positive slots, then the loss.
//
// Layouts: cls [B][S*K][H][W], reg [B][7S][H][W], labels [B][H][W][S], targets [B][H][W][S][7]; S = slots per location (rotations x
// class blocks), K = classes. The logits of slot j are channels j*K .. j*K+K-1, its regression channels 7j .. 7j+6.
// Per sample b: P_b = #{label > 0}; cls weight [label == 0 or label > 0] / max(P_b, 1), reg weight [label > 0] / max(P_b, 1) (float32,
// :104-114). The one-hot target over the K logits comes from the label VALUE l (class l - 1; l = -1 is multiplied by `cared` first and is
// background, :116-125). Focal loss with alpha 0.25 and gamma 2 (:78-79) in float32. Regression: smooth-L1 with beta = 1/9 and a strict
// `<`, NaN targets replaced by the prediction (difference 0, gradient 0), in the targets' dtype T as the reference's type promotion
// does (sin / cos of the float32 prediction rounded to float32, then promoted). Both sums are divided by B (psm.shape[0]).
// One thread per (sample, slot j, pixel): consecutive threads walk the pixels of one channel (coalesced in the NCHW maps).
// -------------------------------------------------------------------------------------------------------------------------------------
constexpr int kLossMcMaxClasses = 8;

template <typename T>
__device__ __forceinline__ T wave_sum_t(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T>
struct HeadLossMcArgs {
  const float *cls, *reg;
  const T *lab, *tgt;
  const unsigned* count;   // [B] positive slots per sample (head_loss_mc_count_kernel)
  float *gcls, *greg;      // d (conf_loss + reg_loss) / d map, same layouts as cls / reg
  double* sums;            // [3] += conf_loss, reg_loss, their sum; the caller zeroes it
  int B, S, K, HW;
  double cls_weight, reg_weight;
};

// count[b] += #{labels[b][..] > 0}: one vector atomic per workgroup into the caller-zeroed counter
template <typename T>
__global__ __launch_bounds__(256) void head_loss_mc_count_kernel(const T* __restrict__ lab, unsigned* __restrict__ count, int n) {
  __shared__ unsigned s_cnt[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  unsigned c = 0;
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) c += lab[(size_t)b * n + i] > T(0) ? 1u : 0u;
  c = wave_sum_t(c);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    const unsigned tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (tot) atomicAdd(&count[b], tot);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void head_loss_mc_kernel(const HeadLossMcArgs<T> a) {
  __shared__ float s_cls[4];
  __shared__ T s_reg[4];
  const int b = blockIdx.y, tid = threadIdx.x, S = a.S, K = a.K, HW = a.HW;
  const float inv_bs = 1.0f / (float)a.B;
  float l_cls = 0.f;
  T l_reg = T(0);
  const int i = blockIdx.x * 256 + tid;   // (slot j, pixel hw) of sample b
  if (i < S * HW) {
    const int j = i / HW, hw = i - j * HW;
    const size_t slot = ((size_t)b * HW + hw) * S + j;   // index of the slot in labels / targets
    const T l = a.lab[slot];
    const bool positive = l > T(0), negative = l == T(0);
    const float pos_norm = fmaxf((float)a.count[b], 1.0f);
    const float w = ((negative ? 1.0f : 0.f) + (positive ? 1.0f : 0.f)) / pos_norm;
    // ---- classification: sigmoid focal loss over the K logits of the slot (:168-199), one-hot of the label value
    const int cls_idx = l >= T(0) && l <= T(K) ? (int)l - 1 : -1;   // -1: background (an ignored slot's weight is 0)
    const float cw = (float)a.cls_weight * inv_bs;
    for (int k = 0; k < K; ++k) {
      const size_t e = ((size_t)b * S * K + (size_t)j * K + k) * HW + hw;
      const float x = a.cls[e];
      const float t = k == cls_idx ? 1.f : 0.f;
      const float p = 1.0f / (1.0f + expf(-x));
      const float aw = t * 0.25f + (1.f - t) * 0.75f;
      const float pt = t * (1.f - p) + (1.f - t) * p;
      const float ex = expf(-fabsf(x));
      const float bce = fmaxf(x, 0.f) - x * t + log1pf(ex);
      l_cls += aw * (pt * pt) * bce * w;
      // clamp(min = 0) passes the gradient at 0, |x| does not
      const float dbce = (x >= 0.f ? 1.f : 0.f) - t - (x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f)) * ex / (1.f + ex);
      const float dpt = (1.f - 2.f * t) * p * (1.f - p);
      a.gcls[e] = aw * (2.f * pt * dpt * bce + pt * pt * dbce) * w * cw;
    }
    // ---- regression: smooth-L1 (beta 1/9, strict <) on (x, y, z, h, w, l, sin-difference of the yaw), positives only
    const T beta = T(1.0 / 9.0), half_beta = T(0.5 * (1.0 / 9.0));
    const T rw = (T)((positive ? 1.0f : 0.f) / pos_norm);
    const T gw = (T)a.reg_weight / (T)a.B * rw;   // d reg_loss / d (weighted smooth-L1 term), autograd's order
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const size_t e = ((size_t)b * 7 * S + (size_t)j * 7 + c) * HW + hw;
      const float pv = a.reg[e];
      const T tv = a.tgt[slot * 7 + c];
      float sp = 0.f, cp = 0.f;
      T st = T(0), ct = T(0), d;   // d = encoded prediction - encoded target (NaN target: the prediction)
      bool nan;
      if (c == 6) {
        // correctly rounded float32 sin / cos of the prediction (and T ones of the target): the reference's CPU float32 trig is
        // within 1 ulp of these, no closer form is available to a GPU
        double sd, cd;
        sincos((double)pv, &sd, &cd);
        sp = (float)sd;
        cp = (float)cd;
        sincos((double)tv, &sd, &cd);
        st = (T)sd;
        ct = (T)cd;
        const T pe = (T)sp * ct, te = (T)cp * st;
        nan = te != te;
        d = pe - (nan ? pe : te);
      } else {
        nan = tv != tv;
        d = (T)pv - (nan ? (T)pv : tv);
      }
      const T n = d < T(0) ? -d : d;
      const bool lt = n < beta;
      l_reg += (lt ? T(0.5) * (n * n) / beta : n - half_beta) * rw;
      const T sgn = d > T(0) ? T(1) : (d < T(0) ? T(-1) : T(0));
      const T gd = (lt ? gw / beta * T(0.5) * (T(2) * n) : gw) * sgn;   // d reg_loss / d d
      float g;
      if (nan) {
        g = 0.f;   // where(isnan(target), input, target): the two paths cancel exactly
      } else if (c == 6) {
        // the reference's two float32 paths into the prediction, rounded as autograd rounds them (the sum cancels near |d| = 1)
        g = __fadd_rn(__fmul_rn((float)(gd * ct), cp), __fmul_rn((float)(-gd * st), -sp));   // no contraction into an FMA
      } else {
        g = (float)gd;
      }
      a.greg[e] = g;
    }
  }
  l_cls = wave_sum(l_cls);
  l_reg = wave_sum_t(l_reg);
  if ((tid & 63) == 0) { s_cls[tid >> 6] = l_cls; s_reg[tid >> 6] = l_reg; }
  __syncthreads();
  if (tid == 0) {
    const double c = ((double)s_cls[0] + (double)s_cls[1] + (double)s_cls[2] + (double)s_cls[3]) * a.cls_weight / a.B;
    const double r = ((double)s_reg[0] + (double)s_reg[1] + (double)s_reg[2] + (double)s_reg[3]) * a.reg_weight / a.B;
    atomicAdd(&a.sums[0], c);
    atomicAdd(&a.sums[1], r);
    atomicAdd(&a.sums[2], c + r);   // their sum: the differentiable output of the host-side Function
  }
}

template <typename T>
inline int head_loss_mc_enqueue(const HeadLossMcArgs<T>& a, unsigned* count, hipStream_t st) {
  const int n = a.HW * a.S;
  const int cnt_blocks = (n + 255) / 256 < 64 ? (n + 255) / 256 : 64;   // grid-stride beyond 16 K slots per sample
  head_loss_mc_count_kernel<T><<<dim3(cnt_blocks, a.B), 256, 0, st>>>(a.lab, count, n);
  GC_HIP(hipGetLastError());
  head_loss_mc_kernel<T><<<dim3((n + 255) / 256, a.B), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}


// -------------------------------------------------------------------------------------------------------------------------------------
// Depth term of the camera criteria (opencood/loss/point_pillar_depth_loss.py:40-54 with FocalLoss :105-185, reduction "none", no
// smoothing, no foreground mask): per pixel -alpha (1 - p_t)^gamma log p_t at the target bin t of softmax(logit) over the D bins,
// `.mean() * weight`, and its gradient with respect to the logits, in one launch.  logit / grad [BN][D][HW], target int64 [BN][HW].
// One thread per pixel (coalesced along hw).  1 - p_t is formed as sum_{d != t} e_d / sum_d e_d (no cancellation near p_t = 1);
// d loss / d z_d = -alpha ([d == t] - p_d) ((1 - p_t)^gamma - gamma (1 - p_t)^(gamma - 1) p_t log p_t).  The value is accumulated in
// float64 (sum += scale * block sum; the caller zeroes it), scale = weight / (BN HW).  A target outside [0, D) poisons the value and
// its pixel's gradients with NaN (the reference's one_hot raises).
// -------------------------------------------------------------------------------------------------------------------------------------
struct DepthFocalArgs {
  const float* logit;
  const long long* target;
  float* grad;
  double* sum;
  int D, HW;
  long long total;
  float alpha, gamma, scale;
};

__global__ __launch_bounds__(256) void depth_focal_loss_kernel(const DepthFocalArgs a) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const long long i = (long long)blockIdx.x * 256 + tid;
  double loss = 0.0;
  if (i < a.total) {
    const int D = a.D, HW = a.HW;
    const long long bn = i / HW;
    const int hw = (int)(i - bn * HW);
    const float* __restrict__ lg = a.logit + (size_t)bn * D * HW + hw;
    float* __restrict__ gr = a.grad + (size_t)bn * D * HW + hw;
    const long long t = a.target[i];
    const bool ok = t >= 0 && t < D;
    float m = -INFINITY;
    for (int d = 0; d < D; ++d) m = fmaxf(m, lg[(size_t)d * HW]);
    float s = 0.f, rest = 0.f, et = 0.f, zt = 0.f;
    for (int d = 0; d < D; ++d) {
      const float z = lg[(size_t)d * HW], e = expf(z - m);
      s += e;
      if (d == t) { et = e; zt = z; } else rest += e;
    }
    const float rs = 1.0f / s;
    const float logp = (zt - m) - logf(s), pt = et * rs, q = rest * rs;
    const float mod = a.gamma == 2.0f ? q * q : powf(q, a.gamma);
    const float dmod = a.gamma == 2.0f ? 2.0f * q : (q > 0.f ? a.gamma * powf(q, a.gamma - 1.0f) : 0.f);
    const float k = ok ? -a.alpha * (mod - dmod * pt * logp) * a.scale : NAN;
    loss = ok ? (double)(-a.alpha * mod * logp) : (double)NAN;
    for (int d = 0; d < D; ++d) gr[(size_t)d * HW] = k * (d == t ? q : -expf(lg[(size_t)d * HW] - m) * rs);
  }
  loss = wave_sum_t<double>(loss);
  if ((tid & 63) == 0) s_red[tid >> 6] = loss;
  __syncthreads();
  if (tid == 0) atomicAdd(a.sum, (s_red[0] + s_red[1] + s_red[2] + s_red[3]) * (double)a.scale);
}

#pragma clang fp contract(fast)

}  // namespace gc
