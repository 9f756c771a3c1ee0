// Detection tail on the device (gfx950, wave64): anchor decoding + score filter + ordered compaction,
// rotated NMS (score sort, pairwise convex-quad IoU in fp64, greedy scan, range mask) and the axis-aligned
// overlap matrix of target assignment.  SURVEY.md 8f rank 3.
//
// Reference (all CPU/torch/numpy/shapely there):
//   VoxelPostprocessor.post_process     opencood/data_utils/post_processor/voxel_postprocessor.py:1084-1244
//   delta_to_boxes3d                    .../voxel_postprocessor.py:1351-1396
//   limit_period, rotate_points_along_z opencood/utils/common_utils.py:104-113, :139-161
//   boxes_to_corners_3d, project_box3d  opencood/utils/box_utils.py:152-204, :278-316
//   remove_large_pred_bbx, remove_bbx_abnormal_z, mask_boxes_outside_range_numpy   box_utils.py:1062-1112, :384-421
//   nms_rotated (+ shapely IoU)         box_utils.py:915-960, common_utils.py:230-270
//   bbox_overlaps                       opencood/utils/box_overlaps.pyx:17-57
//
// Arithmetic mirrors the reference op by op (fp32 for the boxes, fp64 for polygon areas) with fused
// multiply-add contraction switched off, so that the same candidates cross the same thresholds.
#pragma once
#include "common.h"
#include "box_overlap.h"

namespace gc {

#pragma clang fp contract(off)

struct DetArgs {
  const float* cls;      // [A][H][W]      (batch 1)
  const float* reg;      // [7A][H][W]
  const float* dir;      // [A*nb][H][W] or null
  const float* anchors;  // [H][W][A][7]
  const float* T;        // [4][4] row-major, agent -> ego
  float* score_tmp;      // [H*W*A] scratch: sigmoid score or -1
  int* block_count;      // [nblocks] scratch
  int* block_off;        // [nblocks] scratch
  float* corners;        // [cap][8][3] (appended at *count)
  float* scores;         // [cap]
  int* anchor_idx;       // [cap]
  int* count;            // device counter: candidates so far (in/out)
  int H, W, A, nb, cap, hwl;
  float thr, dir_offset;
};

__device__ __forceinline__ float limit_period_f(float val, float offset, float period) {
  return val - floorf(val / period + offset) * period;
}

// delta_to_boxes3d of anchor `an` at pixel `pix` (regression channel 7 an + d); ab = that anchor's 7 values
__device__ __forceinline__ void det_box7(const float* __restrict__ reg, const float* __restrict__ ab, int an, int pix, int HW,
                                         float (&b)[7]) {
  float d[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) d[k] = reg[(size_t)(an * 7 + k) * HW + pix];
  const float diag = sqrtf(ab[4] * ab[4] + ab[5] * ab[5]);
  b[0] = d[0] * diag + ab[0];
  b[1] = d[1] * diag + ab[1];
  b[2] = d[2] * ab[3] + ab[2];
  b[3] = expf(d[3]) * ab[3];
  b[4] = expf(d[4]) * ab[4];
  b[5] = expf(d[5]) * ab[5];
  b[6] = d[6] + ab[6];
}

// finite: no projected corner is NaN or infinite (fminf / fmaxf skip a NaN, so the extents alone would let such a box pass, while the
// reference's torch max / min propagate it and its comparisons then reject the box)
struct BoxExtent { float xmin, xmax, ymin, ymax, zmin, zmax; bool finite; };

// boxes_to_corners_3d (-> u, unprojected) + project_box3d (-> c); returns the extents of c
__device__ __forceinline__ BoxExtent det_corners(const float (&b)[7], int hwl, const float* __restrict__ T, float (&u)[8][3],
                                                 float (&c)[8][3]) {
  // boxes_to_corners_3d: (l, w, h) extents; 'hwl' stores them as [h, w, l]
  const float ex = hwl ? b[5] : b[3], ey = b[4], ez = hwl ? b[3] : b[5];
  const float cosa = cosf(b[6]), sina = sinf(b[6]);
  const float sx[8] = {1, 1, -1, -1, 1, 1, -1, -1}, sy[8] = {-1, 1, 1, -1, -1, 1, 1, -1}, sz[8] = {-1, -1, -1, -1, 1, 1, 1, 1};
  BoxExtent e{INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY, true};
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float px = ex * (sx[k] / 2.f), py = ey * (sy[k] / 2.f), pz = ez * (sz[k] / 2.f);
    // row vector times [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]]
    const float rx = px * cosa + py * (-sina) + pz * 0.f + b[0];
    const float ry = px * sina + py * cosa + pz * 0.f + b[1];
    const float rz = px * 0.f + py * 0.f + pz * 1.f + b[2];
    u[k][0] = rx; u[k][1] = ry; u[k][2] = rz;
    const float X = T[0] * rx + T[1] * ry + T[2] * rz + T[3];
    const float Y = T[4] * rx + T[5] * ry + T[6] * rz + T[7];
    const float Z = T[8] * rx + T[9] * ry + T[10] * rz + T[11];
    c[k][0] = X; c[k][1] = Y; c[k][2] = Z;
    e.xmin = fminf(e.xmin, X); e.xmax = fmaxf(e.xmax, X);
    e.ymin = fminf(e.ymin, Y); e.ymax = fmaxf(e.ymax, Y);
    e.zmin = fminf(e.zmin, Z); e.zmax = fmaxf(e.zmax, Z);
    e.finite = e.finite && X - X == 0.f && Y - Y == 0.f && Z - Z == 0.f;
  }
  return e;
}

// box7 of anchor i after direction fix -> 8 projected corners; returns false when a size / z filter rejects it
__device__ __forceinline__ bool det_decode_one(const DetArgs& a, int i, float (&c)[8][3]) {
  const int HW = a.H * a.W;
  const int an = i % a.A, pix = i / a.A;
  float b[7];
  det_box7(a.reg, a.anchors + (size_t)i * 7, an, pix, HW, b);
  if (a.dir != nullptr) {
    int label = 0;
    float best = a.dir[(size_t)(an * a.nb) * HW + pix];
    for (int k = 1; k < a.nb; ++k) {
      const float v = a.dir[(size_t)(an * a.nb + k) * HW + pix];
      if (v > best) { best = v; label = k; }  // first maximum wins, like torch.max
    }
    const float period = (float)(2.0 * 3.14159265358979323846 / (double)a.nb);
    const float rot = limit_period_f(b[6] - a.dir_offset, 0.f, period);
    b[6] = rot + a.dir_offset + period * (float)label;
    b[6] = limit_period_f(b[6], 0.5f, (float)(2.0 * 3.14159265358979323846));
  }
  float u[8][3];
  const BoxExtent e = det_corners(b, a.hwl, a.T, u, c);
  const float x_len = e.xmax - e.xmin, y_len = e.ymax - e.ymin;
  // remove_large_pred_bbx: its "z extent" is the y extent again and is used as a truth value (non-zero)
  const bool size_ok = x_len <= 6.f && y_len <= 6.f && y_len != 0.f;
  const bool z_ok = e.zmin >= -3.f && e.zmax <= 1.f;
  return e.finite && size_ok && z_ok;
}

__device__ __forceinline__ float det_score(const DetArgs& a, int i) {
  const int HW = a.H * a.W;
  const int an = i % a.A, pix = i / a.A;
  const float x = a.cls[(size_t)an * HW + pix];
  return 1.0f / (1.0f + expf(-x));
}

// pass 1: score + all filters -> score_tmp (or -1) and the number of survivors per workgroup
__global__ __launch_bounds__(256) void det_flag_kernel(const DetArgs a) {
  __shared__ int s_cnt[4];
  const int n = a.H * a.W * a.A;
  const int i = blockIdx.x * 256 + threadIdx.x;
  float s = -1.f;
  if (i < n) {
    const float p = det_score(a, i);
    if (p > a.thr) {
      float c[8][3];
      if (det_decode_one(a, i, c)) s = p;
    }
    a.score_tmp[i] = s;
  }
  const unsigned long long m = __ballot(s >= 0.f);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0) a.block_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// pass 2: exclusive scan of the workgroup counts (single workgroup), starting at *count; *count += total
__global__ __launch_bounds__(1024) void det_scan_kernel(const int* __restrict__ block_count, int* __restrict__ block_off,
                                                       int nblocks, int* __restrict__ count) {
  __shared__ int s_part[1024];
  __shared__ int s_base;
  if (threadIdx.x == 0) s_base = *count;
  __syncthreads();
  for (int b0 = 0; b0 < nblocks; b0 += 1024) {
    const int i = b0 + threadIdx.x;
    const int v = i < nblocks ? block_count[i] : 0;
    s_part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
      const int t = threadIdx.x >= o ? s_part[threadIdx.x - o] : 0;
      __syncthreads();
      s_part[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nblocks) block_off[i] = s_base + s_part[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) s_base += s_part[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) *count = s_base;
}

// pass 3: survivors are written in anchor order (the order torch.masked_select produces)
__global__ __launch_bounds__(256) void det_emit_kernel(const DetArgs a) {
  __shared__ int s_cnt[4];
  const int n = a.H * a.W * a.A;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const float s = i < n ? a.score_tmp[i] : -1.f;
  const bool keep = s >= 0.f;
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) s_cnt[wv] = __popcll(m);
  __syncthreads();
  int base = a.block_off[blockIdx.x];
  for (int w = 0; w < wv; ++w) base += s_cnt[w];
  if (!keep) return;
  const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
  if (slot >= a.cap) return;  // the host compares *count with cap and fails loudly
  float c[8][3];
  det_decode_one(a, i, c);
  float* __restrict__ dst = a.corners + (size_t)slot * 24;
#pragma unroll
  for (int k = 0; k < 8; ++k) { dst[3 * k] = c[k][0]; dst[3 * k + 1] = c[k][1]; dst[3 * k + 2] = c[k][2]; }
  a.scores[slot] = s;
  a.anchor_idx[slot] = i;
}

// ---------------------------------------------------------------------------------------------
// Multi-class decoding (V2X-Real heads): VoxelPostprocessor.post_process_v2xreal, voxel_postprocessor.py:787-943.
// All agents of a call (up to kDetMaxAgents) go through ONE flag / scan / emit sequence: the per-agent pointers and sizes
// travel in the kernel arguments, and a workgroup covers 256 anchors of one agent.
// ---------------------------------------------------------------------------------------------
constexpr int kDetMaxAgents = 8;  // MAX_AGENTS_PER_SCENE of the Python package

struct DetMcAgent {
  const float* cls;      // [A*nc][H][W]   class k of anchor j in channel j*nc + k   (batch 1)
  const float* reg;      // [7A][H][W]
  const float* anchors;  // [H][W][A][7]   anchor j = class set * rotations + rotation
  const float* T;        // [4][4] row-major, agent -> ego
  int H, W;
  int block0;            // first workgroup of this agent in the launch
};

struct DetMcArgs {
  DetMcAgent ag[kDetMaxAgents];
  int n_agents, A, nc, hwl, cap;
  int append;                // 0: the launch starts the call (counters start at 0); 1: later chunk (counters are read)
  float thr;
  float* score_tmp;          // [nblocks*256] scratch: best sigmoid, or -1 at or below the threshold
  unsigned char* label_tmp;  // [nblocks*256] scratch: its class (0-based)
  int* block_count;          // [nblocks] scratch: candidates per workgroup
  int* block_bad;            // [nblocks] scratch: of those, the ones the size / z filters reject
  int* block_off;            // [nblocks] scratch
  float* corners;            // [cap][8][3] projected   (appended at *count)
  float* unprojected;        // [cap][8][3] or null
  float* scores;             // [cap]
  int* labels;               // [cap] 1-based class
  int* count;                // device: candidates so far
  int* violations;           // device: candidates so far that remove_large_pred_bbx_v2xreal / remove_bbx_abnormal_z_v2xreal reject
};

__device__ __forceinline__ int detmc_agent(const DetMcArgs& a) {
  int k = 0;
  while (k + 1 < a.n_agents && (int)blockIdx.x >= a.ag[k + 1].block0) ++k;
  return k;
}

// max over the class sigmoids, not the logits: two classes saturated to 1.0 tie, and the first wins (torch.max)
__device__ __forceinline__ float detmc_score(const DetMcArgs& a, const DetMcAgent& g, int i, int& label) {
  const int HW = g.H * g.W;
  const int an = i % a.A, pix = i / a.A;
  const float* __restrict__ p = g.cls + (size_t)(an * a.nc) * HW + pix;
  float best = 1.0f / (1.0f + expf(-p[0]));
  label = 0;
  for (int k = 1; k < a.nc; ++k) {
    const float v = 1.0f / (1.0f + expf(-p[(size_t)k * HW]));
    if (v > best) { best = v; label = k; }
  }
  return best;
}

// box of anchor i (no direction fix) -> unprojected and projected corners; false when remove_large_pred_bbx_v2xreal or
// remove_bbx_abnormal_z_v2xreal (box_utils.py:1115-1166) would remove it
__device__ __forceinline__ bool detmc_decode_one(const DetMcArgs& a, const DetMcAgent& g, int i, float (&u)[8][3], float (&c)[8][3]) {
  const int an = i % a.A, pix = i / a.A;
  float b[7];
  det_box7(g.reg, g.anchors + (size_t)i * 7, an, pix, g.H * g.W, b);
  const BoxExtent e = det_corners(b, a.hwl, g.T, u, c);
  const float x_len = e.xmax - e.xmin, y_len = e.ymax - e.ymin;
  // as in the single-class filter, the "z extent" is the y extent again, used as a truth value
  const bool size_ok = x_len <= 100.f && y_len <= 100.f && y_len != 0.f;
  const bool z_ok = e.zmin >= -100.f && e.zmax <= 100.f;
  return e.finite && size_ok && z_ok;
}

// pass 1: class max + score filter -> score_tmp / label_tmp; candidates and filter violations per workgroup
__global__ __launch_bounds__(256) void detmc_flag_kernel(const DetMcArgs a) {
  __shared__ int s_cnt[4], s_bad[4];
  const DetMcAgent& g = a.ag[detmc_agent(a)];
  const int n = g.H * g.W * a.A;
  const int i = ((int)blockIdx.x - g.block0) * 256 + threadIdx.x;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  float s = -1.f;
  bool bad = false;
  if (i < n) {
    int label;
    const float p = detmc_score(a, g, i, label);
    if (p > a.thr) {
      s = p;
      float u[8][3], c[8][3];
      bad = !detmc_decode_one(a, g, i, u, c);
    }
    a.score_tmp[t] = s;
    a.label_tmp[t] = (unsigned char)label;
  }
  const unsigned long long m = __ballot(s >= 0.f), mb = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    s_cnt[threadIdx.x >> 6] = __popcll(m);
    s_bad[threadIdx.x >> 6] = __popcll(mb);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.block_count[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    a.block_bad[blockIdx.x] = s_bad[0] + s_bad[1] + s_bad[2] + s_bad[3];
  }
}

// pass 2 (single workgroup): exclusive scan of the workgroup counts from *count (0 for the first chunk of a call); sum of the
// violations into *violations likewise
__global__ __launch_bounds__(1024) void detmc_scan_kernel(const DetMcArgs a, int nblocks) {
  __shared__ int s_part[1024];
  __shared__ int s_base, s_bad;
  if (threadIdx.x == 0) {
    s_base = a.append ? *a.count : 0;
    s_bad = a.append ? *a.violations : 0;
  }
  __syncthreads();
  int bad = 0;
  for (int b0 = 0; b0 < nblocks; b0 += 1024) {
    const int i = b0 + threadIdx.x;
    const int v = i < nblocks ? a.block_count[i] : 0;
    bad += i < nblocks ? a.block_bad[i] : 0;
    s_part[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan
      const int t = threadIdx.x >= o ? s_part[threadIdx.x - o] : 0;
      __syncthreads();
      s_part[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nblocks) a.block_off[i] = s_base + s_part[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) s_base += s_part[1023];
    __syncthreads();
  }
  if (bad) atomicAdd(&s_bad, bad);
  __syncthreads();
  if (threadIdx.x == 0) {
    *a.count = s_base;
    *a.violations = s_bad;
  }
}

// pass 3: candidates in the order of the reference's masked_select over the concatenated agents (agent, pixel, class set,
// rotation)
__global__ __launch_bounds__(256) void detmc_emit_kernel(const DetMcArgs a) {
  __shared__ int s_cnt[4];
  const DetMcAgent& g = a.ag[detmc_agent(a)];
  const int n = g.H * g.W * a.A;
  const int i = ((int)blockIdx.x - g.block0) * 256 + threadIdx.x;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  const float s = i < n ? a.score_tmp[t] : -1.f;
  const bool keep = s >= 0.f;
  const unsigned long long m = __ballot(keep);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) s_cnt[wv] = __popcll(m);
  __syncthreads();
  int base = a.block_off[blockIdx.x];
  for (int w = 0; w < wv; ++w) base += s_cnt[w];
  if (!keep) return;
  const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
  if (slot >= a.cap) return;  // the host compares *count with cap and fails loudly
  float u[8][3], c[8][3];
  detmc_decode_one(a, g, i, u, c);
  float* __restrict__ dst = a.corners + (size_t)slot * 24;
#pragma unroll
  for (int k = 0; k < 8; ++k) { dst[3 * k] = c[k][0]; dst[3 * k + 1] = c[k][1]; dst[3 * k + 2] = c[k][2]; }
  if (a.unprojected != nullptr) {
    float* __restrict__ du = a.unprojected + (size_t)slot * 24;
#pragma unroll
    for (int k = 0; k < 8; ++k) { du[3 * k] = u[k][0]; du[3 * k + 1] = u[k][1]; du[3 * k + 2] = u[k][2]; }
  }
  a.scores[slot] = s;
  a.labels[slot] = (int)a.label_tmp[t] + 1;
}

// after nms_rotated: [score, label] rows and the unprojected corners of the kept candidates, through out_index
__global__ __launch_bounds__(256) void detmc_gather_kernel(const int* __restrict__ out_index, const int* __restrict__ out_count,
                                                          const float* __restrict__ out_scores, const int* __restrict__ labels,
                                                          const float* __restrict__ unprojected, int cap, int top,
                                                          float* __restrict__ score_labels, float* __restrict__ out_unprojected) {
  const int m = min(*out_count, top);
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= m) return;
  const int src = out_index[t];
  if (src < 0 || src >= cap) return;
  score_labels[2 * t] = out_scores[t];
  score_labels[2 * t + 1] = (float)labels[src];
  if (unprojected != nullptr)
    for (int k = 0; k < 24; ++k) out_unprojected[(size_t)t * 24 + k] = unprojected[(size_t)src * 24 + k];
}

// ---------------------------------------------------------------------------------------------
// Rotated NMS
// ---------------------------------------------------------------------------------------------
constexpr int kNmsMaxN = 16384;  // candidates that fit the single-workgroup sort (128 KB of LDS)
constexpr int kNmsMaxTop = 1024;

// order[r] = index of the r-th candidate by (score descending, index descending) -- a stable ascending argsort read
// backwards -- for r < min(n, top).  One workgroup, bitonic sort in LDS.
__global__ __launch_bounds__(1024) void nms_sort_kernel(const float* __restrict__ scores, const int* __restrict__ n_dev,
                                                       int top, int* __restrict__ order, int* __restrict__ k_dev) {
  extern __shared__ unsigned long long s_key[];
  const int n = min(*n_dev, kNmsMaxN);
  int P = 1;
  while (P < n) P <<= 1;
  // key: larger = earlier.  The score's bit pattern with the sign bit set (score >= 0) or all bits inverted (score < 0) is
  // monotone over every finite float (for positive scores it is the plain bit order); ties -> larger index first
  for (int i = threadIdx.x; i < P; i += 1024) {
    const unsigned u = i < n ? __float_as_uint(scores[i]) : 0u;
    const unsigned key = u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
    s_key[i] = i < n ? ((unsigned long long)key << 32) | (unsigned)i : 0ull;
  }
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P; i += 1024) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long x = s_key[i], y = s_key[l];
          const bool desc = (i & k) == 0;  // descending overall
          if (desc ? x < y : x > y) { s_key[i] = y; s_key[l] = x; }
        }
      }
      __syncthreads();
    }
  }
  const int K = min(n, top);
  for (int i = threadIdx.x; i < K; i += 1024) order[i] = (int)(s_key[i] & 0xffffffffull);
  if (threadIdx.x == 0) *k_dev = K;
}

struct Pt { double x, y; };

__device__ __forceinline__ double poly_area(const Pt* p, int n) {
  if (n < 3) return 0.0;
  double s = 0.0;
  for (int i = 0; i < n; ++i) {
    const int j = i + 1 == n ? 0 : i + 1;
    s += p[i].x * p[j].y - p[j].x * p[i].y;
  }
  return 0.5 * s;
}

// Sutherland-Hodgman: part of `in` on the left of (or on) a->b
__device__ __forceinline__ int poly_clip(const Pt* in, int n, Pt a, Pt b, Pt* out) {
  if (n == 0) return 0;
  const double ex = b.x - a.x, ey = b.y - a.y;
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const int j = i + 1 == n ? 0 : i + 1;
    const double si = ex * (in[i].y - a.y) - ey * (in[i].x - a.x);
    const double sj = ex * (in[j].y - a.y) - ey * (in[j].x - a.x);
    if (si >= 0) out[m++] = in[i];
    if ((si > 0 && sj < 0) || (si < 0 && sj > 0)) {
      const double t = si / (si - sj);
      out[m].x = in[i].x + t * (in[j].x - in[i].x);
      out[m].y = in[i].y + t * (in[j].y - in[i].y);
      ++m;
    }
  }
  return m;
}

__device__ __forceinline__ double quad_iou_d(const float* __restrict__ ca, const float* __restrict__ cb) {
  Pt p[4], q[4];
  for (int k = 0; k < 4; ++k) { p[k] = {(double)ca[3 * k], (double)ca[3 * k + 1]}; q[k] = {(double)cb[3 * k], (double)cb[3 * k + 1]}; }
  double ap = poly_area(p, 4), aq = poly_area(q, 4);
  if (ap < 0) { Pt t = p[0]; p[0] = p[3]; p[3] = t; t = p[1]; p[1] = p[2]; p[2] = t; ap = -ap; }
  if (aq < 0) { Pt t = q[0]; q[0] = q[3]; q[3] = t; t = q[1]; q[1] = q[2]; q[2] = t; aq = -aq; }
  // a box without area shares no area with anything: exactly 0, where clipping against a rotated zero-width box left slivers of 1e-15
  if (ap == 0.0 || aq == 0.0) return 0.0;
  Pt buf0[12], buf1[12];
  int n = 4;
  for (int k = 0; k < 4; ++k) buf0[k] = p[k];
  Pt* cur = buf0; Pt* nxt = buf1;
  for (int e = 0; e < 4 && n > 0; ++e) {
    n = poly_clip(cur, n, q[e], q[(e + 1) & 3], nxt);
    Pt* t = cur; cur = nxt; nxt = t;
  }
  const double inter = fabs(poly_area(cur, n));
  const double uni = ap + aq - inter;
  return uni > 0 ? inter / uni : 0.0;
}

// diagnostic (gencomm_quad_iou_fwd): out[i][j] = the float64 IoU the mask kernel thresholds, one thread per pair
__global__ __launch_bounds__(256) void quad_iou_kernel(const float* __restrict__ corners_a, const float* __restrict__ corners_b,
                                                      double* __restrict__ out, int n_a, int n_b) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)n_a * n_b) return;
  const int i = (int)(t / n_b), j = (int)(t - (long long)i * n_b);
  out[t] = quad_iou_d(corners_a + (size_t)i * 24, corners_b + (size_t)j * 24);
}

// mask[i][w] bit b: candidate order[64 w + b] (ranked after i) overlaps candidate order[i] above the threshold
__global__ __launch_bounds__(64) void nms_mask_kernel(const float* __restrict__ corners, const int* __restrict__ order,
                                                     const int* __restrict__ k_dev, float thr,
                                                     unsigned long long* __restrict__ mask /*[kNmsMaxTop][kNmsMaxTop/64]*/) {
  const int K = *k_dev;
  const int i = blockIdx.x * 64 + threadIdx.x, w = blockIdx.y;
  if (i >= K) return;
  unsigned long long bits = 0ull;
  if (64 * w + 63 > i) {
    const float* __restrict__ ci = corners + (size_t)order[i] * 24;
    for (int b = 0; b < 64; ++b) {
      const int j = 64 * w + b;
      if (j > i && j < K) {
        const float iou = (float)quad_iou_d(ci, corners + (size_t)order[j] * 24);
        if (iou > thr) bits |= 1ull << b;
      }
    }
  }
  mask[(size_t)i * (kNmsMaxTop / 64) + w] = bits;
}

// greedy scan in rank order + range mask + ordered gather (single workgroup of 1024)
struct NmsOutArgs {
  const float* corners; const float* scores; const int* order; const int* k_dev;
  const unsigned long long* mask;
  const float* range6;  // may be null
  float* out_boxes; float* out_scores; int* out_index; int* out_count;
};
__global__ __launch_bounds__(1024) void nms_greedy_kernel(const NmsOutArgs a) {
  extern __shared__ unsigned long long s_mask[];  // [K][kNmsMaxTop / 64]: the serial scan reads LDS, not HBM
  __shared__ unsigned char s_keep[kNmsMaxTop];
  __shared__ int s_scan[1024];
  const int K = *a.k_dev;
  const int tid = threadIdx.x;
  for (int i = tid; i < K * (kNmsMaxTop / 64); i += 1024) s_mask[i] = a.mask[i];
  __syncthreads();
  if (tid < 64) {  // wave 0: lane l < 16 owns word l of the suppressed set
    unsigned long long removed = 0ull;
    for (int i = 0; i < K; ++i) {
      const unsigned long long wsel = __shfl(removed, i >> 6, 64);
      const bool kept = !((wsel >> (i & 63)) & 1ull);
      if (kept && tid < kNmsMaxTop / 64) removed |= s_mask[i * (kNmsMaxTop / 64) + tid];
      if (tid == 0) s_keep[i] = kept ? 1 : 0;
    }
  }
  __syncthreads();
  // range mask (all 8 corners inside, bounds inclusive), then ordered compaction
  bool out = false;
  int src = 0;
  if (tid < K && s_keep[tid]) {
    src = a.order[tid];
    out = true;
    if (a.range6 != nullptr) {
      const float* __restrict__ c = a.corners + (size_t)src * 24;
      for (int k = 0; k < 8; ++k)
        for (int d = 0; d < 3; ++d) out = out && c[3 * k + d] >= a.range6[d] && c[3 * k + d] <= a.range6[3 + d];
    }
  }
  s_scan[tid] = out ? 1 : 0;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {
    const int t = tid >= o ? s_scan[tid - o] : 0;
    __syncthreads();
    s_scan[tid] += t;
    __syncthreads();
  }
  if (out) {
    const int slot = s_scan[tid] - 1;
    const float* __restrict__ c = a.corners + (size_t)src * 24;
    for (int k = 0; k < 24; ++k) a.out_boxes[(size_t)slot * 24 + k] = c[k];
    a.out_scores[slot] = a.scores[src];
    a.out_index[slot] = src;
  }
  if (tid == 1023) *a.out_count = s_scan[1023];
}

// ---------------------------------------------------------------------------------------------
// bbox_overlaps (box_overlaps.pyx:17-57): one thread per entry of the (N, K) matrix; the entry itself is box_overlap.h's, which the
// target assignment (target_kernels.h) shares.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bbox_overlaps_kernel(const float* __restrict__ boxes, const float* __restrict__ query,
                                                           float* __restrict__ out, int N, int K) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)N * K) return;
  const int n = (int)(t / K), k = (int)(t - (long long)n * K);
  const float* b = boxes + (size_t)n * 4;
  const float* q = query + (size_t)k * 4;
  out[t] = bbox_overlap_one(b[0], b[1], b[2], b[3], q[0], q[1], q[2], q[3], bbox_query_area(q[0], q[1], q[2], q[3]));
}

#pragma clang fp contract(fast)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline long long det_workspace_bytes(int H, int W, int A) {
  const long long n = (long long)H * W * A, nb = (n + 255) / 256;
  return align_up(n * 4, 256) + 2 * align_up(nb * 4, 256);
}
inline long long nms_workspace_bytes() {
  return align_up(kNmsMaxTop * 4, 256) + 256 + (long long)kNmsMaxTop * (kNmsMaxTop / 64) * 8;
}

inline int det_decode_enqueue(DetArgs a, void* workspace, hipStream_t st) {
  const long long n = (long long)a.H * a.W * a.A;
  const int nblocks = (int)((n + 255) / 256);
  char* ws = (char*)workspace;
  a.score_tmp = (float*)ws;
  a.block_count = (int*)(ws + align_up(n * 4, 256));
  a.block_off = (int*)(ws + align_up(n * 4, 256) + align_up((long long)nblocks * 4, 256));
  det_flag_kernel<<<nblocks, 256, 0, st>>>(a);
  det_scan_kernel<<<1, 1024, 0, st>>>(a.block_count, a.block_off, nblocks, a.count);
  det_emit_kernel<<<nblocks, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// workgroups of the largest chunk of kDetMaxAgents agents
inline long long det_mc_max_chunk_blocks(const int* H, const int* W, int n_agents, int A) {
  long long best = 0;
  for (int c0 = 0; c0 < n_agents; c0 += kDetMaxAgents) {
    long long nb = 0;
    for (int k = c0; k < n_agents && k < c0 + kDetMaxAgents; ++k) nb += ((long long)H[k] * W[k] * A + 255) / 256;
    best = nb > best ? nb : best;
  }
  return best;
}
inline long long det_mc_workspace_bytes(const int* H, const int* W, int n_agents, int A) {
  const long long nb = det_mc_max_chunk_blocks(H, W, n_agents, A);
  return align_up(nb * 256 * 4, 256) + align_up(nb * 256, 256) + 3 * align_up(nb * 4, 256);
}

// three launches per chunk of kDetMaxAgents agents (one chunk up to MAX_AGENTS_PER_SCENE), whatever the number of agents in it
inline int det_mc_decode_enqueue(DetMcArgs a, const float* const* cls, const float* const* reg, const float* const* anchors,
                                 const float* const* T, const int* H, const int* W, int n_agents, void* workspace, hipStream_t st) {
  const long long nb_max = det_mc_max_chunk_blocks(H, W, n_agents, a.A);
  char* ws = (char*)workspace;
  a.score_tmp = (float*)ws;
  ws += align_up(nb_max * 256 * 4, 256);
  a.label_tmp = (unsigned char*)ws;
  ws += align_up(nb_max * 256, 256);
  a.block_count = (int*)ws;
  a.block_bad = (int*)(ws + align_up(nb_max * 4, 256));
  a.block_off = (int*)(ws + 2 * align_up(nb_max * 4, 256));
  for (int c0 = 0; c0 < n_agents; c0 += kDetMaxAgents) {
    const int na = n_agents - c0 < kDetMaxAgents ? n_agents - c0 : kDetMaxAgents;
    int nblocks = 0;
    for (int k = 0; k < na; ++k) {
      const int j = c0 + k;
      a.ag[k] = DetMcAgent{cls[j], reg[j], anchors[j], T[j], H[j], W[j], nblocks};
      nblocks += (int)(((long long)H[j] * W[j] * a.A + 255) / 256);
    }
    a.n_agents = na;
    a.append = c0 > 0;
    detmc_flag_kernel<<<nblocks, 256, 0, st>>>(a);
    detmc_scan_kernel<<<1, 1024, 0, st>>>(a, nblocks);
    detmc_emit_kernel<<<nblocks, 256, 0, st>>>(a);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

inline int nms_rotated_enqueue(const float* corners, const float* scores, const int* n_dev, float thr, int top, const float* range6,
                               float* out_boxes, float* out_scores, int* out_index, int* out_count, void* workspace, hipStream_t st) {
  char* ws = (char*)workspace;
  int* order = (int*)ws;
  int* k_dev = (int*)(ws + align_up(kNmsMaxTop * 4, 256));
  unsigned long long* mask = (unsigned long long*)(ws + align_up(kNmsMaxTop * 4, 256) + 256);
  static LdsAttrOnce attr_sort, attr_greedy;
  if (const int rc = attr_sort.set(nms_sort_kernel, kNmsMaxN * 8)) return rc;
  if (const int rc = attr_greedy.set(nms_greedy_kernel, kNmsMaxTop * (kNmsMaxTop / 64) * 8)) return rc;
  nms_sort_kernel<<<1, 1024, kNmsMaxN * 8, st>>>(scores, n_dev, top, order, k_dev);
  nms_mask_kernel<<<dim3(kNmsMaxTop / 64, kNmsMaxTop / 64), 64, 0, st>>>(corners, order, k_dev, thr, mask);
  NmsOutArgs o{corners, scores, order, k_dev, mask, range6, out_boxes, out_scores, out_index, out_count};
  nms_greedy_kernel<<<1, 1024, kNmsMaxTop * (kNmsMaxTop / 64) * 8, st>>>(o);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

}  // namespace gc
