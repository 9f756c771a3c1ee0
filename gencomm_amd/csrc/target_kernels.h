// Training-time anchor target assignment on the device (gfx950, wave64): pos_equal_one / neg_equal_one / targets of
// VoxelPostprocessor.generate_label and the label map / targets / neg_equal_one of generate_label_v2xreal, for every sample of a
// batch and every class in two launches, without forming the anchors x boxes IoU matrix.  SURVEY.md 8f rank 3.
//
// Reference (numpy + torch-CPU + Cython there, once per sample in every dataloader worker):
//   generate_label, generate_label_v2xreal   opencood/data_utils/post_processor/voxel_postprocessor.py:188-310, :312-463
//   boxes_to_corners_3d, corner2d_to_standup_box   opencood/utils/box_utils.py:152-204, :225-248
//   rotate_points_along_z                    opencood/utils/common_utils.py:139-161
//   bbox_overlaps                            opencood/utils/box_overlaps.pyx:17-57 (box_overlap.h)
//
// What the reference's index logic (:250-303) amounts to, per anchor a and (compacted) box j with IoU[a][j]:
//   best[j]  = the lowest anchor index among the maxima of column j (np.argmax), kept only when that maximum is > 0
//   pos[a]   = some IoU[a][j] > pos_threshold, or a == best[j] for some j
//   match[a] = the lowest j with IoU[a][j] > pos_threshold, else the lowest j with best[j] == a
//              (np.where is row-major, np.unique(return_index=True) keeps the first occurrence of a in [id_pos, id_highest])
//   neg[a]   = every IoU[a][j] < neg_threshold, and a is no best[j]
// Launch 1 finds best[] -- a 64-bit maximum over (IoU bits, ~anchor index) per box, columns whose maximum is 0 never publish --
// and launch 2 recomputes the row of IoUs of its anchor against the boxes in LDS and writes that anchor's complete outputs.
//
// The per-box keys live in a caller-owned workspace that is ZERO when a call starts: the caller zeroes it once when it allocates it,
// and launch 2 leaves it zero again (the last workgroup of a (sample, class) to have read the keys clears them), so that no call needs
// a memset.  0 is below every published key (the low word ~anchor is never 0).
//
// Arithmetic mirrors the reference op by op with contraction off: float32 corners (cos / sin, the 2x2 product, + centre), float32
// stand-up boxes, the overlap of box_overlap.h, float64 deltas from the float64 anchors and the box row as given.
#pragma once
#include "common.h"
#include "box_overlap.h"

namespace gc {

#pragma clang fp contract(off)

constexpr int kTargetMaxBoxes = 256;   // max_num: one thread of a 256-thread workgroup per box slot
constexpr int kTargetMaxClasses = 8;

// boxes_to_corners_3d ('hwl': extents l = b[5], w = b[4]) -> corner2d_to_standup_box -> float32; z does not reach the stand-up box
__device__ __forceinline__ float4 target_standup(const float (&b)[7], int hwl) {
  const float ex = hwl ? b[5] : b[3], ey = b[4];
  const float cosa = cosf(b[6]), sina = sinf(b[6]);
  const float sx[4] = {1, 1, -1, -1}, sy[4] = {-1, 1, 1, -1};
  float x1 = INFINITY, y1 = INFINITY, x2 = -INFINITY, y2 = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float px = ex * (sx[k] / 2.f), py = ey * (sy[k] / 2.f);
    // row vector times [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]], then += centre
    const float rx = px * cosa + py * (-sina) + b[0];
    const float ry = px * sina + py * cosa + b[1];
    x1 = fminf(x1, rx); x2 = fmaxf(x2, rx);
    y1 = fminf(y1, ry); y2 = fmaxf(y2, ry);
  }
  return make_float4(x1, y1, x2, y2);
}

// anchors [n][7] float64 -> stand-up boxes [n][4] float32 (the `.float()` of check_numpy_to_torch first); once per anchor array
__global__ __launch_bounds__(256) void target_standup_kernel(const double* __restrict__ anchors, int n, int hwl, float4* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float b[7];
#pragma unroll
  for (int d = 0; d < 7; ++d) b[d] = (float)anchors[(size_t)i * 7 + d];
  out[i] = target_standup(b, hwl);
}

struct TargetArgs {
  const void* boxes;     // [B][max_num][width], float32 or float64
  const void* mask;      // [B][max_num]
  const double* anchors[kTargetMaxClasses];   // per class [n][7], n = HW * R, anchor i = pixel * R + rotation
  const float4* standup[kTargetMaxClasses];   // per class [n] (target_standup_kernel)
  float pos_thr[kTargetMaxClasses], neg_thr[kTargetMaxClasses];   // compared in float32, as numpy compares a float32 array with a Python float
  unsigned long long* keys;   // [B][nc][max_num]
  unsigned* arrived;          // [B][nc]
  void* pos;       // [B][HW][nc * R]: 1 / 0, or (multiclass) the label map -1 / 0 / class id
  void* neg;       // [B][HW][R], of the last class
  void* targets;   // [B][HW][nc * R][7]
  int B, nc, max_num, n, R, width, box_f64, mask_dtype, multiclass;
};

__device__ __forceinline__ double target_box_value(const TargetArgs& a, int b, int row, int col) {
  const size_t at = ((size_t)b * a.max_num + row) * a.width + col;
  return a.box_f64 ? ((const double*)a.boxes)[at] : (double)((const float*)a.boxes)[at];
}
__device__ __forceinline__ bool target_mask_is_one(const TargetArgs& a, int b, int row) {
  const size_t at = (size_t)b * a.max_num + row;
  switch (a.mask_dtype) {
    case 0: return ((const float*)a.mask)[at] == 1.f;
    case 1: return ((const double*)a.mask)[at] == 1.0;
    case 2: return ((const int*)a.mask)[at] == 1;
    case 3: return ((const long long*)a.mask)[at] == 1;
    default: return ((const unsigned char*)a.mask)[at] == 1;
  }
}

// The valid boxes of (sample b, class k) in input order: s_src[j] = source row of compacted box j, s_gt[j] / s_area[j] = its float32
// stand-up box and query area. Returns their number. 256 threads, one per box slot; ends in a barrier.
__device__ __forceinline__ int target_compact_boxes(const TargetArgs& a, int b, int k, int* s_src, float4* s_gt, float* s_area, int* s_wave) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bool valid = false;
  if (tid < a.max_num) {
    valid = target_mask_is_one(a, b, tid);
    // `gt[:, -1] - 1 == i` on the rows that passed the mask, in the boxes' own precision
    if (valid && a.multiclass) valid = a.box_f64 ? (target_box_value(a, b, tid, a.width - 1) - 1.0 == (double)k)
                                                 : ((float)target_box_value(a, b, tid, a.width - 1) - 1.f == (float)k);
  }
  const unsigned long long bal = __ballot(valid);
  if (lane == 0) s_wave[wave] = __popcll(bal);
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += s_wave[w];
  const int n = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  if (valid) {
    const int j = before + __popcll(bal & ((1ull << lane) - 1ull));
    float v[7];
#pragma unroll
    for (int d = 0; d < 7; ++d) v[d] = (float)target_box_value(a, b, tid, d);   // check_numpy_to_torch(...).float()
    const float4 s = target_standup(v, 1);
    s_src[j] = tid;
    s_gt[j] = s;
    s_area[j] = bbox_query_area(s.x, s.y, s.z, s.w);
  }
  __syncthreads();
  return n;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    v = other > v ? other : v;
  }
  return v;
}

// Launch 1: per box, the maximum over all anchors of (IoU bits << 32 | ~anchor): IoU >= 0 orders like its bit pattern, and among
// equal IoUs the lowest anchor index has the largest complement (np.argmax's first maximum). grid (ceil(n / 256), nc, B).
__global__ __launch_bounds__(256) void target_best_anchor_kernel(const TargetArgs a) {
  __shared__ int s_src[kTargetMaxBoxes];
  __shared__ float4 s_gt[kTargetMaxBoxes];
  __shared__ float s_area[kTargetMaxBoxes];
  __shared__ unsigned long long s_key[kTargetMaxBoxes];
  __shared__ int s_wave[4];
  const int k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  s_key[tid] = 0ull;
  const int nb = target_compact_boxes(a, b, k, s_src, s_gt, s_area, s_wave);   // its barriers also order the s_key stores
  if (nb == 0) return;
  const int i = blockIdx.x * 256 + tid;
  const bool live = i < a.n;
  const float4 an = live ? a.standup[k][i] : make_float4(0.f, 0.f, 0.f, 0.f);
  for (int j = 0; j < nb; ++j) {
    const float4 g = s_gt[j];
    const float iou = live ? bbox_overlap_one(an.x, an.y, an.z, an.w, g.x, g.y, g.z, g.w, s_area[j]) : 0.f;
    // a column's zeros never matter (:254 drops a best IoU of 0): the wave reduces only where one of its anchors overlaps the box
    if (__ballot(iou > 0.f) != 0ull) {
      const unsigned long long key = iou > 0.f ? ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)~(unsigned)i : 0ull;
      const unsigned long long best = wave_max_u64(key);
      if ((tid & 63) == 0) atomicMax(&s_key[j], best);
    }
  }
  __syncthreads();
  if (tid < nb && s_key[tid] != 0ull) atomicMax(&a.keys[((size_t)b * a.nc + k) * a.max_num + tid], s_key[tid]);
}

// Launch 2: one thread per anchor writes that anchor's complete outputs, zeros included. Same grid.
template <typename T>
__global__ __launch_bounds__(256) void target_assign_kernel(const TargetArgs a) {
  __shared__ int s_src[kTargetMaxBoxes];
  __shared__ float4 s_gt[kTargetMaxBoxes];
  __shared__ float s_area[kTargetMaxBoxes];
  __shared__ unsigned s_best[kTargetMaxBoxes];   // best anchor of box j, 0xffffffff when its best IoU is 0
  __shared__ int s_wave[4];
  __shared__ int s_last;
  const int k = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const int nb = target_compact_boxes(a, b, k, s_src, s_gt, s_area, s_wave);
  unsigned long long* keys = a.keys + ((size_t)b * a.nc + k) * a.max_num;
  if (nb > 0) {   // block-uniform
    if (tid < nb) {
      const unsigned long long key = keys[tid];
      s_best[tid] = key != 0ull ? ~(unsigned)key : 0xffffffffu;
    }
    __syncthreads();
    // the keys go back to zero for the next call once every workgroup of this (sample, class) has read them
    if (tid == 0) {
      __threadfence();
      const unsigned seen = atomicAdd(&a.arrived[b * a.nc + k], 1u);
      s_last = seen == gridDim.x - 1;
    }
    __syncthreads();
    if (s_last) {
      if (tid < nb) keys[tid] = 0ull;
      if (tid == 0) a.arrived[b * a.nc + k] = 0u;
    }
  }
  const int i = blockIdx.x * 256 + tid;
  if (i >= a.n) return;
  const float pos_thr = a.pos_thr[k], neg_thr = a.neg_thr[k];
  int first_pos = -1, first_best = -1;
  bool all_below = true;
  if (nb > 0) {
    const float4 an = a.standup[k][i];
    for (int j = 0; j < nb; ++j) {
      const float4 g = s_gt[j];
      const float iou = bbox_overlap_one(an.x, an.y, an.z, an.w, g.x, g.y, g.z, g.w, s_area[j]);
      if (iou > pos_thr && first_pos < 0) first_pos = j;
      if (!(iou < neg_thr)) all_below = false;
      if (s_best[j] == (unsigned)i && first_best < 0) first_best = j;
    }
  }
  const int match = first_pos >= 0 ? first_pos : first_best;
  const bool pos = match >= 0;
  const bool neg = all_below && first_best < 0;
  const int R = a.R, S = a.nc * R;
  const int pix = i / R, r = i - pix * R;
  const size_t HW = (size_t)(a.n / R);
  const size_t slot = ((size_t)b * HW + pix) * S + (size_t)k * R + r;
  double t[7] = {0, 0, 0, 0, 0, 0, 0};
  double label = a.multiclass ? (all_below ? 0.0 : -1.0) : 0.0;   // :351, :435; the positives overwrite last (:446)
  if (pos) {
    // generate_label reads row `match` of the UNFILTERED boxes (:279) although the IoUs are those of the compacted ones;
    // generate_label_v2xreal filters first (:337, :342) and reads the compacted box itself
    const int row = a.multiclass ? s_src[match] : match;
    const double* __restrict__ an = a.anchors[k] + (size_t)i * 7;
    double g[7];
#pragma unroll
    for (int d = 0; d < 7; ++d) g[d] = target_box_value(a, b, row, d);
    const double diag = sqrt(an[4] * an[4] + an[5] * an[5]);
    t[0] = (g[0] - an[0]) / diag;
    t[1] = (g[1] - an[1]) / diag;
    t[2] = (g[2] - an[2]) / an[3];
    t[3] = log(g[3] / an[3]);
    t[4] = log(g[4] / an[4]);
    t[5] = log(g[5] / an[5]);
    t[6] = g[6] - an[6];
    label = a.multiclass ? target_box_value(a, b, row, a.width - 1) : 1.0;
  }
  ((T*)a.pos)[slot] = (T)label;
  if (k == a.nc - 1) ((T*)a.neg)[((size_t)b * HW + pix) * R + r] = (T)(neg ? 1.0 : 0.0);
  T* __restrict__ out = (T*)a.targets + slot * 7;
#pragma unroll
  for (int d = 0; d < 7; ++d) out[d] = (T)t[d];
}

#pragma clang fp contract(fast)

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline long long target_workspace_bytes(int B, int nc, int max_num) {
  return (long long)align_up((size_t)B * nc * max_num * sizeof(unsigned long long), 256) + (long long)align_up((size_t)B * nc * sizeof(unsigned), 256);
}

inline int target_assign_enqueue(TargetArgs a, void* workspace, int out_f64, hipStream_t st) {
  a.keys = (unsigned long long*)workspace;
  a.arrived = (unsigned*)((char*)workspace + align_up((size_t)a.B * a.nc * a.max_num * sizeof(unsigned long long), 256));
  const dim3 grid((unsigned)((a.n + 255) / 256), (unsigned)a.nc, (unsigned)a.B);
  target_best_anchor_kernel<<<grid, 256, 0, st>>>(a);
  if (out_f64) target_assign_kernel<double><<<grid, 256, 0, st>>>(a);
  else target_assign_kernel<float><<<grid, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

}  // namespace gc
