// Second translation unit of libgencomm_hip.so: iou3d_nms (reference extension semantics), the point-cloud voxeliser,
// the V2X-ViT attention kernels, the sparse 3-D convolutions of the SECOND encoder, the Lift-Splat-Shoot camera encoder
// the training-time anchor target assignment, the batched lidar front end, CoBEVT's swap attention, V2VNet's message passing,
// the CodeFilling codec and STAMP's ConvNeXt block.
// Kept apart from gencomm_abi.hip so that the rocPRIM templates do not lengthen the hot path's compile.
#include "../../include/gencomm_hip.h"

#include <algorithm>

#include "common.h"
#include "codebook_bwd_kernels.h"
#include "codebook_kernels.h"
#include "convnext_bwd_kernels.h"
#include "convnext_kernels.h"
#include "criteria_kernels.h"
#include "iou3d_kernels.h"
#include "loss_kernels.h"
#include "lss_kernels.h"
#include "mpda_bwd_kernels.h"
#include "mpda_kernels.h"
#include "pyramid_bwd_kernels.h"
#include "pyramid_kernels.h"
#include "sparse_kernels.h"
#include "swap_attn_bwd_kernels.h"
#include "swap_attn_kernels.h"
#include "target_kernels.h"
#include "v2v_kernels.h"
#include "v2xvit_kernels.h"
#include "voxel_batch_kernels.h"
#include "voxel_kernels.h"

using namespace gc;

extern "C" {

int gencomm_iou3d_pairwise_fwd(const float* boxes_a, int num_a, const float* boxes_b, int num_b, int mode, float* out, void* stream) {
  GC_CHECK_ARG(num_a >= 0 && num_b >= 0 && (mode == 0 || mode == 1), "bad num_a / num_b / mode");
  if (num_a == 0 || num_b == 0) return GC_OK;
  GC_CHECK_ARG(boxes_a && boxes_b && out, "null pointer");
  const long long total = (long long)num_a * num_b;
  GC_CHECK_ARG((total + 255) / 256 < (1LL << 31), "num_a * num_b too large");
  iou3d_pairwise_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(boxes_a, num_a, boxes_b, num_b, mode, out);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_iou3d_max_boxes(void) { return kIou3dMaxBoxes; }
long long gencomm_iou3d_nms_workspace_bytes(int n) {
  if (n < 0 || n > kIou3dMaxBoxes) { fail(GC_ERR_ARG, "n out of range (gencomm_iou3d_max_boxes)"); return -1; }
  return (long long)align_up((size_t)std::max(n, 1) * ((std::max(n, 1) + 63) / 64) * sizeof(unsigned long long), 256);
}

int gencomm_iou3d_nms_fwd(const float* boxes, int n, float thresh, int normal, long long* keep, int* count,
                          void* workspace, long long workspace_bytes, void* stream) {
  GC_CHECK_ARG(n >= 0 && n <= kIou3dMaxBoxes, "n out of range (gencomm_iou3d_max_boxes)");
  GC_CHECK_ARG(count != nullptr, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    GC_HIP(hipMemsetAsync(count, 0, sizeof(int), st));
    return GC_OK;
  }
  GC_CHECK_ARG(boxes && keep && workspace, "null pointer");
  if (gencomm_iou3d_nms_workspace_bytes(n) > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_iou3d_nms_workspace_bytes)");
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(workspace);
  const int cb = (n + 63) / 64;
  if (normal) iou3d_nms_mask_kernel<true><<<dim3(cb, cb), 64, 0, st>>>(n, thresh, boxes, mask);
  else iou3d_nms_mask_kernel<false><<<dim3(cb, cb), 64, 0, st>>>(n, thresh, boxes, mask);
  iou3d_nms_reduce_kernel<<<1, 64, 0, st>>>(n, mask, keep, count);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

static int voxel_args(VoxelArgs& a, const float* points, int n, int nfeat, const float* voxel_size3, const float* range6, int max_points, int max_voxels) {
  GC_CHECK_ARG(n >= 0 && nfeat >= 3 && max_points >= 1 && max_voxels >= 1 && voxel_size3 && range6, "bad n / nfeat / max_points / max_voxels");
  a.points = points; a.n = n; a.nfeat = nfeat; a.max_points = max_points; a.max_voxels = max_voxels;
  long long cells = 1;
  for (int j = 0; j < 3; ++j) {
    a.vs[j] = voxel_size3[j]; a.r0[j] = range6[j];
    GC_CHECK_ARG(voxel_size3[j] > 0.f, "voxel size must be positive");
    a.grid[j] = (int)lrintf((range6[3 + j] - range6[j]) / voxel_size3[j]);  // np.round((range[3:6] - range[0:3]) / voxel_size), sp_voxel_preprocessor.py:37-39
    GC_CHECK_ARG(a.grid[j] >= 1, "empty grid");
    cells *= a.grid[j];
  }
  GC_CHECK_ARG(cells < 0xFFFFFFFFLL, "grid has too many cells for 32-bit keys");
  return GC_OK;
}

long long gencomm_voxelize_workspace_bytes(int n) {
  if (n < 0) { fail(GC_ERR_ARG, "n must be non-negative"); return -1; }
  return (long long)voxel_ws(n).total;
}

int gencomm_voxelize_fwd(const float* points, int n, int nfeat, const float* voxel_size3, const float* range6, int max_points, int max_voxels,
                         float* voxels, int* coords_zyx, int* num_points, int* count, void* workspace, long long workspace_bytes, void* stream) {
  VoxelArgs a{};
  if (int rc = voxel_args(a, points, n, nfeat, voxel_size3, range6, max_points, max_voxels)) return rc;
  GC_CHECK_ARG(voxels && coords_zyx && num_points && count && workspace && (n == 0 || points), "null pointer");
  if ((long long)voxel_ws(n).total > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_voxelize_workspace_bytes)");
  return voxelize_enqueue(a, voxels, coords_zyx, num_points, count, (char*)workspace, (hipStream_t)stream);
}

long long gencomm_voxelize_batch_workspace_bytes(int n, int A, int max_voxels) {
  if (n < 0 || A < 1 || max_voxels < 1) { fail(GC_ERR_ARG, "n must be non-negative, A and max_voxels positive"); return -1; }
  return (long long)voxel_batch_ws(n, A, (int)std::min<long long>((long long)A * max_voxels, n)).total;
}

int gencomm_voxelize_batch_fwd(const float* points, int n, int nfeat, const int* offsets, int A, const float* transforms, const int* perm, int mask_ego,
                               const float* voxel_size3, const float* range6, int max_points, int max_voxels, int cap_rows, float* voxels,
                               int* coords_azyx, int* num_points, int* counts, int* total, void* workspace, long long workspace_bytes, void* stream) {
  GC_CHECK_ARG(n >= 0 && A >= 1 && nfeat >= 3 && max_points >= 1 && max_voxels >= 1 && voxel_size3 && range6, "bad n / A / nfeat / max_points / max_voxels");
  VoxelBatchArgs a{};
  a.points = points; a.offsets = offsets; a.tfm = transforms; a.perm = perm;
  a.n = n; a.nfeat = nfeat; a.A = A; a.mask_ego = mask_ego ? 1 : 0; a.max_points = max_points; a.max_voxels = max_voxels;
  double cells = 1.0;
  a.ncells = 1;
  for (int j = 0; j < 3; ++j) {
    a.vs[j] = voxel_size3[j]; a.r0[j] = range6[j];
    GC_CHECK_ARG(voxel_size3[j] > 0.f, "voxel size must be positive");
    const float g = rintf((range6[3 + j] - range6[j]) / voxel_size3[j]);   // as gencomm_voxelize_fwd: np.round((range[3:6] - range[0:3]) / voxel_size)
    GC_CHECK_ARG(g >= 1.f, "empty grid");
    GC_CHECK_ARG(g < 2147483648.f, "more than 2^31 - 1 cells along one axis");
    a.grid[j] = (int)g;
    cells *= (double)a.grid[j];
  }
  GC_CHECK_ARG((double)A * cells < 9.2e18, "A * cells does not fit the 64-bit keys (limit 2^63)");
  a.ncells = (unsigned long long)a.grid[0] * a.grid[1] * a.grid[2];
  const long long cap = std::min<long long>((long long)A * max_voxels, n);
  GC_CHECK_ARG(cap_rows == cap, "cap_rows must be min(A * max_voxels, n)");
  a.cap_rows = cap_rows;
  GC_CHECK_ARG(offsets && counts && total && workspace, "null pointer");
  GC_CHECK_ARG(n == 0 || (points && voxels && coords_azyx && num_points), "null pointer");
  GC_CHECK_ARG(((uintptr_t)coords_azyx & 15) == 0, "coords must be 16-byte aligned");
  if ((long long)voxel_batch_ws(n, A, cap_rows).total > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_voxelize_batch_workspace_bytes)");
  const bool vec4 = nfeat == 4 && (((uintptr_t)points | (uintptr_t)voxels) & 15) == 0;
  return voxelize_batch_enqueue(a, vec4, voxels, coords_azyx, num_points, counts, total, (char*)workspace, (hipStream_t)stream);
}

int gencomm_warp_affine_fwd(const float* x, const double* theta, float* out, int n, int C, int H, int W, void* stream) {
  GC_CHECK_ARG(x && theta && out && n >= 1 && n <= 65535 && C >= 1 && H >= 1 && W >= 1, "bad arguments");
  WarpArgs a{x, theta, out, C, H, W};
  warp_affine_kernel<<<dim3((H * W + 255) / 256, n), 256, 0, (hipStream_t)stream>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_hgt_attn_fwd(const float* qkv, const int* scene_off, float* out, int B, int heads, int dim_head, int HW, void* stream) {
  GC_CHECK_ARG(qkv && scene_off && out && B >= 1 && B <= 65535 && heads >= 1 && heads <= 65535 && HW >= 1, "bad arguments");
  GC_CHECK_ARG(B <= 65535 / 8, "too many scenes in one launch");
  HgtArgs a{qkv, scene_off, out, heads, HW, 1.0f / sqrtf((float)dim_head)};
  const dim3 grid((HW + 255) / 256, heads, B * 8);  // 8 query-agent slots per scene (v2xvit_kernels.h)
  hipStream_t st = (hipStream_t)stream;
  if ((long long)HW * heads * B >= 131072 && (dim_head == 16 || dim_head == 32)) {   // enough (pixel, head) threads to fill the machine: every value loaded once
    const dim3 gs((HW + 255) / 256, heads, B);
    GC_KLOG("hgt_attn_stream_kernel");
    if (dim_head == 32) hgt_attn_stream_kernel<32><<<gs, 256, 0, st>>>(a);
    else hgt_attn_stream_kernel<16><<<gs, 256, 0, st>>>(a);
    GC_HIP(hipGetLastError());
    return GC_OK;
  }
  if (dim_head == 32) hgt_attn_kernel<32><<<grid, 256, 0, st>>>(a);
  else if (dim_head == 64) hgt_attn_kernel<64><<<grid, 256, 0, st>>>(a);
  else if (dim_head == 16) hgt_attn_kernel<16><<<grid, 256, 0, st>>>(a);
  else if (dim_head == 8) hgt_attn_kernel<8><<<grid, 256, 0, st>>>(a);
  else return fail(GC_ERR_ARG, "hgt attention: dim_head must be 8, 16, 32 or 64");
  GC_KLOG("hgt_attn_kernel");
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_win_attn_fwd(const float* qkv, const float* pos_embedding, float* out, int n, int heads, int dim_head, int window, int H, int W,
                         void* stream) {
  GC_CHECK_ARG(qkv && pos_embedding && out && n >= 1 && n <= 65535 && heads >= 1 && heads <= 65535, "bad arguments");
  GC_CHECK_ARG(H >= window && W >= window && H % window == 0 && W % window == 0, "H and W must be multiples of the window size");
  WinArgs a{qkv, pos_embedding, out, heads, H, W, 1.0f / sqrtf((float)dim_head)};
  hipStream_t st = (hipStream_t)stream;
  if (window == 4 && dim_head == 16) return win_attn_launch<16, 4>(a, n, st);
  if (window == 8 && dim_head == 32) return win_attn_launch<32, 8>(a, n, st);
  if (window == 16 && dim_head == 64) return win_attn_launch<64, 16>(a, n, st);
  if (window == 4 && dim_head == 32) return win_attn_launch<32, 4>(a, n, st);
  if (window == 8 && dim_head == 16) return win_attn_launch<16, 8>(a, n, st);
  if (window == 8 && dim_head == 64) return win_attn_launch<64, 8>(a, n, st);
  if (window == 16 && dim_head == 32) return win_attn_launch<32, 16>(a, n, st);
  return fail(GC_ERR_ARG, "window attention: supported (window, dim_head) pairs are (4,16) (4,32) (8,16) (8,32) (8,64) (16,32) (16,64)");
}

// ---- CoBEVT (swap_attn_kernels.h) ---------------------------------------------------------------------------------------
static int swap_attn_check(int B, int L, int heads, int dim_head, int window, int H, int W, int grid_mode) {
  GC_CHECK_ARG(B >= 1 && B <= 65535 && heads >= 1 && heads <= 65535, "swap attention: 1..65535 scenes and heads");
  GC_CHECK_ARG(L >= 1 && L <= kSwapMaxAgents, "swap attention: agent_size (L) must be 1..8");
  GC_CHECK_ARG(grid_mode == 0 || grid_mode == 1, "swap attention: grid_mode must be 0 (window partition) or 1 (grid partition)");
  GC_CHECK_ARG(window == 4 || window == 8, "swap attention: window_size must be 4 or 8");
  GC_CHECK_ARG(dim_head == 16 || dim_head == 32 || dim_head == 64, "swap attention: dim_head must be 16, 32 or 64");
  GC_CHECK_ARG(H >= window && W >= window && H % window == 0 && W % window == 0, "swap attention: H and W must be multiples of window_size");
  GC_CHECK_ARG((long long)H * W * 3 * heads * dim_head < (1LL << 31), "swap attention: one agent's qkv map must stay below 2^31 elements");
  return GC_OK;
}

int gencomm_swap_attn_fwd(const float* qkv, const float* bias_table, const int* num_agents, float* out, int B, int L, int heads, int dim_head,
                          int window, int H, int W, int grid_mode, void* stream) {
  GC_CHECK_ARG(qkv && bias_table && num_agents && out, "null pointer");
  if (int rc = swap_attn_check(B, L, heads, dim_head, window, H, W, grid_mode)) return rc;
  SwapArgs a{qkv, bias_table, num_agents, out, L, heads, H, W, grid_mode, 0, 0, 1.0f / sqrtf((float)dim_head), nullptr};
  return swap_attn_dispatch<false>(a, B, dim_head, window, (hipStream_t)stream);
}

int gencomm_swap_attn_train_fwd(const float* qkv, const float* bias_table, const int* num_agents, float* out, float* lse, int B, int L, int heads,
                                int dim_head, int window, int H, int W, int grid_mode, void* stream) {
  GC_CHECK_ARG(qkv && bias_table && num_agents && out && lse, "null pointer");
  if (int rc = swap_attn_check(B, L, heads, dim_head, window, H, W, grid_mode)) return rc;
  SwapArgs a{qkv, bias_table, num_agents, out, L, heads, H, W, grid_mode, 0, 0, 1.0f / sqrtf((float)dim_head), lse};
  return swap_attn_dispatch<true>(a, B, dim_head, window, (hipStream_t)stream);
}

int gencomm_swap_attn_bwd(const float* qkv, const float* bias_table, const int* num_agents, const float* out, const float* lse, const float* dout,
                          float* dqkv, float* dtable, int B, int L, int heads, int dim_head, int window, int H, int W, int grid_mode,
                          void* stream) {
  GC_CHECK_ARG(qkv && bias_table && num_agents && out && lse && dout && dqkv && dtable, "null pointer");
  if (int rc = swap_attn_check(B, L, heads, dim_head, window, H, W, grid_mode)) return rc;
  SwapBwdArgs a{qkv, bias_table, num_agents, out, lse, dout, dqkv, dtable, L, heads, H, W, grid_mode, 0, 0, 0, 1.0f / sqrtf((float)dim_head)};
  hipStream_t st = (hipStream_t)stream;
  if (window == 4 && dim_head == 16) return swap_attn_bwd_launch<16, 4>(a, B, st);
  if (window == 4 && dim_head == 32) return swap_attn_bwd_launch<32, 4>(a, B, st);
  if (window == 4 && dim_head == 64) return swap_attn_bwd_launch<64, 4>(a, B, st);
  if (window == 8 && dim_head == 16) return swap_attn_bwd_launch<16, 8>(a, B, st);
  if (window == 8 && dim_head == 32) return swap_attn_bwd_launch<32, 8>(a, B, st);
  return swap_attn_bwd_launch<64, 8>(a, B, st);
}

int gencomm_agent_mean_fwd(const float* x, float* out, int B, int L, long long count, void* stream) {
  GC_CHECK_ARG(x && out, "null pointer");
  GC_CHECK_ARG(B >= 1 && B <= 65535 && L >= 1 && count >= 1 && (count + 255) / 256 < (1LL << 31), "agent mean: bad B / L / count");
  agent_mean_kernel<<<dim3((unsigned)((count + 255) / 256), B), 256, 0, (hipStream_t)stream>>>(x, out, L, count);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- V2VNet message passing (v2v_kernels.h) ------------------------------------------------------------------------------
int gencomm_v2v_warp_pairs_fwd(const float* x, const double* theta, const int* src_row, float* out, int P, int C, int H, int W, void* stream) {
  GC_CHECK_ARG(x && theta && src_row && out, "null pointer");
  GC_CHECK_ARG(P >= 1 && P <= 65535 && C >= 1 && H >= 1 && W >= 1, "v2v warp pairs: 1..65535 pairs, positive C / H / W");
  GC_CHECK_ARG((long long)C * H * W < (1LL << 31), "v2v warp pairs: one agent's map must stay below 2^31 elements");
  V2vWarpArgs a{x, theta, src_row, out, C, H, W};
  GC_KLOG("v2v_warp_pairs_kernel");
  v2v_warp_pairs_kernel<<<dim3((H * W + 63) / 64, P), 256, 0, (hipStream_t)stream>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// The inference entry (winner == nullptr, train == false) and the training entry share the checks and the launch geometry.
static int v2v_aggregate_enqueue(const float* y, const float* e, const float* h, const double* theta, const int* node_row, const int* pair_off,
                                 float* out, unsigned char* winner, bool train, int n_nodes, int C, int H, int W, int op, int out_mode,
                                 void* stream) {
  GC_CHECK_ARG(y && e && h && theta && node_row && pair_off && out, "null pointer");
  GC_CHECK_ARG(n_nodes >= 1 && n_nodes <= 65535 && C >= 1 && H >= 1 && W >= 1, "v2v aggregate: 1..65535 nodes, positive C / H / W");
  GC_CHECK_ARG(op == 0 || op == 1, "v2v aggregate: op must be 0 (mean) or 1 (max)");
  GC_CHECK_ARG(out_mode == 0 || out_mode == 1, "v2v aggregate: out_mode must be 0 ([h | agg]) or 1 (h + agg)");
  GC_CHECK_ARG((long long)2 * C * H * W < (1LL << 31), "v2v aggregate: one node's [h | agg] map must stay below 2^31 elements");
  const int HW = H * W;
  GC_CHECK_ARG(!train || op == 0 || winner != nullptr, "v2v aggregate: the training entry needs the winner map for op 1 (max)");
  const bool vec = HW % 4 == 0 && (((uintptr_t)y | (uintptr_t)e | (uintptr_t)h | (uintptr_t)out) & 15) == 0 && ((uintptr_t)winner & 3) == 0;
  const int px = vec ? 256 : 64;                                   // pixels per workgroup
  const int gx = (HW + px - 1) / px;
  // channel slices (blockIdx.z) until the launch has about four workgroups per compute unit; a slice keeps at least 16 channels, so the
  // masks a workgroup computes serve at least four channels per thread
  int cpb = (C + 3) / 4 * 4;
  while (cpb >= 32 && (long long)gx * n_nodes * ((C + cpb - 1) / cpb) < 1024) cpb = (cpb / 2 + 3) / 4 * 4;
  const int gz = (C + cpb - 1) / cpb;
  GC_CHECK_ARG(gz <= 65535, "v2v aggregate: too many channels");
  V2vAggArgs a{y, e, h, theta, node_row, pair_off, out, C, H, W, op, out_mode, cpb, winner};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(gx, n_nodes, gz);
  // The mean keeps no winner: the training entry then launches the inference instantiation itself (the same code object, so the same
  // bits by construction). For the max, `out` is a product folded with fmaxf in both instantiations: nothing the compiler could contract.
  if (train && op == 1) {
    GC_KLOG(vec ? "v2v_aggregate_kernel<4, train>" : "v2v_aggregate_kernel<1, train>");
    if (vec) v2v_aggregate_kernel<4, true><<<grid, 256, 0, st>>>(a);
    else v2v_aggregate_kernel<1, true><<<grid, 256, 0, st>>>(a);
  } else if (vec) {
    GC_KLOG("v2v_aggregate_kernel<4>");
    v2v_aggregate_kernel<4, false><<<grid, 256, 0, st>>>(a);
  } else {
    GC_KLOG("v2v_aggregate_kernel<1>");
    v2v_aggregate_kernel<1, false><<<grid, 256, 0, st>>>(a);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_v2v_aggregate_fwd(const float* y, const float* e, const float* h, const double* theta, const int* node_row, const int* pair_off,
                              float* out, int n_nodes, int C, int H, int W, int op, int out_mode, void* stream) {
  return v2v_aggregate_enqueue(y, e, h, theta, node_row, pair_off, out, nullptr, false, n_nodes, C, H, W, op, out_mode, stream);
}

int gencomm_v2v_aggregate_train_fwd(const float* y, const float* e, const float* h, const double* theta, const int* node_row, const int* pair_off,
                                    float* out, unsigned char* winner, int n_nodes, int C, int H, int W, int op, int out_mode, void* stream) {
  return v2v_aggregate_enqueue(y, e, h, theta, node_row, pair_off, out, winner, true, n_nodes, C, H, W, op, out_mode, stream);
}

int gencomm_v2v_aggregate_bwd(const float* dout, const double* theta, const int* node_row, const int* pair_off, const unsigned char* winner,
                              float* dy, float* de, int n_nodes, int C, int H, int W, int op, int out_mode, void* stream) {
  (void)node_row;   // the pass-through gradient of h is a slice of dout: no kernel touches the rows
  GC_CHECK_ARG(dout && theta && pair_off && dy && de, "null pointer");
  GC_CHECK_ARG(n_nodes >= 1 && n_nodes <= 65535 && C >= 1 && H >= 1 && W >= 1, "v2v aggregate backward: 1..65535 nodes, positive C / H / W");
  GC_CHECK_ARG(op == 0 || op == 1, "v2v aggregate backward: op must be 0 (mean) or 1 (max)");
  GC_CHECK_ARG(out_mode == 0 || out_mode == 1, "v2v aggregate backward: out_mode must be 0 ([h | agg]) or 1 (h + agg)");
  GC_CHECK_ARG(op == 0 || winner != nullptr, "v2v aggregate backward: op 1 (max) needs the winner map of gencomm_v2v_aggregate_train_fwd");
  GC_CHECK_ARG((long long)2 * C * H * W < (1LL << 31), "v2v aggregate backward: one node's [h | agg] map must stay below 2^31 elements");
  const int HW = H * W;
  const float* dagg = out_mode == 0 ? dout + (size_t)C * HW : dout;
  const size_t node_stride = (size_t)(out_mode == 0 ? 2 * C : C) * HW;
  const bool vec = HW % 4 == 0 && (((uintptr_t)dagg | (uintptr_t)dy | (uintptr_t)de) & 15) == 0 && ((uintptr_t)winner & 3) == 0;
  const int px = vec ? 256 : 64;
  const int gx = (HW + px - 1) / px;
  int cpb = (C + 3) / 4 * 4;                                       // the forward's channel slices
  while (cpb >= 32 && (long long)gx * n_nodes * ((C + cpb - 1) / cpb) < 1024) cpb = (cpb / 2 + 3) / 4 * 4;
  const int gz = (C + cpb - 1) / cpb;
  GC_CHECK_ARG(gz <= 65535, "v2v aggregate backward: too many channels");
  V2vAggBwdArgs a{dagg, node_stride, theta, pair_off, winner, dy, de, C, H, W, op, cpb};
  hipStream_t st = (hipStream_t)stream;
  GC_KLOG(vec ? "v2v_aggregate_bwd_kernel<4>" : "v2v_aggregate_bwd_kernel<1>");
  if (vec) v2v_aggregate_bwd_kernel<4><<<dim3(gx, n_nodes, gz), 256, 0, st>>>(a);
  else v2v_aggregate_bwd_kernel<1><<<dim3(gx, n_nodes, gz), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

long long gencomm_v2v_warp_pairs_bwd_scratch_floats(int P) {
  if (P < 1 || P > 65535) { fail(GC_ERR_ARG, "v2v warp pairs backward: 1..65535 pairs"); return -1; }
  return (long long)P + 64;
}

int gencomm_v2v_warp_pairs_bwd(const float* dwarped, const double* theta, const int* src_row, const int* row_pair_off, const int* row_pairs,
                               float* dx, float* scratch, int P, int rows, int C, int H, int W, int accumulate, void* stream) {
  GC_CHECK_ARG(dwarped && theta && src_row && row_pair_off && row_pairs && dx && scratch, "null pointer");
  GC_CHECK_ARG(P >= 1 && P <= 65535 && rows >= 1 && rows <= 65535 && C >= 1 && H >= 1 && W >= 1,
               "v2v warp pairs backward: 1..65535 pairs and rows, positive C / H / W");
  GC_CHECK_ARG(accumulate == 0 || accumulate == 1, "v2v warp pairs backward: accumulate must be 0 or 1");
  GC_CHECK_ARG((long long)C * H * W < (1LL << 31), "v2v warp pairs backward: one agent's map must stay below 2^31 elements");
  const int HW = H * W;
  const int gx = (HW + 63) / 64;
  // channel slices (blockIdx.z) until the launch has about 1024 workgroups; a slice keeps at least 16 channels, so the match lists a
  // workgroup builds serve at least four channels per thread
  int cpb = (C + 3) / 4 * 4;
  while (cpb >= 32 && (long long)gx * rows * ((C + cpb - 1) / cpb) < 1024) cpb = (cpb / 2 + 3) / 4 * 4;
  const int gz = (C + cpb - 1) / cpb;
  GC_CHECK_ARG(gz <= 65535, "v2v warp pairs backward: too many channels");
  V2vWarpBwdArgs a{dwarped, theta, src_row, row_pair_off, row_pairs, dx, reinterpret_cast<int*>(scratch), P, C, H, W, accumulate, cpb};
  hipStream_t st = (hipStream_t)stream;
  GC_KLOG("v2v_warp_bwd_gather_kernel");
  v2v_warp_bwd_plan_kernel<<<(P + 63) / 64, 64, 0, st>>>(a);
  v2v_warp_bwd_gather_kernel<<<dim3(gx, rows, gz), 256, 0, st>>>(a);
  v2v_warp_bwd_scatter_kernel<<<dim3(gx, P), 256, 0, st>>>(a);   // a workgroup whose pair was gathered leaves at once
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_gru_gate_fwd(const float* g, float* h, int n, int C, int HW, void* stream) {
  GC_CHECK_ARG(g && h, "null pointer");
  GC_CHECK_ARG(n >= 1 && n <= 65535 && C >= 1 && HW >= 1, "gru gate: 1..65535 rows, positive C / HW");
  const long long count = (long long)C * HW;
  GC_CHECK_ARG(count < (1LL << 31), "gru gate: one row must stay below 2^31 elements");
  hipStream_t st = (hipStream_t)stream;
  if (count % 4 == 0 && (((uintptr_t)g | (uintptr_t)h) & 15) == 0) {
    GC_KLOG("gru_gate_kernel<4>");
    gru_gate_kernel<4><<<dim3((unsigned)((count / 4 + 255) / 256), n), 256, 0, st>>>(g, h, count);
  } else {
    GC_KLOG("gru_gate_kernel<1>");
    gru_gate_kernel<1><<<dim3((unsigned)((count + 255) / 256), n), 256, 0, st>>>(g, h, count);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_gru_gate_bwd(const float* g, const float* dh, float* dg, int n, int C, int HW, void* stream) {
  GC_CHECK_ARG(g && dh && dg, "null pointer");
  GC_CHECK_ARG(n >= 1 && n <= 65535 && C >= 1 && HW >= 1, "gru gate backward: 1..65535 rows, positive C / HW");
  const long long count = (long long)C * HW;
  GC_CHECK_ARG(count < (1LL << 31), "gru gate backward: one row must stay below 2^31 elements");
  hipStream_t st = (hipStream_t)stream;
  if (count % 4 == 0 && (((uintptr_t)g | (uintptr_t)dh | (uintptr_t)dg) & 15) == 0) {
    GC_KLOG("gru_gate_bwd_kernel<4>");
    gru_gate_bwd_kernel<4><<<dim3((unsigned)((count / 4 + 255) / 256), n), 256, 0, st>>>(g, dh, dg, count);
  } else {
    GC_KLOG("gru_gate_bwd_kernel<1>");
    gru_gate_bwd_kernel<1><<<dim3((unsigned)((count + 255) / 256), n), 256, 0, st>>>(g, dh, dg, count);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- V2X-ViT backward building blocks (v2xvit_kernels.h) ----------------------------------------------------------------
int gencomm_warp_affine_bwd(const double* theta, const float* dout, float* dx, int n, int C, int H, int W, void* stream) {
  GC_CHECK_ARG(theta && dout && dx && n >= 1 && n <= 65535 && C >= 1 && H >= 1 && W >= 1, "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  GC_HIP(hipMemsetAsync(dx, 0, (size_t)n * C * H * W * sizeof(float), st));
  WarpArgs a{nullptr, theta, dx, C, H, W};
  warp_affine_bwd_kernel<<<dim3((H * W + 255) / 256, n), 256, 0, st>>>(a, dout);
  GC_HIP(hipGetLastError());
  return GC_OK;
}
int gencomm_hgt_attn_bwd(const float* qkv, const int* scene_off, const float* dout, float* dqkv, int B, int heads, int dim_head, int HW, void* stream) {
  GC_CHECK_ARG(qkv && scene_off && dout && dqkv && B >= 1 && B <= 65535 && heads >= 1 && heads <= 65535 && HW >= 1, "bad arguments");
  HgtBwdArgs a{qkv, scene_off, dout, dqkv, heads, HW, 1.0f / sqrtf((float)dim_head)};
  const dim3 grid((HW + 255) / 256, heads, B);
  hipStream_t st = (hipStream_t)stream;
  if (dim_head == 32) hgt_attn_bwd_kernel<32><<<grid, 256, 0, st>>>(a);
  else if (dim_head == 64) hgt_attn_bwd_kernel<64><<<grid, 256, 0, st>>>(a);
  else if (dim_head == 16) hgt_attn_bwd_kernel<16><<<grid, 256, 0, st>>>(a);
  else if (dim_head == 8) hgt_attn_bwd_kernel<8><<<grid, 256, 0, st>>>(a);
  else return fail(GC_ERR_ARG, "hgt attention: dim_head must be 8, 16, 32 or 64");
  GC_HIP(hipGetLastError());
  return GC_OK;
}
long long gencomm_win_attn_bwd_scratch_floats(int n, int heads, int window, int H, int W) {
  if (n < 1 || heads < 1 || window < 1 || H < window || W < window || H % window || W % window) { fail(GC_ERR_ARG, "bad arguments"); return -1; }
  const long long T = (long long)window * window, nwin = (long long)(H / window) * (W / window);
  return (long long)n * heads * nwin * 2 * T * T;
}
// dqkv [n][3 inner][H][W] is overwritten; dpos [(2 window - 1)^2] is ACCUMULATED (+=); `out` = the forward's output
int gencomm_win_attn_bwd(const float* qkv, const float* pos_embedding, const float* out, const float* dout, float* dqkv, float* dpos,
                         float* scratch, int n, int heads, int dim_head, int window, int H, int W, void* stream) {
  GC_CHECK_ARG(qkv && pos_embedding && out && dout && dqkv && dpos && scratch && n >= 1 && n <= 65535 && heads >= 1 && heads <= 65535, "bad arguments");
  GC_CHECK_ARG(H >= window && W >= window && H % window == 0 && W % window == 0, "H and W must be multiples of the window size");
  WinBwdArgs a{qkv, pos_embedding, out, dout, dqkv, dpos, scratch, heads, H, W, 1.0f / sqrtf((float)dim_head)};
  hipStream_t st = (hipStream_t)stream;
  if (window == 4 && dim_head == 16) return win_attn_bwd_launch<16, 4>(a, n, st);
  if (window == 8 && dim_head == 32) return win_attn_bwd_launch<32, 8>(a, n, st);
  if (window == 16 && dim_head == 64) return win_attn_bwd_launch<64, 16>(a, n, st);
  if (window == 4 && dim_head == 32) return win_attn_bwd_launch<32, 4>(a, n, st);
  if (window == 8 && dim_head == 16) return win_attn_bwd_launch<16, 8>(a, n, st);
  if (window == 8 && dim_head == 64) return win_attn_bwd_launch<64, 8>(a, n, st);
  if (window == 16 && dim_head == 32) return win_attn_bwd_launch<32, 16>(a, n, st);
  return fail(GC_ERR_ARG, "window attention: supported (window, dim_head) pairs are (4,16) (4,32) (8,16) (8,32) (8,64) (16,32) (16,64)");
}

// radix-3 split attention over three branch maps [n][C][HW] (+ residual): gap -> fc1 -> LayerNorm -> ReLU -> fc2 -> softmax over the
// branches -> weighted sum (sub_modules/split_attn.py:31-62 with radix 3); scratch >= 4 n C floats
int gencomm_split3_attn_fwd(const float* a, const float* b, const float* c, const float* fc1_w, const float* ln_w, const float* ln_b,
                            const float* fc2_w, const float* residual, float* out, float* scratch, int n, int C, int HW, void* stream) {
  GC_CHECK_ARG(a && b && c && fc1_w && ln_w && ln_b && fc2_w && out && scratch, "null pointer");
  GC_CHECK_ARG(n >= 1 && n <= 65535 && C >= 1 && C <= 256 && HW >= 1, "split attention: 1 <= C <= 256");
  hipStream_t st = (hipStream_t)stream;
  float* gap = scratch;
  float* gate = scratch + (size_t)n * C;
  split3_gap_kernel<<<dim3(C, n), 256, 0, st>>>(a, b, c, gap, C, HW);
  Split3GateArgs ga{gap, fc1_w, ln_w, ln_b, fc2_w, gate, C};
  split3_gate_kernel<<<n, 256, 0, st>>>(ga);
  split3_apply_kernel<<<dim3((HW + 255) / 256, C, n), 256, 0, st>>>(a, b, c, gate, residual, out, C, HW);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- sparse 3-D convolution (SECOND encoder) -------------------------------------------------------------------------
static int sp_grid(SpGrid& g, int B, const int* dims3, const char* what) {
  GC_CHECK_ARG(dims3 != nullptr && B >= 1 && dims3[0] >= 1 && dims3[1] >= 1 && dims3[2] >= 1, what);
  g.B = B; g.D = dims3[0]; g.H = dims3[1]; g.W = dims3[2];
  return GC_OK;
}
static int sp_geom(SpConvGeom& g, int B, const int* in_dims3, const int* kernel3, const int* stride3, const int* pad3) {
  if (int rc = sp_grid(g.in, B, in_dims3, "bad input grid")) return rc;
  GC_CHECK_ARG(kernel3 && stride3 && pad3, "null pointer");
  g.out.B = B;
  int od[3];
  for (int j = 0; j < 3; ++j) {
    GC_CHECK_ARG(kernel3[j] >= 1 && kernel3[j] <= 7 && stride3[j] >= 1 && pad3[j] >= 0, "bad kernel / stride / padding");
    g.k[j] = kernel3[j]; g.stride[j] = stride3[j]; g.pad[j] = pad3[j];
    const int num = in_dims3[j] + 2 * pad3[j] - kernel3[j];
    GC_CHECK_ARG(num >= 0, "kernel larger than the padded grid");
    od[j] = num / stride3[j] + 1;
  }
  g.out.D = od[0]; g.out.H = od[1]; g.out.W = od[2];
  return GC_OK;
}

int gencomm_sp_out_dims(const int* in_dims3, const int* kernel3, const int* stride3, const int* pad3, int* out_dims3) {
  SpConvGeom g{};
  if (int rc = sp_geom(g, 1, in_dims3, kernel3, stride3, pad3)) return rc;
  GC_CHECK_ARG(out_dims3 != nullptr, "null pointer");
  out_dims3[0] = g.out.D; out_dims3[1] = g.out.H; out_dims3[2] = g.out.W;
  return GC_OK;
}

long long gencomm_sp_index_workspace_bytes(int n) {
  if (n < 0) { fail(GC_ERR_ARG, "n must be non-negative"); return -1; }
  return (long long)sp_sort_ws(n).total;
}
int gencomm_sp_index_fwd(const int* coords_bzyx, int n, int B, const int* dims3, long long* keys, int* perm, void* workspace, long long workspace_bytes,
                         void* stream) {
  SpGrid g{};
  if (int rc = sp_grid(g, B, dims3, "bad grid")) return rc;
  GC_CHECK_ARG(n >= 0, "n must be non-negative");
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(coords_bzyx && keys && perm && workspace, "null pointer");
  const SpSortWs w = sp_sort_ws(n);
  if ((long long)w.total > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_sp_index_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  char* wsp = (char*)workspace;
  long long* key = reinterpret_cast<long long*>(wsp + w.key);
  int* val = reinterpret_cast<int*>(wsp + w.val);
  sp_key_kernel<<<(n + 255) / 256, 256, 0, st>>>(coords_bzyx, n, g, key, val);
  size_t tb = w.temp_bytes;
  GC_HIP(rocprim::radix_sort_pairs(wsp + w.temp, tb, key, keys, val, perm, (size_t)n, 0, 63, st));   // keys are non-negative; out-of-grid rows carry kSpNoKey
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_sp_rules_fwd(const long long* out_keys, int n_out, const long long* in_keys, int n_in, int B, const int* in_dims3, const int* kernel3,
                         const int* stride3, const int* pad3, int* nbr, void* stream) {
  SpConvGeom g{};
  if (int rc = sp_geom(g, B, in_dims3, kernel3, stride3, pad3)) return rc;
  GC_CHECK_ARG(n_out >= 0 && n_in >= 0, "negative count");
  if (n_out == 0) return GC_OK;
  GC_CHECK_ARG(out_keys && nbr && (n_in == 0 || in_keys), "null pointer");
  const int K = g.k[0] * g.k[1] * g.k[2];
  sp_rules_kernel<<<dim3((n_out + 255) / 256, K), 256, 0, (hipStream_t)stream>>>(out_keys, n_out, in_keys, n_in, g, nbr);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

static long long sp_slots(const int* kernel3, const int* stride3) {
  long long s = 1;
  for (int j = 0; j < 3; ++j) s *= (kernel3[j] + stride3[j] - 1) / stride3[j];
  return s;
}
long long gencomm_sp_sites_capacity(int n_in, const int* kernel3, const int* stride3) {
  if (n_in < 0 || !kernel3 || !stride3 || stride3[0] < 1 || stride3[1] < 1 || stride3[2] < 1) { fail(GC_ERR_ARG, "bad arguments"); return -1; }
  return (long long)n_in * sp_slots(kernel3, stride3);
}
long long gencomm_sp_sites_workspace_bytes(int n_in, const int* kernel3, const int* stride3) {
  const long long cap = gencomm_sp_sites_capacity(n_in, kernel3, stride3);
  if (cap < 0) return -1;
  return (long long)sp_sites_ws(cap).total;
}
// out_keys must hold gencomm_sp_sites_capacity entries (the upper bound); *n_out (device) receives the number of output sites
int gencomm_sp_sites_fwd(const long long* in_keys, int n_in, int B, const int* in_dims3, const int* kernel3, const int* stride3, const int* pad3,
                         long long* out_keys, int* n_out, void* workspace, long long workspace_bytes, void* stream) {
  SpConvGeom g{};
  if (int rc = sp_geom(g, B, in_dims3, kernel3, stride3, pad3)) return rc;
  GC_CHECK_ARG(n_in >= 0 && n_out != nullptr, "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (n_in == 0) {
    GC_HIP(hipMemsetAsync(n_out, 0, sizeof(int), st));
    return GC_OK;
  }
  GC_CHECK_ARG(in_keys && out_keys && workspace, "null pointer");
  SpSlots sl{};
  for (int j = 0; j < 3; ++j) sl.n[j] = sp_slot_count(g, j);
  const int slots = sl.n[0] * sl.n[1] * sl.n[2];
  const long long nc = (long long)n_in * slots;
  GC_CHECK_ARG(nc < (1LL << 31), "too many candidate sites");
  const SpSitesWs w = sp_sites_ws(nc);
  if ((long long)w.total > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_sp_sites_workspace_bytes)");
  const long long nokey = (long long)B * g.out.D * g.out.H * g.out.W;   // one past the largest key
  int bits = 1;
  while ((1LL << bits) <= nokey) ++bits;                                // radix passes over the bits in use only
  char* wsp = (char*)workspace;
  long long* cand = reinterpret_cast<long long*>(wsp + w.cand);
  long long* sorted = reinterpret_cast<long long*>(wsp + w.sorted);
  sp_candidates_kernel<<<dim3((n_in + 255) / 256, slots), 256, 0, st>>>(in_keys, n_in, g, sl, nokey, cand);
  size_t tb = w.temp_bytes;
  GC_HIP(rocprim::radix_sort_keys(wsp + w.temp, tb, cand, sorted, (size_t)nc, 0, bits, st));
  tb = w.temp_bytes;
  GC_HIP(rocprim::unique(wsp + w.temp, tb, sorted, out_keys, n_out, (size_t)nc, rocprim::equal_to<long long>(), st));
  sp_fix_count_kernel<<<1, 64, 0, st>>>(out_keys, nokey, n_out);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

long long gencomm_sp_prepared_floats(int K, int Cin, int Cout) {
  if (K < 1 || Cin < 1 || Cin > 64 || Cout < 1) { fail(GC_ERR_ARG, "sparse conv: 1 <= Cin <= 64"); return -1; }
  return (long long)K * sp_cin_padded(Cin) * (long long)align_up((size_t)Cout, 32);
}
int gencomm_sp_prepare(const float* w, float* prepared, int K, int Cin, int Cout, int layout, void* stream) {
  GC_CHECK_ARG(w && prepared && layout >= 0 && layout <= 3, "bad arguments");
  const long long total = gencomm_sp_prepared_floats(K, Cin, Cout);
  if (total < 0) return GC_ERR_ARG;
  sp_prep_w_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(w, prepared, K, Cin, Cout, sp_cin_padded(Cin), (int)align_up((size_t)Cout, 32), layout);
  GC_HIP(hipGetLastError());
  return GC_OK;
}
int gencomm_sp_conv_fwd(const float* x, const int* nbr, const float* prepared, const float* scale, const float* shift, float* y, int n_out, int K, int Cin,
                        int Cout, int relu, void* stream) {
  GC_CHECK_ARG(n_out >= 0 && K >= 1 && Cin >= 1 && Cin <= 64 && Cout >= 1, "bad arguments");
  if (n_out == 0) return GC_OK;
  GC_CHECK_ARG(x && nbr && prepared && scale && shift && y, "null pointer");
  SpConvArgs a{x, nbr, prepared, scale, shift, y, n_out, K, Cin, Cout, (int)align_up((size_t)Cout, 32), relu};
  return sp_conv_enqueue(a, (hipStream_t)stream);
}
// ---- training of the sparse layers -------------------------------------------------------------------------------------
int gencomm_bnrow_train_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var, float* y, float* save,
                            double* scratch, float momentum, float eps, int relu, int n, int C, void* stream) {
  GC_CHECK_ARG(x && gamma && beta && y && save && scratch && n >= 1 && (C == 16 || C == 32 || C == 64 || C == 128), "BatchNorm over rows: C in {16, 32, 64, 128}");
  GC_CHECK_ARG((running_mean == nullptr) == (running_var == nullptr), "running statistics: both or neither");
  hipStream_t st = (hipStream_t)stream;
  GC_HIP(hipMemsetAsync(scratch, 0, (size_t)C * 2 * sizeof(double), st));
  const int slots = 256 / C;
  bnrow_stats_kernel<<<std::max(1, std::min((n + slots * 16 - 1) / (slots * 16), 512)), 256, 0, st>>>(x, scratch, n, C);
  bn2d_finish_rows_kernel<<<(C + 63) / 64, 64, 0, st>>>(x, scratch, save, running_mean, running_var, momentum, eps, (long long)n, C);
  const long long total = (long long)n * C;
  bnrow_apply_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(x, save, gamma, beta, y, total, C, relu);
  GC_HIP(hipGetLastError());
  return GC_OK;
}
int gencomm_bnrow_train_bwd(const float* x, const float* y, const float* dy, const float* save, const float* gamma, float* dx, float* dgamma,
                            float* dbeta, double* scratch, int relu, int n, int C, void* stream) {
  GC_CHECK_ARG(x && y && dy && save && gamma && dx && scratch && n >= 1 && (C == 16 || C == 32 || C == 64 || C == 128), "BatchNorm over rows: C in {16, 32, 64, 128}");
  hipStream_t st = (hipStream_t)stream;
  GC_HIP(hipMemsetAsync(scratch, 0, (size_t)C * 2 * sizeof(double), st));
  const int slots = 256 / C;
  bnrow_bwd_reduce_kernel<<<std::max(1, std::min((n + slots * 16 - 1) / (slots * 16), 512)), 256, 0, st>>>(x, y, dy, save, scratch, n, C, relu);
  const long long total = (long long)n * C;
  bnrow_bwd_apply_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(x, y, dy, save, gamma, scratch, dx, dgamma, dbeta, total, (long long)n, C, relu);
  GC_HIP(hipGetLastError());
  return GC_OK;
}
int gencomm_sp_rules_inv_fwd(const long long* in_keys, int n_in, const long long* out_keys, int n_out, int B, const int* in_dims3, const int* kernel3,
                             const int* stride3, const int* pad3, int* inv, void* stream) {
  SpConvGeom g{};
  if (int rc = sp_geom(g, B, in_dims3, kernel3, stride3, pad3)) return rc;
  GC_CHECK_ARG(n_out >= 0 && n_in >= 0, "negative count");
  if (n_in == 0) return GC_OK;
  GC_CHECK_ARG(in_keys && inv && (n_out == 0 || out_keys), "null pointer");
  const int K = g.k[0] * g.k[1] * g.k[2];
  sp_rules_inv_kernel<<<dim3((n_in + 255) / 256, K), 256, 0, (hipStream_t)stream>>>(in_keys, n_in, out_keys, n_out, g, inv);
  GC_HIP(hipGetLastError());
  return GC_OK;
}
// dw: raw layout 0 [Cout][K][Cin], ACCUMULATED (+=)
int gencomm_sp_wgrad(const float* x, const float* dy, const int* nbr, float* dw, int n_out, int K, int Cin, int Cout, void* stream) {
  GC_CHECK_ARG(n_out >= 0 && K >= 1 && K <= 65535 && Cin >= 1 && Cin <= 64 && Cout >= 1 && Cout <= 64, "sparse wgrad: at most 64 channels on either side");
  if (n_out == 0) return GC_OK;
  GC_CHECK_ARG(x && dy && nbr && dw, "null pointer");
  SpWgradArgs a{x, dy, nbr, dw, n_out, K, Cin, Cout, 0};
  a.rows_per_block = 1024;
  while (a.rows_per_block > 64 && (long long)((n_out + a.rows_per_block - 1) / a.rows_per_block) * K < 512) a.rows_per_block >>= 1;
  sp_wgrad_kernel<<<dim3((n_out + a.rows_per_block - 1) / a.rows_per_block, K), 256, 0, (hipStream_t)stream>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_sp_dense_fwd(const float* feat, const long long* keys, int n, int C, int B, const int* dims3, float* out, void* stream) {
  SpGrid g{};
  if (int rc = sp_grid(g, B, dims3, "bad grid")) return rc;
  GC_CHECK_ARG(n >= 0 && C >= 1 && out, "bad arguments");
  hipStream_t st = (hipStream_t)stream;
  GC_HIP(hipMemsetAsync(out, 0, (size_t)B * C * g.D * g.H * g.W * sizeof(float), st));
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(feat && keys, "null pointer");
  const long long total = (long long)n * C;
  sp_dense_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(feat, keys, n, C, g, out);
  GC_HIP(hipGetLastError());
  return GC_OK;
}
int gencomm_mean_vfe_fwd(const float* voxels, const int* num_points, const int* perm, float* out, int n, int max_points, int nfeat, void* stream) {
  GC_CHECK_ARG(n >= 0 && max_points >= 1 && nfeat >= 1, "bad arguments");
  if (n == 0) return GC_OK;
  GC_CHECK_ARG(voxels && num_points && out, "null pointer");
  const long long total = (long long)n * nfeat;
  mean_vfe_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(voxels, num_points, perm, out, n, max_points, nfeat);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_head_loss(const float* cls, const float* reg, const float* dir, const float* pos, const float* neg, const float* tgt, float* gcls,
                      float* greg, float* gdir, double* sums, int B, int A, int H, int W, int num_bins, const double* anchor_yaw, double dir_offset,
                      float pos_cls_weight, float gamma, float alpha, float cls_weight, float sigma, float reg_weight, float dir_weight,
                      int batch_size, void* stream) {
  GC_CHECK_ARG(cls && reg && pos && neg && tgt && gcls && greg && sums, "null pointer");
  GC_CHECK_ARG(B >= 1 && A >= 1 && A <= kLossMaxAnchors && H >= 1 && W >= 1 && batch_size >= 1 && sigma > 0.f, "bad dims");
  GC_CHECK_ARG((long long)H * W * A < (1LL << 30) && B <= 65535, "map too large");
  GC_CHECK_ARG(dir == nullptr || (gdir && anchor_yaw && num_bins >= 1 && num_bins <= A), "direction term: gdir, anchor_yaw [A] and 1 <= num_bins <= A");
  HeadLossArgs a{};
  a.cls = cls; a.reg = reg; a.dir = dir; a.pos = pos; a.neg = neg; a.tgt = tgt;
  a.gcls = gcls; a.greg = greg; a.gdir = gdir; a.sums = sums;
  a.B = B; a.A = A; a.HW = H * W; a.has_dir = dir != nullptr; a.num_bins = num_bins;
  a.pos_cls_weight = pos_cls_weight; a.gamma = gamma; a.alpha = alpha; a.cls_weight = cls_weight; a.sigma = sigma; a.reg_weight = reg_weight;
  a.dir_weight = dir_weight; a.inv_bs = 1.0f / (float)batch_size; a.dir_offset = dir_offset;
  for (int i = 0; i < kLossMaxAnchors; ++i) a.anchor_yaw[i] = (dir != nullptr && i < A) ? anchor_yaw[i] : 0.0;
  return head_loss_enqueue(a, (hipStream_t)stream);
}

int gencomm_head_loss_mc(const float* cls, const float* reg, const void* labels, const void* targets, int dtype, unsigned* count, float* gcls,
                         float* greg, double* sums, int B, int S, int K, int H, int W, double cls_weight, double reg_weight, void* stream) {
  GC_CHECK_ARG(cls && reg && labels && targets && count && gcls && greg && sums, "null pointer");
  GC_CHECK_ARG(dtype == 0 || dtype == 1, "bad dtype flag (0: float32, 1: float64 labels / targets)");
  GC_CHECK_ARG(B >= 1 && S >= 1 && K >= 1 && K <= kLossMcMaxClasses && H >= 1 && W >= 1, "bad dims (B, S, H, W >= 1, 1 <= K <= 8)");
  GC_CHECK_ARG((long long)H * W * S * 7 < (1LL << 31) && (long long)H * W * S * K < (1LL << 31) && B <= 65535, "map too large");
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == 1) {
    HeadLossMcArgs<double> a{cls, reg, (const double*)labels, (const double*)targets, count, gcls, greg, sums, B, S, K, H * W, cls_weight, reg_weight};
    return head_loss_mc_enqueue(a, count, st);
  }
  HeadLossMcArgs<float> a{cls, reg, (const float*)labels, (const float*)targets, count, gcls, greg, sums, B, S, K, H * W, cls_weight, reg_weight};
  return head_loss_mc_enqueue(a, count, st);
}

// ---- the terms the HEAL and MPDA criteria add to the head loss (criteria_kernels.h)
int gencomm_pyramid_occ_loss(const float* pos, const float* neg, const float* const* occ, float* const* grad, const int* relative_downsample,
                             const float* weight, int levels, int B, int H, int W, int A, float pos_cls_weight, float gamma, float alpha,
                             double* sums, void* stream) {
  GC_CHECK_ARG(pos && neg && occ && grad && relative_downsample && weight && sums, "null pointer");
  GC_CHECK_ARG(levels >= 1 && levels <= kOccMaxLevels, "1 <= levels <= 4");
  GC_CHECK_ARG(B >= 1 && B <= 65535 && H >= 1 && W >= 1 && A >= 2 && (long long)H * W < (1LL << 24), "bad dims (A >= 2, H W < 2^24, B <= 65535)");
  GC_CHECK_ARG(gamma >= 0.f, "gamma must not be negative");
  OccLossArgs a{};
  a.pos = pos; a.neg = neg; a.sums = sums; a.part = sums + 5;
  a.B = B; a.H = H; a.W = W; a.A = A; a.levels = levels;
  a.pos_cls_weight = pos_cls_weight; a.alpha = alpha; a.gamma = gamma; a.inv_bs = 1.0f / (float)B;
  for (int i = 0; i < levels; ++i) {
    const int k = relative_downsample[i];
    GC_CHECK_ARG(k >= 1 && k <= H && k <= W, "relative_downsample must be in 1 .. min(H, W)");
    GC_CHECK_ARG(occ[i] && grad[i], "null level pointer");
    a.occ[i] = occ[i]; a.grad[i] = grad[i]; a.k[i] = k; a.Hl[i] = H / k; a.Wl[i] = W / k; a.weight[i] = weight[i];
    a.cell_start[i + 1] = a.cell_start[i] + a.Hl[i] * a.Wl[i];
  }
  return occ_loss_enqueue(a, (hipStream_t)stream);
}

int gencomm_domain_bce_loss(const float* x, const int* source_index, int num_sources, float* grad, double* sums, int N, int C, int H, int W,
                            void* stream) {
  GC_CHECK_ARG(x && grad && sums && (source_index || num_sources == 0), "null pointer");
  GC_CHECK_ARG(N >= 1 && N <= kBceMaxAgents && C >= 1 && H >= 1 && W >= 1 && (long long)C * H * W < (1LL << 30), "bad dims (N <= 1024, C H W < 2^30)");
  GC_CHECK_ARG(num_sources >= 0 && num_sources <= N, "bad num_sources");
  DomainBceArgs a{};
  a.x = x; a.grad = grad; a.sums = sums; a.N = N; a.CHW = C * H * W;
  a.blocks = std::min((a.CHW + 255) / 256, kBceBlocksPerAgent);
  a.inv_numel = 1.0f / ((float)N * (float)a.CHW);
  for (int i = 0; i < num_sources; ++i) {
    GC_CHECK_ARG(source_index[i] >= 0 && source_index[i] < N, "source index outside [0, N)");
    a.source[source_index[i] >> 6] |= 1ull << (source_index[i] & 63);
  }
  return domain_bce_enqueue(a, (hipStream_t)stream);
}

// ---- anchor target assignment (generate_label / generate_label_v2xreal) ---------------------------------------------
long long gencomm_target_assign_workspace_bytes(int B, int nc, int max_num) {
  if (B < 1 || B > 65535 || nc < 1 || nc > kTargetMaxClasses || max_num < 1 || max_num > kTargetMaxBoxes) {
    fail(GC_ERR_ARG, "bad B / nc / max_num (1 <= B <= 65535, 1 <= nc <= 8, 1 <= max_num <= 256)");
    return -1;
  }
  return target_workspace_bytes(B, nc, max_num);
}

int gencomm_target_standup_fwd(const double* anchors, int n_anchors, int hwl, float* out, void* stream) {
  GC_CHECK_ARG(anchors && out, "null pointer");
  GC_CHECK_ARG(n_anchors >= 1 && (hwl == 0 || hwl == 1), "bad n_anchors / hwl");
  target_standup_kernel<<<(unsigned)((n_anchors + 255) / 256), 256, 0, (hipStream_t)stream>>>(anchors, n_anchors, hwl, (float4*)out);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_target_assign_fwd(const void* boxes, int box_dtype, int box_width, const void* mask, int mask_dtype, const double* const* anchors,
                              const float* const* standup, const double* pos_threshold, const double* neg_threshold, int B, int nc, int max_num,
                              int n_anchors, int R, int multiclass, void* pos, void* neg, void* targets, int out_dtype, void* workspace,
                              long long workspace_bytes, void* stream) {
  GC_CHECK_ARG(boxes && mask && anchors && standup && pos_threshold && neg_threshold && pos && neg && targets && workspace, "null pointer");
  GC_CHECK_ARG((box_dtype == 0 || box_dtype == 1) && (out_dtype == 0 || out_dtype == 1) && mask_dtype >= 0 && mask_dtype <= 4,
               "bad dtype flag (boxes / outputs 0: float32, 1: float64; mask 0: float32, 1: float64, 2: int32, 3: int64, 4: uint8 / bool)");
  GC_CHECK_ARG(box_width == 7 || box_width == 8, "box rows are 7 or 8 wide");
  GC_CHECK_ARG(multiclass == 0 || (multiclass == 1 && box_width == 8), "the multi-class layout needs the class id in column 7");
  GC_CHECK_ARG(multiclass == 1 || nc == 1, "the single-class layout has nc = 1");
  const long long need = gencomm_target_assign_workspace_bytes(B, nc, max_num);
  if (need < 0) return GC_ERR_ARG;
  if (need > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_target_assign_workspace_bytes)");
  GC_CHECK_ARG(R >= 1 && n_anchors >= R && n_anchors % R == 0 && (long long)n_anchors * nc * 7 < (1LL << 31), "bad n_anchors / R");
  TargetArgs a{};
  a.boxes = boxes; a.mask = mask; a.pos = pos; a.neg = neg; a.targets = targets;
  a.B = B; a.nc = nc; a.max_num = max_num; a.n = n_anchors; a.R = R; a.width = box_width; a.box_f64 = box_dtype; a.mask_dtype = mask_dtype;
  a.multiclass = multiclass;
  for (int k = 0; k < nc; ++k) {
    GC_CHECK_ARG(anchors[k] && standup[k], "null anchor pointer");
    a.anchors[k] = anchors[k]; a.standup[k] = (const float4*)standup[k];
    a.pos_thr[k] = (float)pos_threshold[k]; a.neg_thr[k] = (float)neg_threshold[k];
  }
  return target_assign_enqueue(a, workspace, out_dtype, (hipStream_t)stream);
}

// ---- Lift-Splat-Shoot camera encoder ---------------------------------------------------------------------------------
static int lss_geom(LssGeom& g, int B, int N, int D, int fH, int fW, int C, const float* lo3, const float* dx3, const int* nx3) {
  GC_CHECK_ARG(lo3 && dx3 && nx3, "null pointer");
  GC_CHECK_ARG(B >= 1 && N >= 1 && D >= 1 && fH >= 1 && fW >= 1 && C >= 1, "bad B / N / D / fH / fW / C");
  GC_CHECK_ARG(nx3[0] >= 1 && nx3[1] >= 1 && nx3[2] >= 1 && B <= 65535 && nx3[1] <= 65535 && (long long)B * nx3[2] <= 65535, "bad grid");
  GC_CHECK_ARG((long long)B * nx3[0] * nx3[1] * nx3[2] < (1LL << 31) - 1, "grid has too many cells for 32-bit ranks");
  GC_CHECK_ARG((long long)B * N * D * fH * fW < (1LL << 31), "too many frustum points");
  GC_CHECK_ARG((long long)B * N * fH * fW * C < (1LL << 40), "feature map too large");
  for (int j = 0; j < 3; ++j) {
    GC_CHECK_ARG(dx3[j] > 0.f, "cell size must be positive");
    g.lo[j] = lo3[j];
    g.dx[j] = dx3[j];
  }
  g.nx = nx3[0]; g.ny = nx3[1]; g.nz = nx3[2];
  g.B = B; g.N = N; g.D = D; g.fH = fH; g.fW = fW; g.C = C;
  return GC_OK;
}
static int lss_sort_bits(const LssGeom& g) {
  const unsigned long long ncells = (unsigned long long)g.B * g.nx * g.ny * g.nz;   // the sentinel key of out-of-grid points
  int bits = 1;
  while ((1ULL << bits) <= ncells) ++bits;
  return bits;
}

long long gencomm_lss_workspace_bytes(int B, int N, int D, int fH, int fW, int C, const int* nx3) {
  const float lo[3] = {0.f, 0.f, 0.f}, dx[3] = {1.f, 1.f, 1.f};
  LssGeom g{};
  if (lss_geom(g, B, N, D, fH, fW, C, lo, dx, nx3) != GC_OK) return -1;
  const long long pixels = (long long)B * N * fH * fW;
  return (long long)lss_ws(pixels * D, pixels, C, lss_sort_bits(g)).total;
}

int gencomm_lss_splat_fwd(const float* depth_logit, const float* feat, const float* frustum, const float* rots, const float* trans,
                          const float* intrins, const float* post_rots, const float* post_trans, const float* lo3, const float* dx3,
                          const int* nx3, int B, int N, int D, int fH, int fW, int C, float* out, int* cell, void* workspace,
                          long long workspace_bytes, void* stream) {
  LssGeom g{};
  if (int rc = lss_geom(g, B, N, D, fH, fW, C, lo3, dx3, nx3)) return rc;
  GC_CHECK_ARG(depth_logit && feat && frustum && rots && trans && intrins && post_rots && post_trans && out && workspace, "null pointer");
  const long long pixels = (long long)B * N * fH * fW, npts = pixels * D;
  const int bits = lss_sort_bits(g);
  const LssWs w = lss_ws(npts, pixels, C, bits);
  if ((long long)w.total > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_lss_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  char* wsp = (char*)workspace;
  float* featT = reinterpret_cast<float*>(wsp + w.featT);
  float* prob = reinterpret_cast<float*>(wsp + w.prob);
  unsigned* key = reinterpret_cast<unsigned*>(wsp + w.key);
  unsigned* skey = reinterpret_cast<unsigned*>(wsp + w.skey);
  int* val = reinterpret_cast<int*>(wsp + w.val);
  int* sval = reinterpret_cast<int*>(wsp + w.sval);
  GC_KLOG("lss_lift_kernel");
  lss_lift_kernel<<<(unsigned)((pixels + 63) / 64), 64, 0, st>>>(depth_logit, feat, frustum, rots, trans, intrins, post_rots, post_trans, g,
                                                                 prob, featT, key, val, cell);
  GC_HIP(hipGetLastError());
  size_t tb = w.temp_bytes;
  GC_HIP(rocprim::radix_sort_pairs(wsp + w.temp, tb, key, skey, val, sval, (size_t)npts, 0, bits, st));   // stable: ties keep point order
  GC_KLOG("lss_splat_kernel");
  lss_splat_kernel<<<dim3((g.nx + kLssTx - 1) / kLssTx, g.ny, g.B * g.nz), 256, 0, st>>>(skey, sval, (int)npts, prob, featT, g, out);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_lss_depth_target_fwd(const float* imgs, int BN, int Cimg, int H, int W, int downsample, int mode, float d_min, float d_max,
                                 int num_bins, long long* indices, unsigned char* mask, void* stream) {
  GC_CHECK_ARG(imgs && indices, "null pointer");
  GC_CHECK_ARG(BN >= 1 && Cimg >= 4 && H >= 1 && W >= 1 && downsample >= 1 && num_bins >= 1 && (mode == 0 || mode == 1), "bad dims / mode");
  LssDepthArgs a{};
  a.imgs = imgs; a.idx = indices; a.mask = mask;
  a.BN = BN; a.Cimg = Cimg; a.H = H; a.W = W; a.ds = downsample; a.mode = mode; a.nb = num_bins;
  a.oH = (H - downsample / 2 + downsample - 1) / downsample;   // len(range(downsample // 2, H, downsample))
  a.oW = (W - downsample / 2 + downsample - 1) / downsample;
  GC_CHECK_ARG(a.oH >= 1 && a.oW >= 1, "image smaller than half the downsample factor");
  a.dmin = d_min; a.dmax = d_max;
  a.bin = mode == 0 ? (float)(((double)d_max - d_min) / num_bins) : (float)(2.0 * ((double)d_max - d_min) / ((double)num_bins * (1 + num_bins)));
  const long long total = (long long)BN * a.oH * a.oW;
  GC_CHECK_ARG((total + 255) / 256 < (1LL << 31), "too many pixels");
  lss_depth_target_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_maxpool3x3s2_fwd(const float* x, float* y, int N, int C, int H, int W, void* stream) {
  GC_CHECK_ARG(x && y, "null pointer");
  GC_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "bad dims");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const long long total = (long long)N * C * Ho * Wo;
  GC_CHECK_ARG((total + 255) / 256 < (1LL << 31), "tensor too large");
  maxpool3x3s2_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, y, total, H, W, Ho, Wo);
  GC_HIP(hipGetLastError());
  return GC_OK;
}


// ---- training the camera encoder: lift-splat backward, max-pool backward, stem weight gradient, depth focal loss ------------------
long long gencomm_lss_splat_bwd_workspace_bytes(int B, int C, const int* nx3) {
  if (!(nx3 && B >= 1 && C >= 1 && nx3[0] >= 1 && nx3[1] >= 1 && nx3[2] >= 1 && (long long)B * nx3[0] * nx3[1] * nx3[2] < (1LL << 31) - 1)) {
    fail(GC_ERR_ARG, "gencomm_lss_splat_bwd_workspace_bytes: bad B / C / grid");
    return -1;
  }
  return (long long)align_up((size_t)B * nx3[0] * nx3[1] * nx3[2] * C * 4, 256);
}

int gencomm_lss_splat_bwd(const float* grad_out, const void* fwd_workspace, long long fwd_workspace_bytes, const int* cell, const int* nx3,
                          int B, int N, int D, int fH, int fW, int C, float* d_depth_logit, float* d_feat, void* workspace,
                          long long workspace_bytes, void* stream) {
  const float lo[3] = {0.f, 0.f, 0.f}, dx[3] = {1.f, 1.f, 1.f};
  LssGeom g{};
  if (int rc = lss_geom(g, B, N, D, fH, fW, C, lo, dx, nx3)) return rc;
  GC_CHECK_ARG(grad_out && fwd_workspace && cell && d_depth_logit && d_feat && workspace, "null pointer");
  GC_CHECK_ARG(D <= kLssBwdMaxD, "the backward supports at most 256 depth bins");
  GC_CHECK_ARG((long long)B * N <= 65535, "too many cameras");
  const long long pixels = (long long)B * N * fH * fW, npts = pixels * D;
  const LssWs w = lss_ws(npts, pixels, C, lss_sort_bits(g));
  if ((long long)w.total > fwd_workspace_bytes) return fail(GC_ERR_WORKSPACE, "forward workspace too small (gencomm_lss_workspace_bytes)");
  const long long need = gencomm_lss_splat_bwd_workspace_bytes(B, C, nx3);
  if (need < 0) return GC_ERR_ARG;
  if (need > workspace_bytes) return fail(GC_ERR_WORKSPACE, "workspace too small (gencomm_lss_splat_bwd_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const int plane = g.ny * g.nx;
  float* gT = reinterpret_cast<float*>(workspace);
  GC_KLOG("lss_grad_rows_kernel");
  lss_grad_rows_kernel<<<dim3((plane + 63) / 64, (C + 63) / 64, g.B * g.nz), 256, 0, st>>>(grad_out, gT, C, plane);
  GC_HIP(hipGetLastError());
  LssBwdArgs a{};
  const char* fws = reinterpret_cast<const char*>(fwd_workspace);
  a.gT = gT; a.prob = reinterpret_cast<const float*>(fws + w.prob); a.featT = reinterpret_cast<const float*>(fws + w.featT);
  a.cell = cell; a.dlogit = d_depth_logit; a.dfeat = d_feat;
  a.B = g.B; a.nx = g.nx; a.ny = g.ny; a.nz = g.nz; a.D = D; a.HW = fH * fW; a.C = C;
  const size_t lds = (size_t)(D + kLssBwdCh) * kLssBwdPitch * sizeof(float);
  GC_KLOG("lss_splat_bwd_kernel");
  lss_splat_bwd_kernel<<<dim3((a.HW + kLssBwdPx - 1) / kLssBwdPx, B * N), 256, lds, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_maxpool3x3s2_bwd(const float* x, const float* dy, float* dx, int N, int C, int H, int W, void* stream) {
  GC_CHECK_ARG(x && dy && dx, "null pointer");
  GC_CHECK_ARG(N >= 1 && C >= 1 && H >= 1 && W >= 1, "bad dims");
  GC_CHECK_ARG((long long)H * W < (1LL << 31), "map too large");
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const long long total = (long long)N * C * H * W;
  GC_CHECK_ARG((total + 255) / 256 < (1LL << 31), "tensor too large");
  maxpool3x3s2_bwd_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, dy, dx, total, H, W, Ho, Wo);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

static bool stem7x7_dims(int N, int Cin, int Hi, int Wi, int Cout, long long& P, int& Ho, int& Wo) {
  if (!(N >= 1 && Cin >= 1 && Cin * 49 <= kStemTaps && Hi >= 1 && Wi >= 1 && Cout >= 64 && Cout % 64 == 0 && Cout / 64 <= 65535)) return false;
  Ho = (Hi + 6 - 7) / 2 + 1; Wo = (Wi + 6 - 7) / 2 + 1;
  P = (long long)N * Ho * Wo;
  return P < (1LL << 31) - kStemPx * (long long)kStemMaxSplit && (long long)N * Cin * Hi * Wi < (1LL << 40);
}
long long gencomm_stem7x7_wgrad_scratch_floats(int N, int Cin, int Hi, int Wi, int Cout) {
  long long P; int Ho, Wo;
  if (!stem7x7_dims(N, Cin, Hi, Wi, Cout, P, Ho, Wo)) {
    fail(GC_ERR_ARG, "gencomm_stem7x7_wgrad_scratch_floats: bad dims (Cin <= 3, Cout a multiple of 64)");
    return -1;
  }
  return (long long)stem7x7_split(P) * Cout * Cin * 49;
}
int gencomm_stem7x7_wgrad(const float* dy, const float* x, float* dw, int N, int Cin, int Hi, int Wi, int Cout, float* scratch,
                          long long scratch_floats, void* stream) {
  GC_CHECK_ARG(dy && x && dw && scratch, "null pointer");
  long long P; int Ho, Wo;
  GC_CHECK_ARG(stem7x7_dims(N, Cin, Hi, Wi, Cout, P, Ho, Wo), "bad dims (7x7 stride 2 pad 3: Cin <= 3, Cout a multiple of 64)");
  const int S = stem7x7_split(P);
  GC_CHECK_ARG(scratch_floats >= (long long)S * Cout * Cin * 49, "scratch smaller than gencomm_stem7x7_wgrad_scratch_floats");
  StemWgradArgs a{};
  a.dy = dy; a.x = x; a.part = scratch; a.N = N; a.Cin = Cin; a.Hi = Hi; a.Wi = Wi; a.Cout = Cout; a.Ho = Ho; a.Wo = Wo; a.P = (int)P;
  a.per = (int)(((P + S - 1) / S + kStemPx - 1) / kStemPx * kStemPx);
  hipStream_t st = (hipStream_t)stream;
  GC_KLOG("stem7x7_wgrad_kernel");
  stem7x7_wgrad_kernel<<<dim3(S, Cout / 64), 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  const int total = Cout * Cin * 49;
  stem7x7_wgrad_reduce_kernel<<<(total + 255) / 256, 256, 0, st>>>(scratch, dw, S, total);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_depth_focal_loss(const float* depth_logit, const long long* target, float* grad, double* sum, int BN, int D, int H, int W,
                             float alpha, float gamma, float scale, void* stream) {
  GC_CHECK_ARG(depth_logit && target && grad && sum, "null pointer");
  GC_CHECK_ARG(BN >= 1 && D >= 1 && H >= 1 && W >= 1 && (long long)H * W < (1LL << 31), "bad dims");
  GC_CHECK_ARG(gamma >= 0.f, "gamma must not be negative");
  DepthFocalArgs a{};
  a.logit = depth_logit; a.target = target; a.grad = grad; a.sum = sum; a.D = D; a.HW = H * W; a.total = (long long)BN * H * W;
  a.alpha = alpha; a.gamma = gamma; a.scale = scale;
  GC_CHECK_ARG((a.total + 255) / 256 < (1LL << 31), "too many pixels");
  depth_focal_loss_kernel<<<(unsigned)((a.total + 255) / 256), 256, 0, (hipStream_t)stream>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- CodeFilling codebook codec (codebook_kernels.h)
long long gencomm_umgm_param_floats(int C, int m, const int* k, int levels) {
  if (umgm_check_shape(C, m, k, levels) != GC_OK) return -1;
  long long total = 0;
  for (int l = 0; l < levels; ++l) total += umgm_level_floats(C, k[l]);
  return total;
}

long long gencomm_umgm_workspace_bytes(long long n, int C) {
  if (n < 1 || !(C == 64 || C == 128 || C == 256)) {
    fail(GC_ERR_ARG, "umgm workspace: n must be at least 1 and channel 64, 128 or 256");
    return -1;
  }
  return (long long)((n + kUmgmRows - 1) / kUmgmRows) * (long long)sizeof(float);
}

static int umgm_rows(long long n, int HW, long long* rows) {
  GC_CHECK_ARG(n >= 1, "umgm: n must be at least 1");
  GC_CHECK_ARG(HW >= 0 && HW < (1 << 30), "umgm: HW must be 0 (rows [n][C]) or the pixels of one NCHW map");
  *rows = HW > 0 ? n * HW : n;   // NCHW: n counts agents
  return GC_OK;
}

int gencomm_umgm_fwd(const float* params, const float* x, const unsigned char* keep, const float* uniforms, unsigned long long seed, int noise,
                     float* restored, long long* codes, long long* sampled, float* logits, float* code_loss, long long n, int HW, int C, int m,
                     const int* k, int levels, void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = umgm_check_shape(C, m, k, levels)) return rc;
  GC_CHECK_ARG(params && x && restored && codes && code_loss, "umgm forward: null pointer");
  GC_CHECK_ARG(noise >= UMGM_NOISE_NONE && noise <= UMGM_NOISE_PHILOX, "umgm forward: noise must be 0 (none), 1 (uniforms) or 2 (Philox)");
  GC_CHECK_ARG(noise != UMGM_NOISE_UNIFORMS || uniforms, "umgm forward: null pointer (uniforms with noise 1)");
  GC_CHECK_ARG(keep == nullptr || HW > 0, "umgm forward: keep needs the NCHW entry (HW > 0)");
  GC_CHECK_ARG(((((uintptr_t)params | (uintptr_t)x | (uintptr_t)restored)) & 15) == 0, "umgm forward: params, x and restored must be 16-byte aligned");
  long long rows = 0;
  if (int rc = umgm_rows(n, HW, &rows)) return rc;
  const long long need = gencomm_umgm_workspace_bytes(rows, C);
  if (workspace == nullptr || workspace_bytes < need) return fail(GC_ERR_WORKSPACE, "umgm forward: workspace too small (gencomm_umgm_workspace_bytes)");
  UmgmArgs a{};
  a.params = params; a.x = x; a.keep = keep; a.uniforms = uniforms; a.out = restored; a.codes = codes; a.sampled = sampled; a.logits = logits;
  a.partials = (float*)workspace; a.n = rows; a.seed = seed; a.HW = HW; a.m = m; a.L = levels; a.task = UMGM_FORWARD; a.noise = noise;
  return umgm_launch(a, C, k, code_loss, (hipStream_t)stream);
}

int gencomm_umgm_encode_fwd(const float* params, const float* x, long long* codes, long long n, int HW, int C, int m, const int* k, int levels,
                            void* stream) {
  if (int rc = umgm_check_shape(C, m, k, levels)) return rc;
  GC_CHECK_ARG(params && x && codes, "umgm encode: null pointer");
  GC_CHECK_ARG((((uintptr_t)params | (uintptr_t)x) & 15) == 0, "umgm encode: params and x must be 16-byte aligned");
  long long rows = 0;
  if (int rc = umgm_rows(n, HW, &rows)) return rc;
  UmgmArgs a{};
  a.params = params; a.x = x; a.codes = codes; a.n = rows; a.HW = HW; a.m = m; a.L = levels; a.task = UMGM_ENCODE; a.noise = UMGM_NOISE_NONE;
  return umgm_launch(a, C, k, nullptr, (hipStream_t)stream);
}

int gencomm_umgm_decode_fwd(const float* params, const long long* codes, float* restored, long long n, int HW, int C, int m, const int* k, int levels,
                            void* stream) {
  if (int rc = umgm_check_shape(C, m, k, levels)) return rc;
  GC_CHECK_ARG(params && codes && restored, "umgm decode: null pointer");
  GC_CHECK_ARG((((uintptr_t)params | (uintptr_t)restored) & 15) == 0, "umgm decode: params and restored must be 16-byte aligned");
  long long rows = 0;
  if (int rc = umgm_rows(n, HW, &rows)) return rc;
  UmgmArgs a{};
  a.params = params; a.codes = const_cast<long long*>(codes); a.out = restored; a.n = rows; a.HW = HW; a.m = m; a.L = levels; a.task = UMGM_DECODE;
  a.noise = UMGM_NOISE_NONE;
  return umgm_launch(a, C, k, nullptr, (hipStream_t)stream);
}

int gencomm_umgm_noise_fwd(float* out, unsigned long long seed, long long n, int m, const int* k, int levels, void* stream) {
  if (int rc = umgm_check_shape(64, m, k, levels)) return rc;
  GC_CHECK_ARG(out && ((uintptr_t)out & 15) == 0, "umgm noise: out must be a 16-byte aligned pointer");
  GC_CHECK_ARG(n >= 1, "umgm noise: n must be at least 1");
  long long off = 0;
  for (int l = 0; l < levels; ++l) {
    const long long items = n * m * (k[l] / 4);
    const unsigned blocks = (unsigned)std::min<long long>((items + 255) / 256, 1 << 20);
    umgm_noise_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(out + off, seed, l, n, m, k[l]);
    off += n * m * k[l];
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- the codec's straight-through backward (codebook_bwd_kernels.h)
long long gencomm_umgm_bwd_workspace_bytes(long long rows, int C, int m, const int* k, int levels) {
  if (umgm_check_shape(C, m, k, levels) != GC_OK) return -1;
  if (rows < 1) {
    fail(GC_ERR_ARG, "umgm backward workspace: rows must be at least 1");
    return -1;
  }
  return umgm_bwd_plan(rows, C, m, k, levels).total * (long long)sizeof(float);
}

int gencomm_umgm_bwd(const float* params, const float* x, const unsigned char* keep, const float* uniforms, unsigned long long seed, int noise,
                     const long long* sampled, const float* d_restored, const float* d_loss, float* dx, float* dparams, int dx_only, long long n,
                     int HW, int C, int m, const int* k, int levels, void* workspace, long long workspace_bytes, void* stream) {
  if (int rc = umgm_check_shape(C, m, k, levels)) return rc;
  GC_CHECK_ARG(params && x, "umgm backward: null pointer (params, x)");
  GC_CHECK_ARG(sampled, "umgm backward: null pointer (sampled: the indices the forward returned)");
  GC_CHECK_ARG(dx, "umgm backward: null pointer (dx)");
  GC_CHECK_ARG(dx_only == 0 || dx_only == 1, "umgm backward: dx_only must be 0 or 1");
  GC_CHECK_ARG(dx_only || dparams, "umgm backward: null pointer (dparams without dx_only)");
  GC_CHECK_ARG(noise >= UMGM_NOISE_NONE && noise <= UMGM_NOISE_PHILOX, "umgm backward: noise must be 0 (none), 1 (uniforms) or 2 (Philox)");
  GC_CHECK_ARG(noise != UMGM_NOISE_UNIFORMS || uniforms, "umgm backward: null pointer (uniforms with noise 1)");
  GC_CHECK_ARG(keep == nullptr || HW > 0, "umgm backward: keep needs the NCHW entry (HW > 0)");
  GC_CHECK_ARG(((((uintptr_t)params | (uintptr_t)x | (uintptr_t)dx | (uintptr_t)d_restored | (uintptr_t)uniforms | (uintptr_t)dparams | (uintptr_t)workspace)) & 15) == 0,
               "umgm backward: params, x, dx, d_restored, uniforms, dparams and workspace must be 16-byte aligned");
  long long rows = 0;
  if (int rc = umgm_rows(n, HW, &rows)) return rc;
  const long long need = gencomm_umgm_bwd_workspace_bytes(rows, C, m, k, levels);
  if (workspace == nullptr || workspace_bytes < need) return fail(GC_ERR_WORKSPACE, "umgm backward: workspace too small (gencomm_umgm_bwd_workspace_bytes)");
  UmgmBwdArgs b{};
  b.f.params = params; b.f.x = x; b.f.keep = keep; b.f.uniforms = uniforms; b.f.n = rows; b.f.seed = seed; b.f.HW = HW; b.f.m = m; b.f.L = levels;
  b.f.task = UMGM_FORWARD; b.f.noise = noise;
  b.sampled = sampled; b.d_restored = d_restored; b.d_loss = d_loss; b.dx = dx; b.dx_only = dx_only;
  return umgm_bwd_launch(b, C, k, dparams, (float*)workspace, (hipStream_t)stream);
}

long long gencomm_rows_wgrad_fixed_scratch_floats(long long rows, int Co, int Ci) {
  if (rows < 1 || Co < 64 || Ci < 64 || Co % 64 || Ci % 64 || Co > 4096 || Ci > 4096) {
    fail(GC_ERR_ARG, "rows wgrad scratch: rows must be at least 1, Co and Ci multiples of 64 in 64 .. 4096");
    return -1;
  }
  return rows_wgrad_scratch_floats(rows, Co, Ci, 1);
}

int gencomm_rows_wgrad_fixed(const float* g, const float* a, float* dw, long long rows, int Co, int Ci, float* scratch, long long scratch_floats,
                             void* stream) {
  GC_CHECK_ARG(g && a && dw, "rows wgrad: null pointer (g, a, dw)");
  GC_CHECK_ARG(rows >= 1, "rows wgrad: rows must be at least 1");
  GC_CHECK_ARG(Co >= 64 && Co <= 4096 && Co % 64 == 0, "rows wgrad: Co must be a multiple of 64 in 64 .. 4096");
  GC_CHECK_ARG(Ci >= 64 && Ci <= 4096 && Ci % 64 == 0, "rows wgrad: Ci must be a multiple of 64 in 64 .. 4096");
  if (scratch == nullptr || scratch_floats < rows_wgrad_scratch_floats(rows, Co, Ci, 1))
    return fail(GC_ERR_WORKSPACE, "rows wgrad: scratch too small (gencomm_rows_wgrad_fixed_scratch_floats)");
  RowsWgradArgs w{};
  w.G[0] = g; w.A[0] = a; w.out[0] = dw; w.part = scratch; w.rows = rows; w.Co = Co; w.Ci = Ci; w.count = 1;
  return rows_wgrad_launch(w, (hipStream_t)stream);
}

// ---- STAMP's ConvNeXt block (convnext_kernels.h)
int gencomm_convnext_block_fwd(const float* x, const float* dw_weight, const float* dw_bias, const float* ln_weight, const float* ln_bias,
                               const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma, float* y,
                               int n, int C, int H, int W, void* stream) {
  CnxArgs a{x, dw_weight, dw_bias, ln_weight, ln_bias, w1, b1, w2, b2, gamma, y, H, W, 0};
  return convnext_block_launch(a, n, C, (hipStream_t)stream);
}

// ---- its adjoint (convnext_bwd_kernels.h)
static int cnx_bwd_check_shape(int n, int C, int H, int W, int dx_only, int slabs) {
  if (C != 64 && C != 128) {
    char msg[96];
    snprintf(msg, sizeof msg, "convnext block backward: C must be 64 or 128 (got %d)", C);
    return fail(GC_ERR_ARG, msg);
  }
  GC_CHECK_ARG(n >= 1 && n <= 65535 && H >= 1 && W >= 1, "convnext block backward: 1..65535 maps (n), positive H / W");
  GC_CHECK_ARG((H + kCnxTileH - 1) / kCnxTileH <= 65535, "convnext block backward: H must be at most 262140");
  GC_CHECK_ARG((long long)n * ((H + kCnxTileH - 1) / kCnxTileH) * ((W + kCnxTileW - 1) / kCnxTileW) <= 0x7fffffffll,
               "convnext block backward: n, H, W give more than 2^31 - 1 tiles");
  GC_CHECK_ARG(dx_only == 0 || dx_only == 1, "convnext block backward: dx_only must be 0 or 1");
  GC_CHECK_ARG(slabs >= 0 && slabs <= 65535, "convnext block backward: slabs must be 0 (automatic) .. 65535");
  return GC_OK;
}

long long gencomm_convnext_block_bwd_workspace_bytes(int n, int C, int H, int W, int dx_only, int slabs) {
  if (cnx_bwd_check_shape(n, C, H, W, dx_only, slabs) != GC_OK) return -1;
  return cnx_bwd_plan(n, C, H, W, dx_only, slabs).total * (long long)sizeof(float);
}

int gencomm_convnext_block_bwd(const float* x, const float* dy, const float* dw_weight, const float* dw_bias, const float* ln_weight,
                               const float* ln_bias, const float* w1, const float* b1, const float* w2, const float* b2, const float* gamma,
                               float* dx, float* d_dw_weight, float* d_dw_bias, float* d_ln_weight, float* d_ln_bias, float* d_w1, float* d_b1,
                               float* d_w2, float* d_b2, float* d_gamma, int dx_only, int slabs, int n, int C, int H, int W, void* workspace,
                               long long workspace_bytes, void* stream) {
  if (int rc = cnx_bwd_check_shape(n, C, H, W, dx_only, slabs)) return rc;
  GC_CHECK_ARG(x && dy && dx, "convnext block backward: null pointer (x, dy, dx)");
  GC_CHECK_ARG(dw_weight && dw_bias && ln_weight && ln_bias && w1 && b1 && w2 && b2, "convnext block backward: null pointer (a parameter other than gamma)");
  GC_CHECK_ARG(dx_only || (d_dw_weight && d_dw_bias && d_ln_weight && d_ln_bias && d_w1 && d_b1 && d_w2 && d_b2),
               "convnext block backward: null pointer (a parameter gradient without dx_only)");
  GC_CHECK_ARG(dx_only || gamma == nullptr || d_gamma, "convnext block backward: null pointer (d_gamma with gamma and without dx_only)");
  GC_CHECK_ARG((((uintptr_t)w1 | (uintptr_t)workspace) & 15) == 0, "convnext block backward: w1 and workspace must be 16-byte aligned");
  GC_CHECK_ARG((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)dx) & 3) == 0, "convnext block backward: x, dy and dx must be 4-byte aligned");
  const size_t bytes = (size_t)n * C * H * W * sizeof(float);
  const uintptr_t xb = (uintptr_t)x, db = (uintptr_t)dx, yb = (uintptr_t)dy;
  GC_CHECK_ARG(xb + bytes <= db || db + bytes <= xb, "convnext block backward: dx must not alias x (the tap gradients read x's halo)");
  GC_CHECK_ARG(db == yb || yb + bytes <= db || db + bytes <= yb, "convnext block backward: dx must be dy itself or not overlap dy");
  const CnxBwdPlan p = cnx_bwd_plan(n, C, H, W, dx_only, slabs);
  if (workspace == nullptr || workspace_bytes < p.total * (long long)sizeof(float))
    return fail(GC_ERR_WORKSPACE, "convnext block backward: workspace too small (gencomm_convnext_block_bwd_workspace_bytes)");
  float* ws = (float*)workspace;
  CnxBwdArgs a{};
  a.x = x; a.dy = dy; a.dw_w = dw_weight; a.dw_b = dw_bias; a.ln_w = ln_weight; a.ln_b = ln_bias; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.gamma = gamma; a.dx = dx;
  a.g_dw_w = d_dw_weight; a.g_dw_b = d_dw_bias; a.g_ln_w = d_ln_weight; a.g_ln_b = d_ln_bias; a.g_w1 = d_w1; a.g_b1 = d_b1; a.g_w2 = d_w2;
  a.g_b2 = d_b2; a.g_gamma = gamma != nullptr ? d_gamma : nullptr;
  a.w1t = ws + p.w1t; a.w2g = ws + p.w2g; a.xh = ws + p.xh; a.dd = ws + p.dd; a.p_ln = ws + p.p_ln;
  if (!dx_only) {
    a.p_w = ws + p.p_w; a.p_dw = ws + p.p_dw; a.s_red = ws + p.s_red; a.sdy = ws + p.sdy;
  }
  a.n = n; a.H = H; a.W = W; a.tx = p.tx; a.ty = p.ty; a.tiles = p.tiles; a.slabs = p.slabs; a.tps = p.tps; a.dx_only = dx_only;
  a.vec = (W % 4 == 0 && ((yb | db) & 15) == 0) ? 1 : 0;
  return convnext_block_bwd_launch(a, C, (hipStream_t)stream);
}

// ---- HEAL's PyramidFusion (pyramid_kernels.h)
static int gconv_check(int n, int C, int cpg, int H, int W, int stride) {
  if (cpg != 4 && cpg != 8 && cpg != 16) {
    char msg[128];
    snprintf(msg, sizeof msg, "grouped 3x3: unsupported group width %d channels per group (built: 4, 8, 16 with 32 groups)", cpg);
    return fail(GC_ERR_ARG, msg);
  }
  if (C != 32 * cpg) {
    char msg[128];
    snprintf(msg, sizeof msg, "grouped 3x3: C must be 32 groups x %d = %d channels in AND out (got %d)", cpg, 32 * cpg, C);
    return fail(GC_ERR_ARG, msg);
  }
  GC_CHECK_ARG(stride == 1 || stride == 2, "grouped 3x3: stride must be 1 or 2 (dilation 1, padding 1)");
  GC_CHECK_ARG(n >= 1 && n <= 65535 && H >= 1 && W >= 1, "grouped 3x3: 1..65535 maps (n), positive H / W");
  const long long Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  GC_CHECK_ARG(((Ho + kGcTileH - 1) / kGcTileH) * ((Wo + kGcTileW - 1) / kGcTileW) <= 0x7fffffffll && (long long)H * W <= 0x7fffffffll,
               "grouped 3x3: the map has more than 2^31 - 1 tiles or pixels");
  return GC_OK;
}

int gencomm_gconv3x3_prepare(const float* weight, float* packed, int cpg, void* stream) {
  if (int rc = gconv_check(1, 32 * cpg, cpg, 1, 1, 1)) return rc;
  GC_CHECK_ARG(weight && packed, "grouped 3x3 prepare: null pointer");
  const int total = 32 * cpg * cpg * 9;
  gconv3x3_pack_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(weight, packed, cpg);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_gconv3x3_fwd(const float* x, const float* packed, const float* scale, const float* shift, float* y, int n, int C, int cpg, int H, int W,
                         int stride, int relu, void* stream) {
  if (int rc = gconv_check(n, C, cpg, H, W, stride)) return rc;
  GC_CHECK_ARG(x && packed && scale && shift && y, "grouped 3x3: null pointer");
  return gconv3x3_enqueue(x, packed, scale, shift, y, n, cpg, H, W, stride, relu ? 1 : 0, (hipStream_t)stream);
}

int gencomm_pyramid_score_fwd(const float* x, const float* weight, const float* bias, const int* rect, float* occ, float* score, int n, int C, int H,
                              int W, void* stream) {
  GC_CHECK_ARG(x && weight && bias && occ && score, "pyramid score: null pointer (rect alone may be null)");
  GC_CHECK_ARG(n >= 1 && n <= 65535 && C >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffll - 64, "pyramid score: bad n/C/H/W");
  PyrScoreArgs a{x, weight, bias, rect, occ, score, C, H, W};
  return pyramid_score_enqueue(a, n, (hipStream_t)stream);
}

int gencomm_warp_weightfuse_fwd(const float* x, const float* score, const double* theta, const int* scene_off, float* out, int B, int n, int C, int H,
                                int W, void* stream) {
  GC_CHECK_ARG(x && score && theta && scene_off && out, "weighted fuse: null pointer");
  GC_CHECK_ARG(B >= 1 && B <= 65535 && n >= B && C >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffll - 64, "weighted fuse: bad B/n/C/H/W");
  WeightFuseArgs a{x, score, theta, scene_off, out, C, H, W, 0};
  return warp_weightfuse_enqueue(a, B, (hipStream_t)stream);
}

// ---- MPDA's feature aligner (mpda_kernels.h)
int gencomm_quad_attn_fwd(const float* q, const float* k, const float* v, const float* bias_table, float* out, int N, int Nkv, int heads,
                          int dim_head, int H, int W, int q_ct, int kv_ct, int grid_mode, void* stream) {
  GC_CHECK_ARG(q && k && v && out, "quad attention: null pointer (bias_table alone may be null)");
  if (dim_head != 16 && dim_head != 32 && dim_head != 64) {
    char msg[128];
    snprintf(msg, sizeof msg, "quad attention: unsupported dim_head %d (built: 16, 32, 64)", dim_head);
    return fail(GC_ERR_ARG, msg);
  }
  GC_CHECK_ARG(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0, "quad attention: H and W must be even and >= 2 (2 x 2 groups)");
  GC_CHECK_ARG((long long)H * W <= 0x7fffffffll, "quad attention: the map has more than 2^31 - 1 pixels");
  GC_CHECK_ARG(N >= 1 && N <= 65535 && heads >= 1 && heads <= 65535, "quad attention: 1..65535 query maps (N) and heads");
  GC_CHECK_ARG(Nkv == N || Nkv == 1, "quad attention: Nkv must be N, or 1 (one key / value map for every query map)");
  GC_CHECK_ARG(grid_mode == 0 || grid_mode == 1, "quad attention: grid_mode must be 0 (window) or 1 (grid)");
  GC_CHECK_ARG((long long)heads * dim_head <= q_ct && (long long)heads * dim_head <= kv_ct,
               "quad attention: q_ct / kv_ct (channels of one map of the q and of the k / v tensor) must be >= heads * dim_head");
  GC_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 8 == 0, "quad attention: q, k, v and out must be 8-byte aligned");
  QuadArgs a{q, k, v, bias_table, out, heads, H, W, q_ct, kv_ct, grid_mode, Nkv == 1 ? 1 : 0, 1.0f / sqrtf((float)dim_head)};
  if (dim_head == 16) return quad_attn_launch<16>(a, N, (hipStream_t)stream);
  if (dim_head == 32) return quad_attn_launch<32>(a, N, (hipStream_t)stream);
  return quad_attn_launch<64>(a, N, (hipStream_t)stream);
}

int gencomm_resize_bilinear_fwd(const float* x, float* y, int N, int C, int Hi, int Wi, int Ho, int Wo, void* stream) {
  GC_CHECK_ARG(x && y, "bilinear resize: null pointer");
  GC_CHECK_ARG(N >= 1 && C >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "bilinear resize: bad N/C/Hi/Wi/Ho/Wo");
  GC_CHECK_ARG((long long)Hi * Wi <= 0x7fffffffll && (long long)Ho * Wo <= 0x7fffffffll - 256, "bilinear resize: a map has more than 2^31 - 1 pixels");
  ResizeArgs a{x, y, Hi, Wi, Ho, Wo, (long long)N * C, 0.f, 0.f};
  return resize_bilinear_enqueue(a, (hipStream_t)stream);
}

// ---- MPDA training (mpda_bwd_kernels.h)
static int quad_domain(const char* what, int N, int Nkv, int heads, int dim_head, int H, int W, int q_ct, int kv_ct, int grid_mode) {
  char msg[160];
  if (dim_head != 16 && dim_head != 32 && dim_head != 64) {
    snprintf(msg, sizeof msg, "%s: unsupported dim_head %d (built: 16, 32, 64)", what, dim_head);
    return fail(GC_ERR_ARG, msg);
  }
  const char* bad = nullptr;
  if (!(H >= 2 && W >= 2 && H % 2 == 0 && W % 2 == 0)) bad = "H and W must be even and >= 2 (2 x 2 groups)";
  else if ((long long)H * W > 0x7fffffffll) bad = "the map has more than 2^31 - 1 pixels";
  else if (!(N >= 1 && N <= 65535 && heads >= 1 && heads <= 65535)) bad = "1..65535 query maps (N) and heads";
  else if (!(Nkv == N || Nkv == 1)) bad = "Nkv must be N, or 1 (one key / value map for every query map)";
  else if (!(grid_mode == 0 || grid_mode == 1)) bad = "grid_mode must be 0 (window) or 1 (grid)";
  else if (!((long long)heads * dim_head <= q_ct && (long long)heads * dim_head <= kv_ct))
    bad = "q_ct / kv_ct (channels of one map of the q and of the k / v tensor) must be >= heads * dim_head";
  if (bad == nullptr) return GC_OK;
  snprintf(msg, sizeof msg, "%s: %s", what, bad);
  return fail(GC_ERR_ARG, msg);
}

int gencomm_quad_attn_train_fwd(const float* q, const float* k, const float* v, const float* bias_table, const unsigned short* keep, float keep_scale,
                                float* out, int N, int Nkv, int heads, int dim_head, int H, int W, int q_ct, int kv_ct, int grid_mode, void* stream) {
  GC_CHECK_ARG(q && k && v && out, "quad attention train: null pointer (bias_table and keep alone may be null)");
  if (int rc = quad_domain("quad attention train", N, Nkv, heads, dim_head, H, W, q_ct, kv_ct, grid_mode)) return rc;
  GC_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)out) % 8 == 0, "quad attention train: q, k, v and out must be 8-byte aligned");
  GC_CHECK_ARG((uintptr_t)keep % 2 == 0, "quad attention train: keep must be 2-byte aligned");
  QuadTrainArgs a{{q, k, v, bias_table, out, heads, H, W, q_ct, kv_ct, grid_mode, Nkv == 1 ? 1 : 0, 1.0f / sqrtf((float)dim_head)}, keep, keep_scale};
  if (dim_head == 16) return quad_attn_train_launch<16>(a, N, (hipStream_t)stream);
  if (dim_head == 32) return quad_attn_train_launch<32>(a, N, (hipStream_t)stream);
  return quad_attn_train_launch<64>(a, N, (hipStream_t)stream);
}

// workspace: [2][N][heads dim_head][H][W] floats of per-map dk | dv slabs where one key / value map serves N > 1 query maps, then
// [N ceil(X Y / 64)][heads][9] floats of per-workgroup partials of the table's gradient where there is a table
static long long quad_bwd_slab_floats(int N, int Nkv, int heads, int dim_head, int H, int W) {
  return (Nkv == 1 && N > 1) ? 2ll * N * heads * dim_head * H * W : 0ll;
}

long long gencomm_quad_attn_bwd_workspace_bytes(int N, int Nkv, int heads, int dim_head, int H, int W, int has_bias) {
  if (quad_domain("quad attention backward", N, Nkv, heads, dim_head, H, W, heads * dim_head, heads * dim_head, 0)) return -1;
  const long long wgs = (long long)N * (((H / 2) * (W / 2) + kQuadGroups - 1) / kQuadGroups);
  return (long long)align_up((size_t)(quad_bwd_slab_floats(N, Nkv, heads, dim_head, H, W) + (has_bias ? wgs * heads * 9 : 0)) * sizeof(float), 256);
}

int gencomm_quad_attn_bwd(const float* q, const float* k, const float* v, const float* bias_table, const unsigned short* keep, float keep_scale,
                          const float* dout, float* dq, float* dk, float* dv, float* dbias, int N, int Nkv, int heads, int dim_head, int H, int W,
                          int q_ct, int kv_ct, int grid_mode, void* workspace, long long workspace_bytes, void* stream) {
  GC_CHECK_ARG(q && k && v && dout && dq && dk && dv, "quad attention backward: null pointer (bias_table, dbias, keep and an empty workspace alone may be null)");
  GC_CHECK_ARG(bias_table == nullptr || dbias != nullptr, "quad attention backward: null pointer (dbias with a bias_table)");
  if (int rc = quad_domain("quad attention backward", N, Nkv, heads, dim_head, H, W, q_ct, kv_ct, grid_mode)) return rc;
  GC_CHECK_ARG(((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)workspace) % 8 == 0,
               "quad attention backward: q, k, v, dout, dq, dk, dv and the workspace must be 8-byte aligned");
  GC_CHECK_ARG((uintptr_t)keep % 2 == 0, "quad attention backward: keep must be 2-byte aligned");
  const long long need = gencomm_quad_attn_bwd_workspace_bytes(N, Nkv, heads, dim_head, H, W, bias_table != nullptr);
  if (need > 0 && (workspace == nullptr || workspace_bytes < need))
    return fail(GC_ERR_WORKSPACE, "quad attention backward: workspace too small (gencomm_quad_attn_bwd_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const long long slab = quad_bwd_slab_floats(N, Nkv, heads, dim_head, H, W);
  const long long count = (long long)heads * dim_head * H * W;
  GC_CHECK_ARG((count + 255) / 256 <= 0x7fffffffll, "quad attention backward: heads * dim_head * H * W too large");
  float* ws = reinterpret_cast<float*>(workspace);
  float* part = bias_table != nullptr ? ws + slab : nullptr;
  QuadBwdArgs a{q, k, v, bias_table, dout, keep, dq, dk, dv, part, heads, H, W, q_ct, kv_ct, kv_ct, grid_mode, Nkv == 1 ? 1 : 0,
                1.0f / sqrtf((float)dim_head), keep_scale};
  if (slab) { a.dk = ws; a.dv = ws + slab / 2; a.dkv_ct = heads * dim_head; }
  int rc = dim_head == 16 ? quad_attn_bwd_launch<16>(a, N, st) : dim_head == 32 ? quad_attn_bwd_launch<32>(a, N, st) : quad_attn_bwd_launch<64>(a, N, st);
  if (rc) return rc;
  if (slab) {
    GC_KLOG("quad_kv_reduce_kernel");
    quad_kv_reduce_kernel<<<dim3((unsigned)((count + 255) / 256), 2), 256, 0, st>>>(ws, dk, dv, N, count);
  }
  if (part != nullptr) {
    const int P = N * (((H / 2) * (W / 2) + kQuadGroups - 1) / kQuadGroups);
    GC_KLOG("quad_dbias_reduce_kernel");
    quad_dbias_reduce_kernel<<<dim3(9, heads), 64, 0, st>>>(part, dbias, P, heads);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_resize_bilinear_bwd(const float* dy, float* dx, int N, int C, int Hi, int Wi, int Ho, int Wo, void* stream) {
  GC_CHECK_ARG(dy && dx, "bilinear resize backward: null pointer");
  GC_CHECK_ARG(N >= 1 && C >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "bilinear resize backward: bad N/C/Hi/Wi/Ho/Wo");
  GC_CHECK_ARG((long long)Hi * Wi <= 0x7fffffffll - 256 && (long long)Ho * Wo <= 0x7fffffffll,
               "bilinear resize backward: a map has more than 2^31 - 1 pixels");
  ResizeBwdArgs a{dy, dx, Hi, Wi, Ho, Wo, (long long)N * C, 0.f, 0.f};
  return resize_bilinear_bwd_enqueue(a, (hipStream_t)stream);
}

static unsigned ew_blocks(long long n) { return (unsigned)std::min<long long>((n + 255) / 256, 1 << 20); }

int gencomm_leaky_relu_fwd(const float* x, float* y, long long n, float slope, void* stream) {
  GC_CHECK_ARG(x && y, "leaky relu: null pointer");
  GC_CHECK_ARG(n >= 1, "leaky relu: n must be >= 1");
  GC_KLOG("leaky_relu_fwd_kernel");
  leaky_relu_fwd_kernel<<<ew_blocks(n), 256, 0, (hipStream_t)stream>>>(x, y, n, slope);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_leaky_relu_bwd(const float* y, const float* dy, float* dx, long long n, float slope, void* stream) {
  GC_CHECK_ARG(y && dy && dx, "leaky relu backward: null pointer");
  GC_CHECK_ARG(n >= 1, "leaky relu backward: n must be >= 1");
  GC_KLOG("leaky_relu_bwd_kernel");
  leaky_relu_bwd_kernel<<<ew_blocks(n), 256, 0, (hipStream_t)stream>>>(y, dy, dx, n, slope);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// ---- HEAL's PyramidFusion, training (pyramid_bwd_kernels.h)
int gencomm_gconv3x3_prepare_t(const float* weight, float* packed, int cpg, void* stream) {
  if (int rc = gconv_check(1, 32 * cpg, cpg, 1, 1, 1)) return rc;
  GC_CHECK_ARG(weight && packed, "grouped 3x3 prepare (transposed): null pointer");
  const int total = 32 * cpg * cpg * 9;
  gconv3x3_pack_t_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(weight, packed, cpg);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

int gencomm_gconv3x3_dgrad(const float* dy, const float* packed_t, const float* unit_scale, const float* zero_shift, float* dx, float* spread, int n,
                           int C, int cpg, int H, int W, int stride, void* stream) {
  if (int rc = gconv_check(n, C, cpg, H, W, stride)) return rc;
  GC_CHECK_ARG(dy && packed_t && unit_scale && zero_shift && dx, "grouped 3x3 dgrad: null pointer");
  GC_CHECK_ARG(stride == 1 || spread != nullptr, "grouped 3x3 dgrad: stride 2 needs the spread buffer (n C H W floats)");
  GC_CHECK_ARG(dx != dy && dx != spread, "grouped 3x3 dgrad: dx must not alias dy or the spread buffer (neighbouring tiles read the halo)");
  hipStream_t st = (hipStream_t)stream;
  const float* src = dy;
  if (stride == 2) {
    const long long maps = (long long)n * C, total = maps * H * W;
    gconv3x3_spread_kernel<<<(unsigned)std::min<long long>((total + 255) / 256, 1 << 20), 256, 0, st>>>(dy, spread, maps, H, W, (H - 1) / 2 + 1,
                                                                                                         (W - 1) / 2 + 1);
    src = spread;
  }
  return gconv3x3_enqueue(src, packed_t, unit_scale, zero_shift, dx, n, cpg, H, W, 1, 0, st);
}

long long gencomm_gconv3x3_wgrad_fixed_scratch_floats(int n, int cpg, int H, int W, int stride) {
  if (gconv_check(n, 32 * cpg, cpg, H, W, stride)) return -1;
  return (long long)gconv3x3_wgrad_plan(n, cpg, H, W, stride).slabs * 32 * 9 * cpg * cpg;
}

int gencomm_gconv3x3_wgrad_fixed(const float* x, const float* dy, float* dw, int n, int C, int cpg, int H, int W, int stride, float* scratch,
                                 long long scratch_floats, void* stream) {
  if (int rc = gconv_check(n, C, cpg, H, W, stride)) return rc;
  GC_CHECK_ARG(x && dy && dw && scratch, "grouped 3x3 wgrad: null pointer");
  GC_CHECK_ARG(gconv3x3_wgrad_plan(n, cpg, H, W, stride).total_tiles <= 0x7fffffffll, "grouped 3x3 wgrad: more than 2^31 - 1 tiles");
  if (scratch_floats < gencomm_gconv3x3_wgrad_fixed_scratch_floats(n, cpg, H, W, stride))
    return fail(GC_ERR_WORKSPACE, "grouped 3x3 wgrad: scratch too small (gencomm_gconv3x3_wgrad_fixed_scratch_floats)");
  return gconv3x3_wgrad_enqueue(x, dy, dw, scratch, n, cpg, H, W, stride, (hipStream_t)stream);
}

long long gencomm_pyramid_score_bwd_scratch_floats(int n, int C, int H, int W) {
  if (!(n >= 1 && n <= 65535 && C >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffll - 64)) {
    fail(GC_ERR_ARG, "pyramid score backward: bad n/C/H/W");
    return -1;
  }
  return (long long)pyramid_score_bwd_scratch_floats(n, C, H, W);
}

int gencomm_pyramid_score_bwd(const float* x, const float* weight, const float* occ, const int* rect, const float* d_occ, const float* d_score,
                              float* dx, float* dw, float* db, int n, int C, int H, int W, float* scratch, long long scratch_floats, void* stream) {
  GC_CHECK_ARG(x && weight && occ, "pyramid score backward: null pointer (x, weight, occ)");
  GC_CHECK_ARG(d_occ || d_score, "pyramid score backward: d_occ and d_score are both null");
  GC_CHECK_ARG(dx || dw, "pyramid score backward: nothing to compute (dx and dw are both null)");
  GC_CHECK_ARG((dw == nullptr) == (db == nullptr), "pyramid score backward: dw and db come together");
  const long long need = gencomm_pyramid_score_bwd_scratch_floats(n, C, H, W);
  if (need < 0) return GC_ERR_ARG;
  if (dw != nullptr && (scratch == nullptr || scratch_floats < need))
    return fail(GC_ERR_WORKSPACE, "pyramid score backward: scratch too small (gencomm_pyramid_score_bwd_scratch_floats)");
  PyrScoreBwdArgs a{x, weight, occ, rect, d_occ, d_score, dx, nullptr, C, H, W};
  return pyramid_score_bwd_enqueue(a, dw, db, scratch, n, (hipStream_t)stream);
}

long long gencomm_warp_weightfuse_bwd_scratch_floats(int n, int H, int W) {
  if (!(n >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffll - 128)) {
    fail(GC_ERR_ARG, "weighted fuse backward: bad n/H/W");
    return -1;
  }
  return (long long)warp_weightfuse_bwd_scratch_floats(n, H, W);
}

int gencomm_warp_weightfuse_bwd(const float* x, const float* score, const double* theta, const int* scene_off, const float* dout, float* dx,
                                float* dscore, float* scratch, long long scratch_floats, int B, int n, int C, int H, int W, void* stream) {
  GC_CHECK_ARG(x && score && theta && scene_off && dout && dx && dscore && scratch, "weighted fuse backward: null pointer");
  GC_CHECK_ARG(B >= 1 && B <= 65535 && n >= B && n <= 65535 && C >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffll - 128,
               "weighted fuse backward: bad B/n/C/H/W");
  if (scratch_floats < (long long)warp_weightfuse_bwd_scratch_floats(n, H, W))
    return fail(GC_ERR_WORKSPACE, "weighted fuse backward: scratch too small (gencomm_warp_weightfuse_bwd_scratch_floats)");
  WeightFuseBwdArgs a{x, score, theta, scene_off, dout, dx, dscore, nullptr, nullptr, C, H, W, 0};
  return warp_weightfuse_bwd_enqueue(a, scratch, B, n, (hipStream_t)stream);
}

}  // extern "C"
