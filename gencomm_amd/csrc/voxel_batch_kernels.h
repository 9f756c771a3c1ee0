// Batched lidar front end: the raw point clouds of all A agents of a call -> collated voxels, in one launch sequence.
// Per agent it restates the reference's dataset loop (intermediate_heter_fusion_dataset.py:443-471): shuffle_points (the
// permutation is an INPUT), mask_ego_points (pcd_utils.py:84-86: the closed box -1.95 <= x <= 2.95, -1.1 <= y <= 1.1 is removed,
// compared in float32), project_points_by_matrix_torch (box_utils.py:1169: both operands float32, x' = sum_k p_k * T[0][k] over
// (x, y, z, 1) -- torch's CPU matmul is a fused multiply-add chain in k order from a zero accumulator for more than 16 points),
// the voxeliser of voxel_kernels.h, and SpVoxelPreprocessor.collate_batch (agent index in front of (z, y, x), agents back to back).
//   1 key[i] = agent * ncells + cell of logical point i (sentinel A * ncells when masked / outside the grid), value[i] = i
//   2 ONE stable radix sort over the bits A * ncells needs (32-bit keys where the sentinel fits, 64-bit keys otherwise)
//   3 segment heads -> flag[first point of the cell]; every flag is written exactly once (the sorted values are a permutation),
//     so nothing is cleared per call. Exclusive scan of the flags over the points; an agent's points are a contiguous range of
//     logical indices, so its voxel number is scan[first point] - scan[offsets[agent]]: first appearance, segmented per agent.
//     Inclusive max-scan of the head positions = every element's segment start.
//   4 one wave scans min(voxels of agent, max_voxels) over the agents: counts, output bases, total -- no host read in between
//   5 the LAST element of every kept segment writes the voxel's row record, coordinates and point count (one writer, no atomics)
//   6 one thread per (output row, slot) copies its point (projected again, same arithmetic) or writes the zero padding: every
//     element of the rows [0, total) is written exactly once, coalesced, so no memset either. Rows >= total are left alone.
#pragma once
#include <rocprim/rocprim.hpp>

#include "common.h"
#include "voxel_kernels.h"

namespace gc {

struct VoxelBatchArgs {
  const float* points;   // [n][nfeat]
  const int* offsets;    // [A + 1] logical point ranges of the agents
  const float* tfm;      // [A][16] row-major 4x4, or null
  const int* perm;       // [n]: logical point i is input row perm[i]; or null
  int n, nfeat, A, mask_ego;
  float vs[3], r0[3];
  int grid[3];           // x, y, z cells
  unsigned long long ncells;
  int max_points, max_voxels, cap_rows;
};

__device__ __forceinline__ int vb_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// largest a in [0, A) with offsets[a] <= i (empty agents in front of i are skipped)
__device__ __forceinline__ int vb_agent_of(const int* __restrict__ off, int A, int i) {
  int lo = 0, hi = A - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// torch.einsum("ik,jk->ij", [x y z 1], T) in float32: acc = 0; acc = fma(p_k, T[j][k], acc) for k = 0..3
__device__ __forceinline__ void vb_project(const float* __restrict__ m, float& x, float& y, float& z) {
#pragma clang fp contract(off)
  const float px = x, py = y, pz = z;
  x = fmaf(pz, m[2], fmaf(py, m[1], fmaf(px, m[0], 0.f))) + m[3];
  y = fmaf(pz, m[6], fmaf(py, m[5], fmaf(px, m[4], 0.f))) + m[7];
  z = fmaf(pz, m[10], fmaf(py, m[9], fmaf(px, m[8], 0.f))) + m[11];
}

template <typename K, bool VEC4>
__global__ __launch_bounds__(256) void vb_key_kernel(const VoxelBatchArgs a, K* __restrict__ key, unsigned int* __restrict__ val) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const int agent = vb_agent_of(a.offsets, a.A, i);
  K k = (K)((unsigned long long)a.A * a.ncells);
  const int src = a.perm ? a.perm[i] : i;
  if ((unsigned)src < (unsigned)a.n) {
    float p[3];
    if (VEC4) {
      const float4 v = *reinterpret_cast<const float4*>(a.points + (size_t)src * 4);   // one 16-byte load per point row
      p[0] = v.x; p[1] = v.y; p[2] = v.z;
    } else {
      const float* __restrict__ s = a.points + (size_t)src * a.nfeat;
      p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
    }
    const bool ego = a.mask_ego && p[0] >= -1.95f && p[0] <= 2.95f && p[1] >= -1.1f && p[1] <= 1.1f;
    if (!ego) {
      if (a.tfm) vb_project(a.tfm + (size_t)agent * 16, p[0], p[1], p[2]);
      int c[3];
      bool ok = true;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float f = floorf((p[j] - a.r0[j]) / a.vs[j]);
        ok = ok && f >= 0.f && f < (float)a.grid[j];
        c[j] = (int)f;
      }
      if (ok) k = (K)((unsigned long long)agent * a.ncells + ((unsigned long long)c[2] * a.grid[1] + c[1]) * a.grid[0] + c[0]);
    }
  }
  key[i] = k;
  val[i] = (unsigned int)i;
}

// on the sorted arrays: head position (for the max-scan) and the first-appearance flag of EVERY point (flag has n + 1 entries)
template <typename K>
__global__ __launch_bounds__(256) void vb_head_kernel(int n, K sentinel, const K* __restrict__ skey, const unsigned int* __restrict__ sval,
                                                      int* __restrict__ headpos, int* __restrict__ flag) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const K k = skey[j];
  const bool head = k != sentinel && (j == 0 || skey[j - 1] != k);
  headpos[j] = head ? j : 0;
  flag[sval[j]] = head ? 1 : 0;
  if (j == 0) flag[n] = 0;
}

// counts[a] = min(voxels of agent a, max_voxels), base = exclusive scan of the counts, total: one wave, 64 agents per step
__global__ __launch_bounds__(64) void vb_agent_kernel(int A, int n, const int* __restrict__ offsets, const int* __restrict__ vid, int max_voxels,
                                                      int cap_rows, int* __restrict__ counts, int* __restrict__ base, int* __restrict__ total) {
  const int lane = threadIdx.x;
  int carry = 0;
  for (int a0 = 0; a0 < A; a0 += 64) {
    const int a = a0 + lane;
    int c = 0;
    if (a < A) {
      c = vid[vb_clamp(offsets[a + 1], 0, n)] - vid[vb_clamp(offsets[a], 0, n)];
      c = vb_clamp(c, 0, max_voxels);
    }
    int s = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(s, d, 64);
      if (lane >= d) s += t;
    }
    if (a < A) { counts[a] = c; base[a] = carry + s - c; }
    carry += __shfl(s, 63, 64);
  }
  if (lane == 0) *total = carry < cap_rows ? carry : cap_rows;
}

__global__ __launch_bounds__(64) void vb_empty_kernel(int A, int* __restrict__ counts, int* __restrict__ total) {
  for (int a = threadIdx.x; a < A; a += 64) counts[a] = 0;
  if (threadIdx.x == 0) *total = 0;
}

// the last element of a segment knows the segment's length: it alone writes the voxel's record
template <typename K>
__global__ __launch_bounds__(256) void vb_tail_kernel(const VoxelBatchArgs a, K sentinel, const K* __restrict__ skey, const unsigned int* __restrict__ sval,
                                                      const int* __restrict__ segstart, const int* __restrict__ vid, const int* __restrict__ base,
                                                      int4* __restrict__ rowinfo, int4* __restrict__ coords, int* __restrict__ num_points) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= a.n) return;
  const K k = skey[j];
  if (k == sentinel || (j + 1 < a.n && skey[j + 1] == k)) return;
  const int hp = segstart[j];
  const int agent = (int)(k / (K)a.ncells);
  const K cell = k - (K)agent * (K)a.ncells;
  const int v = vid[sval[hp]] - vid[vb_clamp(a.offsets[agent], 0, a.n)];
  if (v < 0 || v >= a.max_voxels) return;
  const int row = base[agent] + v;
  if (row >= a.cap_rows) return;
  const int len = j - hp + 1, kept = len < a.max_points ? len : a.max_points;
  const K gx = (K)a.grid[0], gy = (K)a.grid[1];
  coords[row] = make_int4(agent, (int)(cell / (gx * gy)), (int)((cell / gx) % gy), (int)(cell % gx));
  num_points[row] = kept;
  rowinfo[row] = make_int4(hp, kept, agent, 0);
}

template <bool VEC4>
__global__ __launch_bounds__(256) void vb_fill_kernel(const VoxelBatchArgs a, const unsigned int* __restrict__ sval, const int4* __restrict__ rowinfo,
                                                      const int* __restrict__ total, float* __restrict__ voxels) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int row = (int)(t / a.max_points), slot = (int)(t - (long long)row * a.max_points);
  if (row >= *total) return;
  const int4 info = rowinfo[row];
  float* __restrict__ dst = voxels + ((size_t)row * a.max_points + slot) * a.nfeat;
  int src = -1;
  if (slot < info.y && (unsigned)(info.x + slot) < (unsigned)a.n) {
    const unsigned int i = sval[info.x + slot];
    if (i < (unsigned)a.n) src = a.perm ? a.perm[i] : (int)i;
  }
  if ((unsigned)src >= (unsigned)a.n) {   // padding (or a record that inconsistent offsets left behind)
    if (VEC4) *reinterpret_cast<float4*>(dst) = make_float4(0.f, 0.f, 0.f, 0.f);
    else for (int f = 0; f < a.nfeat; ++f) dst[f] = 0.f;
    return;
  }
  const float* __restrict__ m = a.tfm ? a.tfm + (size_t)vb_clamp(info.z, 0, a.A - 1) * 16 : nullptr;
  if (VEC4) {
    float4 v = *reinterpret_cast<const float4*>(a.points + (size_t)src * 4);
    if (m) vb_project(m, v.x, v.y, v.z);
    *reinterpret_cast<float4*>(dst) = v;
  } else {
    const float* __restrict__ s = a.points + (size_t)src * a.nfeat;
    float x = s[0], y = s[1], z = s[2];
    if (m) vb_project(m, x, y, z);
    dst[0] = x; dst[1] = y; dst[2] = z;
    for (int f = 3; f < a.nfeat; ++f) dst[f] = s[f];
  }
}

struct VoxelBatchWs {
  size_t key, skey, val, sval, headpos, segstart, flag, vid, base, rowinfo, temp, temp_bytes, total;
};
// sized for 64-bit keys whatever the grid: the workspace query needs no grid
inline VoxelBatchWs voxel_batch_ws(int n, int A, int cap_rows) {
  VoxelBatchWs w{};
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off += align_up(bytes, 256); return o; };
  const size_t nn = (size_t)(n > 0 ? n : 1);
  w.key = take(nn * 8); w.skey = take(nn * 8); w.val = take(nn * 4); w.sval = take(nn * 4);
  w.headpos = take(nn * 4); w.segstart = take(nn * 4); w.flag = take((nn + 1) * 4); w.vid = take((nn + 1) * 4);
  w.base = take((size_t)(A > 0 ? A : 1) * 4);
  w.rowinfo = take((size_t)(cap_rows > 0 ? cap_rows : 1) * sizeof(int4));
  size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t1, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, nn, 0, 32, (hipStream_t)0);
  (void)rocprim::radix_sort_pairs(nullptr, t4, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned int*)nullptr, (unsigned int*)nullptr, nn, 0, 64, (hipStream_t)0);
  (void)rocprim::exclusive_scan(nullptr, t2, (int*)nullptr, (int*)nullptr, 0, nn + 1, rocprim::plus<int>(), (hipStream_t)0);
  (void)rocprim::inclusive_scan(nullptr, t3, (int*)nullptr, (int*)nullptr, nn, MaxOp(), (hipStream_t)0);
  w.temp_bytes = std::max(std::max(t1, t4), std::max(t2, t3)) + 256;
  w.temp = take(w.temp_bytes);
  w.total = off;
  return w;
}

template <typename K>
inline int voxelize_batch_enqueue_k(const VoxelBatchArgs& a, bool vec4, int key_bits, float* voxels, int* coords, int* num_points, int* counts, int* total,
                                    char* wsp, hipStream_t st) {
  const VoxelBatchWs w = voxel_batch_ws(a.n, a.A, a.cap_rows);
  auto U = [&](size_t o) { return reinterpret_cast<unsigned int*>(wsp + o); };
  auto I = [&](size_t o) { return reinterpret_cast<int*>(wsp + o); };
  K* key = reinterpret_cast<K*>(wsp + w.key);
  K* skey = reinterpret_cast<K*>(wsp + w.skey);
  int4* rowinfo = reinterpret_cast<int4*>(wsp + w.rowinfo);
  const K sentinel = (K)((unsigned long long)a.A * a.ncells);
  const int nb = (a.n + 255) / 256;
  if (vec4) vb_key_kernel<K, true><<<nb, 256, 0, st>>>(a, key, U(w.val));
  else vb_key_kernel<K, false><<<nb, 256, 0, st>>>(a, key, U(w.val));
  size_t tb = w.temp_bytes;
  GC_HIP(rocprim::radix_sort_pairs(wsp + w.temp, tb, key, skey, U(w.val), U(w.sval), (size_t)a.n, 0, (unsigned)key_bits, st));
  vb_head_kernel<K><<<nb, 256, 0, st>>>(a.n, sentinel, skey, U(w.sval), I(w.headpos), I(w.flag));
  tb = w.temp_bytes;
  GC_HIP(rocprim::inclusive_scan(wsp + w.temp, tb, I(w.headpos), I(w.segstart), (size_t)a.n, MaxOp(), st));
  tb = w.temp_bytes;
  GC_HIP(rocprim::exclusive_scan(wsp + w.temp, tb, I(w.flag), I(w.vid), 0, (size_t)a.n + 1, rocprim::plus<int>(), st));
  vb_agent_kernel<<<1, 64, 0, st>>>(a.A, a.n, a.offsets, I(w.vid), a.max_voxels, a.cap_rows, counts, I(w.base), total);
  vb_tail_kernel<K><<<nb, 256, 0, st>>>(a, sentinel, skey, U(w.sval), I(w.segstart), I(w.vid), I(w.base), rowinfo, reinterpret_cast<int4*>(coords), num_points);
  const long long slots = (long long)a.cap_rows * a.max_points;
  if (slots > 0) {
    const unsigned fb = (unsigned)((slots + 255) / 256);
    if (vec4) vb_fill_kernel<true><<<fb, 256, 0, st>>>(a, U(w.sval), rowinfo, total, voxels);
    else vb_fill_kernel<false><<<fb, 256, 0, st>>>(a, U(w.sval), rowinfo, total, voxels);
  }
  GC_HIP(hipGetLastError());
  return GC_OK;
}

inline int voxelize_batch_enqueue(const VoxelBatchArgs& a, bool vec4, float* voxels, int* coords, int* num_points, int* counts, int* total, char* wsp,
                                  hipStream_t st) {
  if (a.n == 0 || a.cap_rows == 0) {
    vb_empty_kernel<<<1, 64, 0, st>>>(a.A, counts, total);
    GC_HIP(hipGetLastError());
    return GC_OK;
  }
  const unsigned long long sentinel = (unsigned long long)a.A * a.ncells;
  int bits = 1;
  while (bits < 64 && (sentinel >> bits) != 0) ++bits;
  if (sentinel <= 0xFFFFFFFFull) return voxelize_batch_enqueue_k<unsigned int>(a, vec4, bits, voxels, coords, num_points, counts, total, wsp, st);
  return voxelize_batch_enqueue_k<unsigned long long>(a, vec4, bits, voxels, coords, num_points, counts, total, wsp, st);
}

}  // namespace gc
