// MPDA's feature aligner (reference: opencood/models/mpda_modules/wg_fusion_modules.py + resizer.py) -- the two kernels the library
// lacked; every LayerNorm, Linear and 3x3 layer around them runs on kernels it already has (ln_nchw, the implicit-GEMM convolution
// with act 4 = LeakyReLU(0.01) for resizer.py's residual_block).
//   quad_attn_kernel        attention inside 2 x 2 groups of an NCHW map: per query map n, head m and group (x, y) the 4 x 4 matrix
//                           softmax(dim_head^-0.5 q k^T + bias) v over the group's four tokens.  Both of MPDA's attentions are this:
//                             cross  CrossAttention (wg_fusion_modules.py:12-97): q from the collaborator's map, k / v from the ego's
//                                    (Nkv = 1: ONE ego map serves every query map, where the reference repeats it n times), no bias
//                             self   Attention (:101-174) at window_size 2: q | k | v are channel blocks of one to_qkv output, the bias
//                                    is rel_pos_bias [9][heads] at rel = (hi - hj + 1) 3 + (wi - wj + 1), the module's rel_pos_indices
//                           Partitions are index arithmetic on the maps (X = H / 2, Y = W / 2), token t = 2 w1 + w2:
//                             window (grid_mode 0)  token (w1, w2) of group (x, y) = pixel (2 x + w1, 2 y + w2)    '(x w1) (y w2)'
//                             grid   (grid_mode 1)  token (w1, w2) of group (x, y) = pixel (w1 X + x, w2 Y + y)    '(w1 x) (w2 y)'
//   resize_bilinear_kernel  F.interpolate(mode='bilinear', align_corners=False) to a given size, torch's CPU arithmetic: source
//                           coordinate max((o + 0.5) in / out - 0.5, 0) in fp32, upper neighbour clamped to the last row / column,
//                           columns interpolated first inside each of the two rows, then the rows; a weight of exactly 0 drops its
//                           term, so a resize to the input's own size returns the input's bits.
//
// quad_attn_kernel is VALU work on a bandwidth-bound pass: 16 scores per head and group, no matrix cores.  A LANE owns one group
// of one (head, map); consecutive lanes own consecutive groups along y, so a wave reads runs of consecutive pixels in both
// partitions -- window mode as one 8-byte load per lane for the pixel pair (2 y, 2 y + 1) of each of the two rows (512-byte runs),
// grid mode as four 4-byte loads per lane (256-byte runs at columns y and Y + y).  A workgroup is 64 groups x FOUR waves, each wave
// taking a quarter of the head's channels: pass 1 walks the wave's DH / 4 channels of q and k once into 16 partial scores per lane,
// the partials meet in 16 KB of LDS, every wave adds the four in the same order (so the four hold the same scores), the softmax
// stays in registers, and pass 2 walks the wave's DH / 4 channels of v once and stores each output pixel as it is complete.
// Nothing is held across the passes but the 16 probabilities: v is read in pass 2 only (READ ONCE, not kept in registers), so
// every input element is loaded once and every output element is stored exactly once.  The first form of this kernel gave a lane
// all DH channels: at the shipped shape with one collaborator that is 2 waves per CU walking 8 dependent steps, 33 us for 67 MB
// (2.0 TB/s); four waves per group cut the dependent steps to 2 (DESIGN.md 4.11 has both measurements).  The channel loops walk
// up to 8 (window) or 4 (grid) channels per step: up to 64 or 32 floats per lane in flight in pass 1, half that in pass 2.
// Compiler report for gfx950 (-O3) at dim_head 32: window mode 69 VGPRs, grid mode 78 VGPRs (68 / 68 at dim_head 16, 73 / 78 at 64),
// no scratch, 0 / 25 SGPRs spilled to VGPR lanes (the wave-uniform plane bases), 16 KB of LDS per workgroup: 6 - 7 waves per SIMD.
#pragma once
#include "common.h"

namespace gc {

// Contraction is off in this header, as in swap_attn_kernels.h: only the explicit fmaf below fuse.
#pragma clang fp contract(off)

struct QuadArgs {
  const float* q;      // [N][q_ct][H][W], the pointer at the first query channel (head-major: channel m * DH + d)
  const float* k;      // [Nkv][kv_ct][H][W], at the first key channel
  const float* v;      // [Nkv][kv_ct][H][W], at the first value channel
  const float* bias;   // [9][heads] or NULL
  float* out;          // [N][heads * DH][H][W]
  int heads, H, W, q_ct, kv_ct, grid_mode, kv_bcast;   // kv_bcast: Nkv == 1, one key / value map for every query map
  float scale;
};

template <int MODE>
struct QuadTokens {
  int p0, s1, s2;   // window: p0 = pixel of token 0, s1 = W; grid: p0 = pixel of token 0, s1 = X W (w1 step), s2 = Y (w2 step)
  __device__ __forceinline__ QuadTokens(int gx, int gy, int X, int Y, int W) {
    if (MODE == 0) { p0 = 2 * gx * W + 2 * gy; s1 = W; s2 = 1; }
    else { p0 = gx * W + gy; s1 = X * W; s2 = Y; }
  }
  // the four tokens of one channel plane (W is even and the plane base 8-byte aligned: the window pair is one aligned float2)
  __device__ __forceinline__ void load(const float* __restrict__ plane, float (&t)[4]) const {
    if (MODE == 0) {
      const float2 a = *reinterpret_cast<const float2*>(plane + p0), b = *reinterpret_cast<const float2*>(plane + p0 + s1);
      t[0] = a.x, t[1] = a.y, t[2] = b.x, t[3] = b.y;
    } else {
      t[0] = plane[p0], t[1] = plane[p0 + s2], t[2] = plane[p0 + s1], t[3] = plane[p0 + s1 + s2];
    }
  }
  __device__ __forceinline__ void store(float* __restrict__ plane, const float (&t)[4]) const {
    if (MODE == 0) {
      *reinterpret_cast<float2*>(plane + p0) = make_float2(t[0], t[1]);
      *reinterpret_cast<float2*>(plane + p0 + s1) = make_float2(t[2], t[3]);
    } else {
      plane[p0] = t[0], plane[p0 + s2] = t[1], plane[p0 + s1] = t[2], plane[p0 + s1 + s2] = t[3];
    }
  }
};

constexpr int kQuadGroups = 64;   // groups per workgroup: one per lane; the workgroup's four waves split the head's channels

template <int DH, int MODE>
__global__ __launch_bounds__(256) void quad_attn_kernel(const QuadArgs a) {
  constexpr int DQ = DH / 4;   // channels of this wave
  // channels per step of the two channel loops.  Every load is a wave-uniform base (channel, token) in SGPRs plus the lane's pixel offset:
  // grid mode has four bases per channel and tensor, and 8 channels of q and k (128 SGPRs of bases) spilled 287 SGPRs; 4 fit
  constexpr int CH = MODE ? 4 : (DQ < 8 ? DQ : 8);
  static_assert(DH % 4 == 0 && DQ % CH == 0, "four waves share a head; the channel loops walk CH channels at a time");
  __shared__ float part[4][16][kQuadGroups];   // each wave's partial scores, [wave][i * 4 + j][lane]: consecutive lanes, consecutive banks
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: the plane bases stay in SGPRs
  const int X = a.H >> 1, Y = a.W >> 1, G = X * Y;
  const int graw = blockIdx.x * kQuadGroups + lane;
  const bool live = graw < G;
  const int g = live ? graw : G - 1;   // a lane beyond the last group repeats it (loads in bounds, no store) and meets the barrier
  const int gx = g / Y, gy = g - gx * Y, m = blockIdx.y, n = blockIdx.z, nkv = a.kv_bcast ? 0 : n;
  const size_t HW = (size_t)a.H * a.W;
  const QuadTokens<MODE> tok(gx, gy, X, Y, a.W);
  const float* __restrict__ qb = a.q + ((size_t)n * a.q_ct + (size_t)m * DH + wave * DQ) * HW;
  const float* __restrict__ kb = a.k + ((size_t)nkv * a.kv_ct + (size_t)m * DH + wave * DQ) * HW;
  const float* __restrict__ vb = a.v + ((size_t)nkv * a.kv_ct + (size_t)m * DH + wave * DQ) * HW;
  float* __restrict__ ob = a.out + (((size_t)n * a.heads + m) * DH + wave * DQ) * HW;

  float s[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] = 0.f;
#pragma unroll 1
  for (int d0 = 0; d0 < DQ; d0 += CH, qb += CH * HW, kb += CH * HW) {   // 8 CH floats per lane in flight; the bases advance
#pragma unroll
    for (int d = 0; d < CH; ++d) {
      float qd[4], kd[4];
      tok.load(qb + d * HW, qd);
      tok.load(kb + d * HW, kd);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[i][j] = fmaf(qd[i], kd[j], s[i][j]);
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) part[wave][e][lane] = s[e >> 2][e & 3];
  __syncthreads();
  // every wave sums the four partials in the same order: the four waves of a group hold the same scores, bit for bit
#pragma unroll
  for (int e = 0; e < 16; ++e) s[e >> 2][e & 3] = ((part[0][e][lane] + part[1][e][lane]) + part[2][e][lane]) + part[3][e][lane];
  // token t = (t >> 1, t & 1): rel(i, j) = (hi - hj + 1) 3 + (wi - wj + 1)
  float bt[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) bt[r] = a.bias != nullptr ? a.bias[r * a.heads + m] : 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] = fmaf(s[i][j], a.scale, bt[((i >> 1) - (j >> 1) + 1) * 3 + ((i & 1) - (j & 1) + 1)]);
    const float mx = fmaxf(fmaxf(s[i][0], s[i][1]), fmaxf(s[i][2], s[i][3]));
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[i][j] = expf(s[i][j] - mx); den += s[i][j]; }
    const float rden = 1.0f / den;
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] *= rden;
  }
  if (!live) return;   // no barrier follows
#pragma unroll 1
  for (int d0 = 0; d0 < DQ; d0 += CH, vb += CH * HW, ob += CH * HW) {
#pragma unroll
    for (int d = 0; d < CH; ++d) {
      float vd[4], o[4];
      tok.load(vb + d * HW, vd);
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = fmaf(s[i][3], vd[3], fmaf(s[i][2], vd[2], fmaf(s[i][1], vd[1], s[i][0] * vd[0])));
      tok.store(ob + d * HW, o);
    }
  }
}

template <int DH>
inline int quad_attn_launch(const QuadArgs& a, int N, hipStream_t st) {
  const int groups = (a.H / 2) * (a.W / 2);
  const dim3 grid((groups + kQuadGroups - 1) / kQuadGroups, a.heads, N);
  GC_KLOG(a.grid_mode ? "quad_attn_kernel<grid>" : "quad_attn_kernel<window>");
  if (a.grid_mode) quad_attn_kernel<DH, 1><<<grid, 256, 0, st>>>(a);
  else quad_attn_kernel<DH, 0><<<grid, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

struct ResizeArgs {
  const float* x;   // [NC][Hi][Wi]
  float* y;         // [NC][Ho][Wo]
  int Hi, Wi, Ho, Wo;
  long long planes;
  float sh, sw;     // (float)Hi / Ho, (float)Wi / Wo
};

// source index and upper weight of output index o (torch's area_pixel_compute_source_index + guard_index_and_lambda)
__device__ __forceinline__ void resize_source(int o, float scale, int in, int& i0, int& i1, float& l1) {
  const float src = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.f);
  i0 = min((int)src, in - 1);
  i1 = min(i0 + 1, in - 1);
  l1 = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

__global__ __launch_bounds__(256) void resize_bilinear_kernel(const ResizeArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.Ho * a.Wo) return;
  const int oy = p / a.Wo, ox = p - oy * a.Wo;
  int y0, y1, x0, x1;
  float ly, lx;
  resize_source(oy, a.sh, a.Hi, y0, y1, ly);
  resize_source(ox, a.sw, a.Wi, x0, x1, lx);
  const float my = 1.0f - ly, mx = 1.0f - lx;
  const size_t iplane = (size_t)a.Hi * a.Wi, oplane = (size_t)a.Ho * a.Wo;
  for (long long c = blockIdx.y; c < a.planes; c += gridDim.y) {
    const float* __restrict__ xp = a.x + (size_t)c * iplane;
    const float* __restrict__ r0 = xp + (size_t)y0 * a.Wi;
    const float* __restrict__ r1 = xp + (size_t)y1 * a.Wi;
    const float top = lx == 0.f ? r0[x0] : mx * r0[x0] + lx * r0[x1];
    float v = top;
    if (ly != 0.f) {
      const float bot = lx == 0.f ? r1[x0] : mx * r1[x0] + lx * r1[x1];
      v = my * top + ly * bot;
    }
    a.y[(size_t)c * oplane + p] = v;
  }
}

inline int resize_bilinear_enqueue(ResizeArgs a, hipStream_t st) {
  a.sh = (float)a.Hi / (float)a.Ho;
  a.sw = (float)a.Wi / (float)a.Wo;
  const dim3 grid((a.Ho * a.Wo + 255) / 256, (unsigned)(a.planes < 65535 ? a.planes : 65535));
  GC_KLOG("resize_bilinear_kernel");
  resize_bilinear_kernel<<<grid, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

#pragma clang fp contract(fast)

}  // namespace gc
