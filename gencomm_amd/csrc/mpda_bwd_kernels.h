// Training kernels of MPDA's feature aligner (mpda_kernels.h has the inference pair; DESIGN.md 4.11 "Training").
//   quad_attn_train_kernel  quad_attn_kernel plus an optional dropout on the 4 x 4 probabilities (the reference's Attention.attend is
//                           Softmax -> Dropout): keep [N][heads][X Y] holds one uint16 per group, bit 4 i + j set = probability (query
//                           token i, key token j) survives and is multiplied by keep_scale = 1 / (1 - p).  keep == NULL runs the
//                           inference kernel's arithmetic, instruction for instruction; so does an all-ones mask at keep_scale 1
//                           (p * 1.0f == p).  No log-sum-exp is saved.
//   quad_attn_bwd_kernel    the adjoint.  The forward's layout: a lane owns one group of one (map, head), four waves split the head's
//                           channels.  Pass 1 walks the wave's DH / 4 channels of q, k, v and dout once into TWO partial 4 x 4
//                           matrices per lane, S = q k^T and dPd = dout v^T; both meet in 32 KB of LDS ([2][4 waves][16][64 lanes])
//                           and every wave adds the four partials in the same order.  Registers then hold P = softmax(scale S +
//                           bias), Pd = P o M and dS = P o (dP - rowsum(P o dP)) with dP = dPd o M.  Pass 2 walks the wave's channels
//                           of q, k and dout a SECOND time (v is read once) and stores dq = scale dS k, dk = scale dS^T q,
//                           dv = Pd^T dout, each element exactly once.  The table's gradient: wave 0 (the four waves hold the same
//                           dS) bins its lane's 16 entries into the 9 relative positions, a fixed butterfly sums the 64 lanes, lane
//                           0 writes the workgroup's 9 partials; quad_dbias_reduce_kernel adds the partials of all workgroups in a
//                           fixed order.  Nkv == 1 (one ego map for N query maps): each map writes its dk / dv to a scratch slab
//                           [N][inner][H][W] and quad_kv_reduce_kernel adds the N slabs in map order.  No float atomics anywhere.
//   resize_bilinear_bwd_kernel  the adjoint of resize_bilinear_kernel as a GATHER: a thread owns one source pixel.  The lower source
//                           index of resize_source() is monotone in the output index, so the outputs that read source row (column)
//                           i as lower or as (clamped) upper neighbour are the contiguous range [lo(i - 1), lo(i + 1)), lo(i) = the
//                           first output index whose lower index is >= i, found from a float estimate corrected with resize_source()
//                           itself.  The weights come from resize_source(): the forward's own floats.  A zero weight drops its term
//                           and the first term initialises the sum, so a same-size call returns dy's bits.
//   leaky_relu_{fwd,bwd}_kernel  elementwise; the backward reads the sign from the OUTPUT (y > 0 <=> x > 0 for a positive slope).
#pragma once
#include "common.h"
#include "mpda_kernels.h"

namespace gc {

#pragma clang fp contract(off)

struct QuadTrainArgs {
  QuadArgs f;
  const unsigned short* keep;   // [N][heads][X Y] or NULL
  float keep_scale;
};

template <int DH, int MODE>
__global__ __launch_bounds__(256) void quad_attn_train_kernel(const QuadTrainArgs ta) {
  const QuadArgs& a = ta.f;
  constexpr int DQ = DH / 4;
  constexpr int CH = MODE ? 4 : (DQ < 8 ? DQ : 8);
  __shared__ float part[4][16][kQuadGroups];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int X = a.H >> 1, Y = a.W >> 1, G = X * Y;
  const int graw = blockIdx.x * kQuadGroups + lane;
  const bool live = graw < G;
  const int g = live ? graw : G - 1;
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
  for (int d0 = 0; d0 < DQ; d0 += CH, qb += CH * HW, kb += CH * HW) {
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
#pragma unroll
  for (int e = 0; e < 16; ++e) s[e >> 2][e & 3] = ((part[0][e][lane] + part[1][e][lane]) + part[2][e][lane]) + part[3][e][lane];
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
  if (ta.keep != nullptr) {   // dropout on the probabilities: bit 4 i + j of the group's word
    const unsigned kw = ta.keep[((size_t)n * a.heads + m) * G + g];
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e >> 2][e & 3] = ((kw >> e) & 1u) ? s[e >> 2][e & 3] * ta.keep_scale : 0.f;
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
inline int quad_attn_train_launch(const QuadTrainArgs& a, int N, hipStream_t st) {
  const int groups = (a.f.H / 2) * (a.f.W / 2);
  const dim3 grid((groups + kQuadGroups - 1) / kQuadGroups, a.f.heads, N);
  GC_KLOG(a.f.grid_mode ? "quad_attn_train_kernel<grid>" : "quad_attn_train_kernel<window>");
  if (a.f.grid_mode) quad_attn_train_kernel<DH, 1><<<grid, 256, 0, st>>>(a);
  else quad_attn_train_kernel<DH, 0><<<grid, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

struct QuadBwdArgs {
  const float* q;      // as QuadArgs
  const float* k;
  const float* v;
  const float* bias;   // [9][heads] or NULL
  const float* dout;   // [N][heads * DH][H][W]
  const unsigned short* keep;
  float* dq;           // [N][q_ct][H][W] at the first query channel
  float* dk;           // map n of dk / dv is dk + n dkv_ct H W: the caller's [N][kv_ct] tensor, or the scratch slabs [N][inner] (Nkv == 1 < N)
  float* dv;
  float* dbias_part;   // [N gridDim.x][heads][9] or NULL
  int heads, H, W, q_ct, kv_ct, dkv_ct, grid_mode, kv_bcast;
  float scale, keep_scale;
};

template <int DH, int MODE>
__global__ __launch_bounds__(256) void quad_attn_bwd_kernel(const QuadBwdArgs a) {
  constexpr int DQ = DH / 4;
  constexpr int CH = MODE ? 2 : (DQ < 4 ? DQ : 4);   // four tensors in pass 1: half the forward's step, the same floats in flight
  static_assert(DH % 4 == 0 && DQ % CH == 0, "four waves share a head; the channel loops walk CH channels at a time");
  __shared__ float part[2][4][16][kQuadGroups];   // [S | dPd][wave][i * 4 + j][lane]: 32 KB
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int X = a.H >> 1, Y = a.W >> 1, G = X * Y;
  const int graw = blockIdx.x * kQuadGroups + lane;
  const bool live = graw < G;
  const int g = live ? graw : G - 1;   // a lane beyond the last group repeats it: loads in bounds, contributes 0, stores nothing
  const int gx = g / Y, gy = g - gx * Y, m = blockIdx.y, n = blockIdx.z, nkv = a.kv_bcast ? 0 : n;
  const size_t HW = (size_t)a.H * a.W;
  const QuadTokens<MODE> tok(gx, gy, X, Y, a.W);
  const size_t qoff = ((size_t)n * a.q_ct + (size_t)m * DH + wave * DQ) * HW;
  const size_t koff = ((size_t)nkv * a.kv_ct + (size_t)m * DH + wave * DQ) * HW;
  const size_t ooff = (((size_t)n * a.heads + m) * DH + wave * DQ) * HW;
  const size_t dkoff = ((size_t)n * a.dkv_ct + (size_t)m * DH + wave * DQ) * HW;

  float s[4][4], t[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] = 0.f, t[i][j] = 0.f;
  {
    const float* __restrict__ qb = a.q + qoff;
    const float* __restrict__ kb = a.k + koff;
    const float* __restrict__ vb = a.v + koff;
    const float* __restrict__ gb = a.dout + ooff;
#pragma unroll 1
    for (int d0 = 0; d0 < DQ; d0 += CH, qb += CH * HW, kb += CH * HW, vb += CH * HW, gb += CH * HW) {
#pragma unroll
      for (int d = 0; d < CH; ++d) {
        float qd[4], kd[4], vd[4], gd[4];
        tok.load(qb + d * HW, qd);
        tok.load(kb + d * HW, kd);
        tok.load(vb + d * HW, vd);
        tok.load(gb + d * HW, gd);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s[i][j] = fmaf(qd[i], kd[j], s[i][j]);
            t[i][j] = fmaf(gd[i], vd[j], t[i][j]);
          }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    part[0][wave][e][lane] = s[e >> 2][e & 3];
    part[1][wave][e][lane] = t[e >> 2][e & 3];
  }
  __syncthreads();
  // every wave sums the four partials in the same order: the four waves hold the same S and dPd, bit for bit
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    s[e >> 2][e & 3] = ((part[0][0][e][lane] + part[0][1][e][lane]) + part[0][2][e][lane]) + part[0][3][e][lane];
    t[e >> 2][e & 3] = ((part[1][0][e][lane] + part[1][1][e][lane]) + part[1][2][e][lane]) + part[1][3][e][lane];
  }
  float bt[9];
#pragma unroll
  for (int r = 0; r < 9; ++r) bt[r] = a.bias != nullptr ? a.bias[r * a.heads + m] : 0.f;
  unsigned kw = 0xffffu;
  float ks = 1.0f;
  if (a.keep != nullptr) { kw = a.keep[((size_t)n * a.heads + m) * G + g]; ks = a.keep_scale; }
  // s becomes scale dS, t becomes Pd
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] = fmaf(s[i][j], a.scale, bt[((i >> 1) - (j >> 1) + 1) * 3 + ((i & 1) - (j & 1) + 1)]);
    const float mx = fmaxf(fmaxf(s[i][0], s[i][1]), fmaxf(s[i][2], s[i][3]));
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { s[i][j] = expf(s[i][j] - mx); den += s[i][j]; }
    const float rden = 1.0f / den;
    float dp[4], rs = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p = s[i][j] * rden;
      const bool kept = (kw >> (4 * i + j)) & 1u;
      dp[j] = kept ? t[i][j] * ks : 0.f;   // dP = dPd o M
      t[i][j] = kept ? p * ks : 0.f;        // Pd = P o M
      s[i][j] = p;
      rs = fmaf(p, dp[j], rs);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] = s[i][j] * (dp[j] - rs);   // dS
  }
  if (a.dbias_part != nullptr && wave == 0) {   // wave-uniform branch: all 64 lanes take the butterfly
    float bin[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) bin[r] = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) bin[((i >> 1) - (j >> 1) + 1) * 3 + ((i & 1) - (j & 1) + 1)] += live ? s[i][j] : 0.f;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) bin[r] += __shfl_xor(bin[r], off, 64);
    }
    if (lane == 0) {
      float* __restrict__ dst = a.dbias_part + (((size_t)n * gridDim.x + blockIdx.x) * a.heads + m) * 9;
#pragma unroll
      for (int r = 0; r < 9; ++r) dst[r] = bin[r];
    }
  }
  if (!live) return;   // no barrier follows
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) s[i][j] *= a.scale;
  {
    const float* __restrict__ qb = a.q + qoff;
    const float* __restrict__ kb = a.k + koff;
    const float* __restrict__ gb = a.dout + ooff;
    float* __restrict__ dqb = a.dq + qoff;
    float* __restrict__ dkb = a.dk + dkoff;
    float* __restrict__ dvb = a.dv + dkoff;
#pragma unroll 1
    for (int d0 = 0; d0 < DQ; d0 += CH, qb += CH * HW, kb += CH * HW, gb += CH * HW, dqb += CH * HW, dkb += CH * HW, dvb += CH * HW) {
#pragma unroll
      for (int d = 0; d < CH; ++d) {
        float qd[4], kd[4], gd[4], o[4];
        tok.load(qb + d * HW, qd);
        tok.load(kb + d * HW, kd);
        tok.load(gb + d * HW, gd);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = fmaf(s[i][3], kd[3], fmaf(s[i][2], kd[2], fmaf(s[i][1], kd[1], s[i][0] * kd[0])));
        tok.store(dqb + d * HW, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(s[3][j], qd[3], fmaf(s[2][j], qd[2], fmaf(s[1][j], qd[1], s[0][j] * qd[0])));
        tok.store(dkb + d * HW, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = fmaf(t[3][j], gd[3], fmaf(t[2][j], gd[2], fmaf(t[1][j], gd[1], t[0][j] * gd[0])));
        tok.store(dvb + d * HW, o);
      }
    }
  }
}

// dbias[r][m] = sum over the P workgroup partials part[p][m][r], one wave per (r, m): lane l adds p = l, l + 64, ... in order, then the
// same butterfly.  grid (9, heads), 64 threads.
__global__ __launch_bounds__(64) void quad_dbias_reduce_kernel(const float* __restrict__ part, float* __restrict__ dbias, int P, int heads) {
  const int r = blockIdx.x, m = blockIdx.y, lane = threadIdx.x;
  float acc = 0.f;
  for (int p = lane; p < P; p += 64) acc += part[((size_t)p * heads + m) * 9 + r];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if (lane == 0) dbias[r * heads + m] = acc;
}

// dk | dv of the one shared key / value map = the N per-map slabs added in map order.  slabs [2][N][count], dst0 / dst1 [count].
__global__ __launch_bounds__(256) void quad_kv_reduce_kernel(const float* __restrict__ slabs, float* __restrict__ dst0, float* __restrict__ dst1, int N,
                                                             long long count) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const float* __restrict__ src = slabs + (size_t)blockIdx.y * N * count + i;
  float acc = src[0];
  for (int n = 1; n < N; ++n) acc += src[(size_t)n * count];
  (blockIdx.y ? dst1 : dst0)[i] = acc;
}

template <int DH>
inline int quad_attn_bwd_launch(const QuadBwdArgs& a, int N, hipStream_t st) {
  const int groups = (a.H / 2) * (a.W / 2);
  const dim3 grid((groups + kQuadGroups - 1) / kQuadGroups, a.heads, N);
  GC_KLOG(a.grid_mode ? "quad_attn_bwd_kernel<grid>" : "quad_attn_bwd_kernel<window>");
  if (a.grid_mode) quad_attn_bwd_kernel<DH, 1><<<grid, 256, 0, st>>>(a);
  else quad_attn_bwd_kernel<DH, 0><<<grid, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

// lo(i): the first output index whose lower source index is >= i (0 for i <= 0, `out` for i >= in); the float estimate is corrected
// with resize_source() itself, so the ranges are exact for the forward's own rounding
__device__ __forceinline__ int resize_first_output(int i, float scale, int in, int out) {
  if (i <= 0) return 0;
  if (i >= in) return out;
  int o = (int)ceilf(((float)i + 0.5f) / scale - 0.5f);
  o = max(0, min(o, out));
  int i0, i1;
  float l1;
  while (o > 0) {
    resize_source(o - 1, scale, in, i0, i1, l1);
    if (i0 < i) break;
    --o;
  }
  while (o < out) {
    resize_source(o, scale, in, i0, i1, l1);
    if (i0 >= i) break;
    ++o;
  }
  return o;
}

// weight of source index i in output index o: (1 - l1) as the lower neighbour plus l1 as the upper one (both where the upper is clamped)
__device__ __forceinline__ float resize_weight(int o, int i, float scale, int in) {
  int i0, i1;
  float l1;
  resize_source(o, scale, in, i0, i1, l1);
  float w = 0.f;
  if (i0 == i) w = 1.0f - l1;
  if (i1 == i && l1 != 0.f) w += l1;
  return w;
}

struct ResizeBwdArgs {
  const float* dy;   // [NC][Ho][Wo]
  float* dx;         // [NC][Hi][Wi]
  int Hi, Wi, Ho, Wo;
  long long planes;
  float sh, sw;
};

__global__ __launch_bounds__(256) void resize_bilinear_bwd_kernel(const ResizeBwdArgs a) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= a.Hi * a.Wi) return;
  const int iy = p / a.Wi, ix = p - iy * a.Wi;
  const int oy0 = resize_first_output(iy - 1, a.sh, a.Hi, a.Ho), oy1 = resize_first_output(iy + 1, a.sh, a.Hi, a.Ho);
  const int ox0 = resize_first_output(ix - 1, a.sw, a.Wi, a.Wo), ox1 = resize_first_output(ix + 1, a.sw, a.Wi, a.Wo);
  const size_t iplane = (size_t)a.Hi * a.Wi, oplane = (size_t)a.Ho * a.Wo;
  for (long long c = blockIdx.y; c < a.planes; c += gridDim.y) {
    const float* __restrict__ g = a.dy + (size_t)c * oplane;
    float acc = 0.f;
    bool have = false;
    for (int oy = oy0; oy < oy1; ++oy) {
      const float wy = resize_weight(oy, iy, a.sh, a.Hi);
      if (wy == 0.f) continue;
      float row = 0.f;
      bool rhave = false;
      for (int ox = ox0; ox < ox1; ++ox) {
        const float wx = resize_weight(ox, ix, a.sw, a.Wi);
        if (wx == 0.f) continue;
        const float term = wx * g[(size_t)oy * a.Wo + ox];
        row = rhave ? row + term : term;
        rhave = true;
      }
      if (!rhave) continue;
      const float term = wy * row;
      acc = have ? acc + term : term;
      have = true;
    }
    a.dx[(size_t)c * iplane + p] = acc;
  }
}

inline int resize_bilinear_bwd_enqueue(ResizeBwdArgs a, hipStream_t st) {
  a.sh = (float)a.Hi / (float)a.Ho;   // the forward's scales
  a.sw = (float)a.Wi / (float)a.Wo;
  // a thread finds its four range ends once and then walks planes: about 4096 workgroups in all, so the index arithmetic is shared by
  // several planes where there are many (the shipped 64 x 128 map: 32 pixel blocks x 128 plane slots)
  const long long bx = (a.Hi * a.Wi + 255) / 256;
  const long long by = std::max<long long>(1, std::min<long long>(a.planes, std::min<long long>(65535, 4096 / bx)));
  const dim3 grid((unsigned)bx, (unsigned)by);
  GC_KLOG("resize_bilinear_bwd_kernel");
  resize_bilinear_bwd_kernel<<<grid, 256, 0, st>>>(a);
  GC_HIP(hipGetLastError());
  return GC_OK;
}

__global__ __launch_bounds__(256) void leaky_relu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, float slope) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float v = x[i];
    y[i] = v > 0.f ? v : v * slope;
  }
}

__global__ __launch_bounds__(256) void leaky_relu_bwd_kernel(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx, long long n,
                                                             float slope) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float g = dy[i];
    dx[i] = y[i] > 0.f ? g : g * slope;
  }
}

#pragma clang fp contract(fast)

}  // namespace gc
