// Field-weighted FM (Pan et al., WWW 2018) for MI355X/gfx950: one latent
// table V[F, K] as in FM, and one learned scalar per pair of fields,
// R[nf, nf], of which only a <= b is used: Rs[a,b] = R[min(a,b), max(a,b)].
//
//   S_a[k] = sum_{j: a_j = a} V[f_j,k] x_j                 [nf, K] per row
//   T_a[k] = sum_b Rs[a,b] S_b[k]
//   pred   = sum_j W[f_j] x_j
//            + 0.5 ( sum_a <S_a, T_a> - sum_j Rs[a_j,a_j] |V[f_j] x_j|^2 )
//   gw[j]   = d x_j
//   gv[j,k] = d x_j ( T_{a_j}[k] - Rs[a_j,a_j] V[f_j,k] x_j )
//   dR[a,b] = sum_rows d <S_a, S_b>                         a < b
//   dR[a,a] = sum_rows d sum_{i<j, a_i = a_j = a} <V[f_i] x_i, V[f_j] x_j>
//   dR[a,b] = 0                                             a > b
//
// O(nf^2 K) a row however many entries share a field. An entry whose field
// is outside [0, nf) counts in the wide term only (gw = d x, gv = 0); the
// field id is device data, compared with nf before it indexes anything.
//
// Work split. The layout of embed_kernels.hip / deepfm_kernels.hip: one
// wavefront per row, four waves per 256-thread block, lane = (g, k) with
// G = 64/K entries per trip, 4-deep pipelined gathers. Unlike those, a
// bounded grid of blocks strides over the rows, so that Rs is staged in LDS
// once per block and not once per four rows, and so that the number of dR
// partials is fixed by the grid.
//
// LDS (dynamic, fp32 words; fwfm_lds_bytes is the backward's figure and the
// one rule both bindings check):
//   block:  Rs[nf*nf], backward also pair[nf(nf+1)/2] = (a, b) of the t-th
//           cell of the upper triangle in row-major order
//   wave:   S[nf*K], cnt[nf]; backward also T[nf*K], acc[nf(nf+1)/2] (the
//           wave's dR sums) and dq[nf] (the row's diagonal terms)
// 16.7 KB (forward) / 42.9 KB (backward) per block at nf = 39, K = 16;
// 102.8 KB at nf = 39, K = 64; 92.8 KB at nf = 64, K = 16. nf = 64 with
// K = 64 needs 191 KB and is refused.
//
// Scatter into S. A first pass counts the row's entries per field with
// integer LDS atomics (order-free). If no field holds two entries, every
// lane adds its product to its own zeroed cell, all groups at once. Else the
// groups of a trip go one after the other with a wave-level fence between
// them, so a cell's value is ((+0 + p_1) + p_2) + ... in entry order: the
// idea of embed_bag_kernels.hip. No LDS float atomics. In the same step the
// backward takes <S_a before the add, p_j> (a butterfly over the K lanes of
// the group): summed over the field's entries that is the diagonal term of
// dR as a sum over pairs, exactly 0 for a field with one entry and free of
// the cancellation of 0.5 (<S_a,S_a> - Q_a).
//
// T = Rs S. Lane (g, k) owns the cells (a, k), a = g + G c, and computes
// four of them per trip over b: one S[b,k] read feeds four FMAs. The
// forward never stores T, it multiplies each cell by S[a,k] on the spot.
//
// Gram terms. Plain FMA on the upper triangle only: lane t + 64 c takes the
// t-th cell of the triangle from the pair list, so all 64 lanes are busy
// whatever nf is, and reads both rows of S as float4. The fp32 MFMA forms
// would pad nf = 39 to 48 or 64 and compute the full square; by the
// arithmetic (780 x K FMA a row against the row's gather) neither is the
// long phase, so the simpler one was taken. Not measured against MFMA.
//
// dR reduce. Every wave adds d * cell into its own acc, its rows in
// increasing order; the block adds its four waves in wave order and writes
// one partial [nf(nf+1)/2]; fwfm_dr_reduce_kernel adds the partials of a
// cell in 16 interleaved slices, each in block order, and the slices in
// slice order. No float atomics: two runs are bit-identical.
#include "common.h"

// No packed fp32 instructions (v_pk_add_f32 / v_pk_fma_f32) in this file:
// the device code is generated with scalar fp32 arithmetic only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                     \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace lightctr {

static constexpr int kFwWpb = 4;        // waves (rows in flight) per block
static constexpr int kFwFwdGrid = 2048;  // forward: 8 blocks per CU
static constexpr int kFwBwdGrid = 768;   // backward: 3 blocks per CU
static constexpr int kFwRedCells = 16;   // dR reduce: cells per block
static constexpr int kFwRedSlices = 16;  //            slices per cell

extern __shared__ __align__(16) float fwfm_lds[];

__host__ __device__ constexpr int fw_pad4(int n) { return (n + 3) & ~3; }
__host__ __device__ constexpr int fw_ntri(int nf) {
  return nf * (nf + 1) / 2;
}

static long fwfm_forward_lds_bytes(int nf, int K) {
  return ((long)fw_pad4(nf * nf) +
          (long)kFwWpb * (nf * K + fw_pad4(nf))) * (long)sizeof(float);
}

// dynamic LDS per block of fwfm_backward_emit; the forward needs less
long fwfm_lds_bytes(int nf, int K) {
  const long wave = 2L * nf * K + fw_pad4(fw_ntri(nf)) + 2L * fw_pad4(nf);
  return ((long)fw_pad4(nf * nf) + fw_pad4(fw_ntri(nf)) + kFwWpb * wave) *
         (long)sizeof(float);
}

// blocks (= dR partials) of the backward for a batch of B rows
int fwfm_backward_blocks(int B) {
  const int want = (B + kFwWpb - 1) / kFwWpb;
  return want < kFwBwdGrid ? want : kFwBwdGrid;
}

// The runtime header's __shfl_xor, atomicAdd and __syncthreads are compiled
// with packed fp32 on and would stay real calls from functions compiled
// without it, so the few this file needs are written on the builtins.
template <typename T>
__device__ __forceinline__ T fw_shfl_xor(T v, int s) {
  static_assert(sizeof(T) == 4, "32-bit lanes");
  const int lane =
      __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return __builtin_bit_cast(
      T, __builtin_amdgcn_ds_bpermute((lane ^ s) << 2,
                                      __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ float fw_wave_sum(float v) {
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) v += fw_shfl_xor(v, s);
  return v;
}

// __syncthreads
__device__ __forceinline__ void fw_block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// LDS writes of some lanes of the wave become visible to its other lanes
__device__ __forceinline__ void fw_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Rs[a,b] = R[min(a,b), max(a,b)], by the whole block
__device__ __forceinline__ void fw_stage_rs(const float* __restrict__ R,
                                            float* Rs, int nf) {
  for (int i = threadIdx.x; i < nf * nf; i += blockDim.x) {
    const int a = i / nf, b = i % nf;
    Rs[i] = R[min(a, b) * nf + max(a, b)];
  }
}

// One product into its cell of S. Rows where a field repeats add the groups
// of the trip one after the other (entry order); `staged` is uniform over
// the wave and every lane takes every fence. BWD: dq[c] += <S_c, p> with
// S_c as it was before the add.
template <int K, bool BWD>
__device__ __forceinline__ void fw_scatter(bool staged, float* S, float* dq,
                                           int c, float vx, int g, int k) {
  constexpr int G = LCTR_WAVE / K;
  if (!staged) {
    if (c >= 0) S[c * K + k] += vx;
    return;
  }
#pragma unroll 1
  for (int gg = 0; gg < G; ++gg) {
    const bool mine = g == gg && c >= 0;
    float p = 0.f;
    if (mine) {
      const float old = S[c * K + k];
      p = old * vx;
      S[c * K + k] = old + vx;
    }
    if (BWD) {
#pragma unroll
      for (int s = 1; s < K; s <<= 1) p += fw_shfl_xor(p, s);
      if (mine && k == 0) dq[c] += p;
    }
    if (G > 1) fw_wave_sync();
  }
}

// The row's per-field sums S (and dq) in the wave's LDS. The forward also
// returns the lane's share of sum_j W x (lin, k == 0 lanes) and of
// sum_j Rs[a_j,a_j] (V x)^2 (qd).
template <int K, bool BWD>
__device__ __forceinline__ void fw_row_sums(
    const int* __restrict__ fields, const int* __restrict__ fids,
    const float* __restrict__ vals, const float* __restrict__ W,
    const float* __restrict__ V, const float* Rs, int beg, int end, int nf,
    int lane, float* S, float* dq, int* cnt, float& lin, float& qd) {
  constexpr int G = LCTR_WAVE / K;
  const int g = lane / K;
  const int k = lane % K;
  for (int i = lane; i < nf; i += LCTR_WAVE) {
    cnt[i] = 0;
    if (BWD) dq[i] = 0.f;
  }
  for (int i = lane; i < nf * K; i += LCTR_WAVE) S[i] = 0.f;
  fw_wave_sync();
  for (int j = beg + lane; j < end; j += LCTR_WAVE) {
    const int c = fields[j];
    if ((unsigned)c < (unsigned)nf)
      __hip_atomic_fetch_add(&cnt[c], 1, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  fw_wave_sync();
  int mx = 0;
  for (int i = lane; i < nf; i += LCTR_WAVE) mx = max(mx, cnt[i]);
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) mx = max(mx, fw_shfl_xor(mx, s));
  const bool staged = mx > 1;

  // trips are counted from a wave-uniform base: every lane of the wave
  // takes every fence of fw_scatter
  int jb = beg;
  for (; jb + 4 * G <= end; jb += 4 * G) {
    int f[4], c[4];
    float x[4], e[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = jb + u * G + g;
      f[u] = fids[j];
      x[u] = vals[j];
      c[u] = fields[j];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      e[u] = V[(size_t)f[u] * K + k];
      w[u] = (!BWD && k == 0) ? W[f[u]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float vx = e[u] * x[u];
      const int cu = ((unsigned)c[u] < (unsigned)nf) ? c[u] : -1;
      if (!BWD) {
        lin = fmaf(w[u], x[u], lin);
        if (cu >= 0) qd = fmaf(Rs[cu * nf + cu] * vx, vx, qd);
      }
      fw_scatter<K, BWD>(staged, S, dq, cu, vx, g, k);
    }
  }
  for (; jb < end; jb += G) {
    const int j = jb + g;
    float vx = 0.f;
    int cu = -1;
    if (j < end) {
      const int fid = fids[j];
      const float x = vals[j];
      const int c = fields[j];
      vx = V[(size_t)fid * K + k] * x;
      if ((unsigned)c < (unsigned)nf) cu = c;
      if (!BWD) {
        if (k == 0) lin = fmaf(W[fid], x, lin);
        if (cu >= 0) qd = fmaf(Rs[cu * nf + cu] * vx, vx, qd);
      }
    }
    fw_scatter<K, BWD>(staged, S, dq, cu, vx, g, k);
  }
  fw_wave_sync();
}

// Four cells (a[u], k) of T = Rs S for this lane; a[u] >= nf computes row
// nf - 1 again and is discarded by the caller.
template <int K>
__device__ __forceinline__ void fw_t_cells(const float* Rs, const float* S,
                                           int nf, int k, const int a[4],
                                           float acc[4]) {
  const float* r[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    r[u] = Rs + min(a[u], nf - 1) * nf;
    acc[u] = 0.f;
  }
  for (int b = 0; b < nf; ++b) {
    const float s = S[b * K + k];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(r[u][b], s, acc[u]);
  }
}

template <int K>
__global__ __launch_bounds__(256) void fwfm_forward_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const int* __restrict__ fids, const float* __restrict__ vals,
    const float* __restrict__ W, const float* __restrict__ V,
    const float* __restrict__ R, float* __restrict__ pred, int nf, int B) {
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / K;
  const int k = lane % K;
  float* Rs = fwfm_lds;
  float* S = Rs + fw_pad4(nf * nf) + (size_t)wave * (nf * K + fw_pad4(nf));
  int* cnt = (int*)(S + nf * K);
  fw_stage_rs(R, Rs, nf);
  fw_block_sync();

  for (int row = blockIdx.x * kFwWpb + wave; row < B;
       row += gridDim.x * kFwWpb) {
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    if (end <= beg) {  // uniform over the wave
      if (lane == 0) pred[row] = 0.f;
      continue;
    }
    float lin = 0.f, qd = 0.f;
    fw_row_sums<K, false>(fields, fids, vals, W, V, Rs, beg, end, nf, lane,
                          S, nullptr, cnt, lin, qd);
    float pair = 0.f;  // this lane's share of sum_a <S_a, T_a>
    for (int c0 = 0; c0 * G < nf; c0 += 4) {
      int a[4];
      float acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = g + G * (c0 + u);
      fw_t_cells<K>(Rs, S, nf, k, a, acc);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (a[u] < nf) pair = fmaf(acc[u], S[a[u] * K + k], pair);
    }
    pair = fw_wave_sum(pair);
    qd = fw_wave_sum(qd);
    lin = fw_wave_sum(lin);  // non-zero on the k == 0 lanes only
    if (lane == 0) pred[row] = lin + 0.5f * (pair - qd);
    fw_wave_sync();  // S is zeroed again by the next row
  }
}

// gw, gv per entry and one dR partial [nf(nf+1)/2] per block. V is gathered
// twice, for S and for the - Rs[a,a] V x term once T is known; the second
// gather repeats addresses this wave touched a few hundred cycles earlier.
template <int K>
__global__ __launch_bounds__(256) void fwfm_backward_emit_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const int* __restrict__ fids, const float* __restrict__ vals,
    const float* __restrict__ V, const float* __restrict__ R,
    const float* __restrict__ dpred, float* __restrict__ gw,
    float* __restrict__ gv, float* __restrict__ partial, int nf, int B) {
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int g = lane / K;
  const int k = lane % K;
  const int ntri = fw_ntri(nf);
  const int tri_n = fw_pad4(ntri);
  float* Rs = fwfm_lds;
  int* pairs = (int*)(Rs + fw_pad4(nf * nf));
  const int wave_n = 2 * nf * K + tri_n + 2 * fw_pad4(nf);
  float* S = (float*)(pairs + tri_n) + (size_t)wave * wave_n;
  float* T = S + nf * K;
  float* acc = T + nf * K;
  float* dq = acc + tri_n;
  int* cnt = (int*)(dq + fw_pad4(nf));

  fw_stage_rs(R, Rs, nf);
  for (int i = threadIdx.x; i < nf * nf; i += blockDim.x) {
    const int a = i / nf, b = i % nf;
    if (a <= b) pairs[a * nf - a * (a - 1) / 2 + (b - a)] = a | (b << 16);
  }
  for (int t = lane; t < ntri; t += LCTR_WAVE) acc[t] = 0.f;
  fw_block_sync();

  for (int row = blockIdx.x * kFwWpb + wave; row < B;
       row += gridDim.x * kFwWpb) {
    const int beg = row_ptr[row], end = row_ptr[row + 1];
    if (end <= beg) continue;  // uniform over the wave; all its sums are 0
    const float d = dpred[row];
    float lin = 0.f, qd = 0.f;  // forward only
    fw_row_sums<K, true>(fields, fids, vals, nullptr, V, Rs, beg, end, nf,
                         lane, S, dq, cnt, lin, qd);
    for (int c0 = 0; c0 * G < nf; c0 += 4) {
      int a[4];
      float t4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = g + G * (c0 + u);
      fw_t_cells<K>(Rs, S, nf, k, a, t4);
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (a[u] < nf) T[a[u] * K + k] = t4[u];
    }
    fw_wave_sync();

    // emit
    int j = beg + g;
    for (; j + 3 * G < end; j += 4 * G) {
      int f[4], c[4];
      float x[4], e[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f[u] = fids[j + u * G];
        x[u] = vals[j + u * G];
        c[u] = fields[j + u * G];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) e[u] = V[(size_t)f[u] * K + k];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float dx = d * x[u];
        float out = 0.f;
        if ((unsigned)c[u] < (unsigned)nf)
          out = dx * (T[c[u] * K + k] -
                      Rs[c[u] * nf + c[u]] * (e[u] * x[u]));
        gv[(size_t)(j + u * G) * K + k] = out;
        if (k == 0) gw[j + u * G] = dx;
      }
    }
    for (; j < end; j += G) {
      const float x = vals[j];
      const int c = fields[j];
      const float e = V[(size_t)fids[j] * K + k];
      const float dx = d * x;
      float out = 0.f;
      if ((unsigned)c < (unsigned)nf)
        out = dx * (T[c * K + k] - Rs[c * nf + c] * (e * x));
      gv[(size_t)j * K + k] = out;
      if (k == 0) gw[j] = dx;
    }

    // Gram terms of the upper triangle into the wave's sums; a lane only
    // ever touches its own cells of acc
    for (int t = lane; t < ntri; t += LCTR_WAVE) {
      const int pr = pairs[t];
      const int a = pr & 0xffff, b = pr >> 16;
      float v;
      if (a == b) {
        v = dq[a];
      } else {
        const float4* sa = (const float4*)(S + a * K);
        const float4* sb = (const float4*)(S + b * K);
        v = 0.f;
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
          const float4 p = sa[q], r = sb[q];
          v = fmaf(p.x, r.x, v);
          v = fmaf(p.y, r.y, v);
          v = fmaf(p.z, r.z, v);
          v = fmaf(p.w, r.w, v);
        }
      }
      acc[t] = fmaf(d, v, acc[t]);
    }
    fw_wave_sync();  // S, T, dq and cnt are rewritten by the next row
  }

  fw_block_sync();
  const float* acc0 = (const float*)(pairs + tri_n) + 2 * nf * K;
  for (int t = threadIdx.x; t < ntri; t += blockDim.x) {
    float s = acc0[t];
#pragma unroll
    for (int w = 1; w < kFwWpb; ++w) s += acc0[(size_t)w * wave_n + t];
    partial[(size_t)blockIdx.x * ntri + t] = s;
  }
}

// dR[a,b] = sum over the blocks' partials (a <= b), 0 below the diagonal.
// Thread (slice, cell): slice s adds blocks s, s + 16, ... in that order,
// then the 16 slices are added in slice order.
__global__ __launch_bounds__(256) void fwfm_dr_reduce_kernel(
    const float* __restrict__ partial, float* __restrict__ dR, int nf,
    int nblocks) {
  __shared__ float part[kFwRedSlices][kFwRedCells];
  const int cl = threadIdx.x % kFwRedCells;
  const int sl = threadIdx.x / kFwRedCells;
  const int cell = blockIdx.x * kFwRedCells + cl;
  const int ntri = fw_ntri(nf);
  const bool in = cell < nf * nf;
  const int a = in ? cell / nf : 0, b = in ? cell % nf : 0;
  const bool upper = in && a <= b;
  const int t = a * nf - a * (a - 1) / 2 + (b - a);
  float s = 0.f;
  if (upper)
    for (int blk = sl; blk < nblocks; blk += kFwRedSlices)
      s += partial[(size_t)blk * ntri + t];
  part[sl][cl] = s;
  fw_block_sync();
  if (sl == 0 && in) {
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < kFwRedSlices; ++q) tot += part[q][cl];
    dR[cell] = tot;
  }
}

// requests above 64 KB of dynamic LDS have to be announced per kernel
template <typename Kern>
static void fw_raise_lds(Kern kernel, size_t lds) {
  if (lds > 64 * 1024)
    LCTR_CHECK_HIP(hipFuncSetAttribute(
        (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)lds));
}

void fwfm_forward_launch(const int* row_ptr, const int* fields,
                         const int* fids, const float* vals, const float* W,
                         const float* V, const float* R, float* pred, int nf,
                         int B, int K, hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(kFwWpb * LCTR_WAVE);
  const int want = (B + kFwWpb - 1) / kFwWpb;
  dim3 grid(want < kFwFwdGrid ? want : kFwFwdGrid);
  const size_t lds = (size_t)fwfm_forward_lds_bytes(nf, K);
  DISPATCH_K(K, fw_raise_lds(fwfm_forward_kernel<KC>, lds);
             hipLaunchKernelGGL((fwfm_forward_kernel<KC>), grid, block, lds,
                                stream, row_ptr, fields, fids, vals, W, V, R,
                                pred, nf, B));
}

// partial: [fwfm_backward_blocks(B), nf(nf+1)/2] of workspace. dR is
// written for every B, as zeros for an empty batch.
void fwfm_backward_emit_launch(const int* row_ptr, const int* fields,
                               const int* fids, const float* vals,
                               const float* V, const float* R,
                               const float* dpred, float* gw, float* gv,
                               float* partial, float* dR, int nf, int B,
                               int K, hipStream_t stream) {
  const int nblocks = fwfm_backward_blocks(B);
  if (nblocks > 0) {
    dim3 block(kFwWpb * LCTR_WAVE);
    dim3 grid(nblocks);
    const size_t lds = (size_t)fwfm_lds_bytes(nf, K);
    DISPATCH_K(K, fw_raise_lds(fwfm_backward_emit_kernel<KC>, lds);
               hipLaunchKernelGGL((fwfm_backward_emit_kernel<KC>), grid,
                                  block, lds, stream, row_ptr, fields, fids,
                                  vals, V, R, dpred, gw, gv, partial, nf, B));
  }
  dim3 rgrid((nf * nf + kFwRedCells - 1) / kFwRedCells);
  hipLaunchKernelGGL(fwfm_dr_reduce_kernel, rgrid,
                     dim3(kFwRedCells * kFwRedSlices), 0, stream, partial, dR,
                     nf, nblocks > 0 ? nblocks : 0);
}

}  // namespace lightctr

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
