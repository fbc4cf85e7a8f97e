// DeepFM kernels for MI355X/gfx950: one embedding table E[F, K] used twice,
// as the FM latent factors of the pairwise term and as the per-field
// embeddings concatenated into the MLP input.
//
// The forward is fm_forward_kernel and embed_gather_kernel in one trip over
// the row: every CSR entry and every E row is read once, and the bf16 concat,
// sumVX and the FM score (wide + pair term) come out of the same products.
// The backward emit is fm_backward_emit_kernel and embed_backward_emit_kernel
// in one: a single [nnz, K] gradient buffer for the sorted segment-reduce
// apply (fm_kernels.hip::fm_sorted_apply_kernel) instead of two and an add.
//
// Layout of embed_kernels.hip throughout: one wavefront per row, four rows
// per 256-thread block, lane = (g, k) with G = 64/K entries per trip,
// 4-deep pipelined gathers.
#include "common.h"

namespace lightctr {

// fm[row]   = sum_j W[f_j] x_j + 0.5 sum_k (s_k^2 - sum_j (E[f_j,k] x_j)^2)
// sumVX[row,k] = s_k = sum_j E[f_j,k] x_j                 (all entries)
// out_bf[row, pos*K+k] = bf16(E[f_j,k] x_j), pos = j - beg < nf; positions
// len(row) <= pos < nf are written as +0. Entries at pos >= nf count in fm
// and sumVX only.
//
// Reduction: per-lane partials over the lane's entries, the stride-K
// butterfly across the G feature groups (every lane of a k then holds s_k
// and the k's square sum), s_k^2 - q_k per k, and a butterfly over the K
// lanes of a group. Nothing is added more than once, so the sums carry no
// replication factor.
//
// Allocates 44 VGPR (38 at K = 64), under the 64-VGPR boundary of 8
// waves/SIMD that embed_gather_kernel needs its occupancy cap for, so no cap
// here; no scratch (docs/KERNELS.md).
template <int K>
__global__ __launch_bounds__(256) void deepfm_forward_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fids,
    const float* __restrict__ vals, const float* __restrict__ W,
    const float* __restrict__ E, __bf16* __restrict__ out_bf,
    float* __restrict__ sumVX, float* __restrict__ fm, int nf, int B) {
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= B) return;
  const int g = lane / K;
  const int k = lane % K;
  const int beg = row_ptr[row], end = row_ptr[row + 1];
  __bf16* slice = out_bf + (size_t)row * nf * K;

  float sVX = 0.f;    // partial sum_j E[f,k] x over this lane's entries
  float sV2X2 = 0.f;  // partial sum_j (E[f,k] x)^2
  float lin = 0.f;    // partial sum_j W[f] x (k == 0 lanes only)
  int j = beg + g;
  for (; j + 3 * G < end; j += 4 * G) {
    int f[4];
    float x[4], e[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f[u] = fids[j + u * G];
      x[u] = vals[j + u * G];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      e[u] = E[(size_t)f[u] * K + k];
      w[u] = (k == 0) ? W[f[u]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float vx = e[u] * x[u];
      sVX += vx;
      sV2X2 += vx * vx;
      lin = fmaf(w[u], x[u], lin);
      const int pos = j + u * G - beg;
      if (pos < nf) slice[(size_t)pos * K + k] = (__bf16)vx;
    }
  }
  for (; j < end; j += G) {
    const int fid = fids[j];
    const float x = vals[j];
    const float vx = E[(size_t)fid * K + k] * x;
    sVX += vx;
    sV2X2 += vx * vx;
    if (k == 0) lin = fmaf(W[fid], x, lin);
    const int pos = j - beg;
    if (pos < nf) slice[(size_t)pos * K + k] = (__bf16)vx;
  }
  // feature groups: lanes {k, K+k, 2K+k, ...} -> s_k and q_k in every lane
  sVX = group_reduce_sum<K>(sVX);
  sV2X2 = group_reduce_sum<K>(sV2X2);
  // over k, inside each group of K lanes
  float pair = sVX * sVX - sV2X2;
#pragma unroll
  for (int s = 1; s < K; s <<= 1) pair += __shfl_xor(pair, s);
  // lin is non-zero on the k == 0 lanes only: the stride-K butterfly adds
  // exactly those
  lin = group_reduce_sum<K>(lin);
  if (lane < K) sumVX[(size_t)row * K + lane] = sVX;
  if (lane == 0) fm[row] = lin + 0.5f * pair;
  // rows shorter than nf: zero the rest of the slice (the output is
  // at::empty), as embed_gather_kernel does. No trip for fixed-width rows.
  for (int i = min(max(end - beg, 0), nf) * K + lane; i < nf * K;
       i += LCTR_WAVE)
    slice[i] = (__bf16)0.f;
}

// Per entry j of row r, d = dpred[r], D = dDeep[r, pos*K+k] (0 for
// pos >= nf):
//   gw[j]   = d * x_j
//   gv[j,k] = (D + d * (sumVX[r,k] - E[f_j,k] x_j)) * x_j
template <int K>
__global__ __launch_bounds__(256) void deepfm_backward_emit_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fids,
    const float* __restrict__ vals, const float* __restrict__ E,
    const float* __restrict__ sumVX, const float* __restrict__ dDeep,
    const float* __restrict__ dpred, float* __restrict__ gw,
    float* __restrict__ gv, int nf, int B) {
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= B) return;
  const int g = lane / K;
  const int k = lane % K;
  const float d = dpred[row];
  const float sv = sumVX[(size_t)row * K + k];
  const int beg = row_ptr[row], end = row_ptr[row + 1];
  const float* drow = dDeep + (size_t)row * nf * K;
  int j = beg + g;
  for (; j + 3 * G < end; j += 4 * G) {
    int f[4];
    float x[4], e[4], D[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f[u] = fids[j + u * G];
      x[u] = vals[j + u * G];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int pos = j + u * G - beg;
      e[u] = E[(size_t)f[u] * K + k];
      D[u] = (pos < nf) ? drow[(size_t)pos * K + k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      gv[(size_t)(j + u * G) * K + k] =
          (D[u] + d * (sv - e[u] * x[u])) * x[u];
      if (k == 0) gw[j + u * G] = d * x[u];
    }
  }
  for (; j < end; j += G) {
    const int pos = j - beg;
    const float x = vals[j];
    const float e = E[(size_t)fids[j] * K + k];
    const float D = (pos < nf) ? drow[(size_t)pos * K + k] : 0.f;
    gv[(size_t)j * K + k] = (D + d * (sv - e * x)) * x;
    if (k == 0) gw[j] = d * x;
  }
}

void deepfm_forward_launch(const int* row_ptr, const int* fids,
                           const float* vals, const float* W, const float* E,
                           void* out_bf, float* sumVX, float* fm, int nf,
                           int B, int K, hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(256);
  dim3 grid((B + 3) / 4);
  DISPATCH_K(K, hipLaunchKernelGGL((deepfm_forward_kernel<KC>), grid, block,
                                   0, stream, row_ptr, fids, vals, W, E,
                                   (__bf16*)out_bf, sumVX, fm, nf, B));
}

void deepfm_backward_emit_launch(const int* row_ptr, const int* fids,
                                 const float* vals, const float* E,
                                 const float* sumVX, const float* dDeep,
                                 const float* dpred, float* gw, float* gv,
                                 int nf, int B, int K, hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(256);
  dim3 grid((B + 3) / 4);
  DISPATCH_K(K, hipLaunchKernelGGL((deepfm_backward_emit_kernel<KC>), grid,
                                   block, 0, stream, row_ptr, fids, vals, E,
                                   sumVX, dDeep, dpred, gw, gv, nf, B));
}

}  // namespace lightctr
