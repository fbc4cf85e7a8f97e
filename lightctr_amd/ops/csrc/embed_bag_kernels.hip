// Field-addressed embedding bags for MI355X/gfx950: the concat input of
// Wide&Deep and DeepFM laid out by an entry's field instead of its position
// in the row, with sum or mean pooling of the entries that share a field:
//
//   out[r, c*K+k] = bf16( inv(r,c) * sum_{j in row r, fields[j] == c}
//                                        E[fids[j],k] * vals[j] )
//
// inv = 1 for sum pooling and 1/cnt(r,c) for mean, cnt being the number of
// entries of the row in the slot (not the sum of their x). An entry whose
// field is < 0 or >= nf is left out of the concat (its D is 0 in the
// backward); it still counts in wide, fm and sumVX and still gets gw and the
// FM part of gv. The field id is device data: it is compared against nf
// before it is used and never indexes anything unguarded. Slots without an
// entry are written as +0 (the output is at::empty).
//
// Layout of embed_kernels.hip / deepfm_kernels.hip: one wavefront per row,
// four rows per 256-thread block, lane = (g, k) with G = 64/K entries per
// trip, 4-deep pipelined gathers, templated on K.
//
// Per wave the block's dynamic LDS holds nf*K fp32 of staging and nf int
// counters: 16*nf*(K+1) bytes per block (embed_bag_lds_bytes).
//
// Order of additions. A first pass over the row's fields counts the entries
// of every slot with integer LDS atomics (order-free, so deterministic).
//  * No slot holds more than one entry (the common one-value-per-field
//    row): every product goes straight to global memory as
//    bf16(+0 + E x); the staging is not touched. inv is 1 in both modes.
//  * Otherwise the row is staged: the slice is zeroed, and the entries are
//    added to their slots with plain LDS read-modify-writes in ENTRY ORDER:
//    trip after trip, and inside a trip one group g after the other, with a
//    wave-level fence and barrier between two groups (the K lanes of one
//    group hit K consecutive floats: no bank conflict; different groups that
//    land in one slot are what the barrier serialises). A slot's value is
//    ((+0 + p_1) + p_2) + ... for its entries j_1 < j_2 < ... in row order,
//    then one correctly rounded multiply by inv, then bf16.
// With one entry per slot the staged value is (+0 + p) * 1, which is what
// the direct path writes, so the two paths are bit-equal; two launches on
// the same input are bit-equal as well. No LDS float atomics anywhere.
//
// The backward needs cnt only for mean pooling and recounts it with the
// same first pass into nf counters per wave (16*nf bytes per block); sum
// pooling uses no LDS in the backward. See docs/KERNELS.md for why the
// recount was chosen over a stored [B, nf] count tensor.
#include "common.h"

namespace lightctr {

static constexpr int kBagWpb = 4;  // waves (rows) per block

extern __shared__ float bag_lds[];

// dynamic LDS of the forward kernels: [nf, K] fp32 + [nf] int32 per wave
long embed_bag_lds_bytes(int nf, int K) {
  return (long)kBagWpb * nf * (K + 1) * (long)sizeof(float);
}

// LDS writes of some lanes of the wave become visible to its other lanes
__device__ __forceinline__ void bag_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// cnt[c] = number of entries of [beg, end) with field c, 0 <= c < nf
__device__ __forceinline__ void bag_count(const int* __restrict__ fields,
                                          int beg, int end, int nf, int lane,
                                          int* cnt) {
  for (int i = lane; i < nf; i += LCTR_WAVE) cnt[i] = 0;
  bag_wave_sync();
  for (int j = beg + lane; j < end; j += LCTR_WAVE) {
    const int c = fields[j];
    if ((unsigned)c < (unsigned)nf) atomicAdd(&cnt[c], 1);
  }
  bag_wave_sync();
}

// largest slot count of the row, the same in every lane
__device__ __forceinline__ int bag_max_count(const int* cnt, int nf,
                                             int lane) {
  int mx = 0;
  for (int i = lane; i < nf; i += LCTR_WAVE) mx = max(mx, cnt[i]);
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) mx = max(mx, __shfl_xor(mx, s));
  return mx;
}

// The per-slot accumulation of one trip: lane (g, k) holds the product vx
// of the trip's g-th entry and its slot c (-1: none). Staged rows add the
// groups one after the other (entry order); rows without a shared slot
// store bf16(+0 + vx) directly. `staged` is uniform over the wave.
template <int K>
__device__ __forceinline__ void bag_slot_add(bool staged, float* stage,
                                             __bf16* __restrict__ slice,
                                             int c, float vx, int g, int k) {
  constexpr int G = LCTR_WAVE / K;
  if (staged) {
#pragma unroll 1
    for (int gg = 0; gg < G; ++gg) {
      if (g == gg && c >= 0) stage[c * K + k] += vx;
      if (G > 1) bag_wave_sync();
    }
  } else if (c >= 0) {
    slice[(size_t)c * K + k] = (__bf16)(0.f + vx);
  }
}

// One row of the forward. FM adds deepfm_forward_kernel's sums (fm, sumVX
// over all entries of the row) to the same trip over the row.
template <int K, bool FM>
__device__ __forceinline__ void bag_forward_row(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const int* __restrict__ fids, const float* __restrict__ vals,
    const float* __restrict__ W, const float* __restrict__ E,
    __bf16* __restrict__ out_bf, float* __restrict__ sumVX,
    float* __restrict__ fm, int nf, int pooling, int row, int lane,
    float* stage) {
  constexpr int G = LCTR_WAVE / K;
  const int g = lane / K;
  const int k = lane % K;
  const int beg = row_ptr[row], end = row_ptr[row + 1];
  __bf16* slice = out_bf + (size_t)row * nf * K;
  int* cnt = (int*)(stage + nf * K);

  bag_count(fields, beg, end, nf, lane, cnt);
  const bool staged = bag_max_count(cnt, nf, lane) > 1;
  if (staged) {
    for (int i = lane; i < nf * K; i += LCTR_WAVE) stage[i] = 0.f;
    bag_wave_sync();
  }

  float sVX = 0.f, sV2X2 = 0.f, lin = 0.f;
  // trips are counted from a wave-uniform base: every lane of the wave
  // takes every barrier of bag_slot_add
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
      e[u] = E[(size_t)f[u] * K + k];
      w[u] = (FM && k == 0) ? W[f[u]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float vx = e[u] * x[u];
      if (FM) {
        sVX += vx;
        sV2X2 += vx * vx;
        lin = fmaf(w[u], x[u], lin);
      }
      const int cu = ((unsigned)c[u] < (unsigned)nf) ? c[u] : -1;
      bag_slot_add<K>(staged, stage, slice, cu, vx, g, k);
    }
  }
  for (; jb < end; jb += G) {
    const int j = jb + g;
    const bool valid = j < end;
    float vx = 0.f;
    int cu = -1;
    if (valid) {
      const int fid = fids[j];
      const float x = vals[j];
      const int c = fields[j];
      vx = E[(size_t)fid * K + k] * x;
      if (FM) {
        sVX += vx;
        sV2X2 += vx * vx;
        if (k == 0) lin = fmaf(W[fid], x, lin);
      }
      if ((unsigned)c < (unsigned)nf) cu = c;
    }
    bag_slot_add<K>(staged, stage, slice, cu, vx, g, k);
  }

  if (FM) {
    // deepfm_forward_kernel's reduction
    sVX = group_reduce_sum<K>(sVX);
    sV2X2 = group_reduce_sum<K>(sV2X2);
    float pair = sVX * sVX - sV2X2;
#pragma unroll
    for (int s = 1; s < K; s <<= 1) pair += __shfl_xor(pair, s);
    lin = group_reduce_sum<K>(lin);
    if (lane < K) sumVX[(size_t)row * K + lane] = sVX;
    if (lane == 0) fm[row] = lin + 0.5f * pair;
  }

  if (staged) {
    // every slot of the slice: pooled sum -> one multiply by inv -> bf16;
    // slots without an entry still hold the +0 they were zeroed to
    for (int i = lane; i < nf * K; i += LCTR_WAVE) {
      const int n = cnt[i / K];
      const float inv = (pooling == 1 && n > 1) ? __frcp_rn((float)n) : 1.f;
      slice[i] = (__bf16)__fmul_rn(stage[i], inv);
    }
  } else {
    for (int i = lane; i < nf * K; i += LCTR_WAVE)
      if (cnt[i / K] == 0) slice[i] = (__bf16)0.f;
  }
}

template <int K>
__global__ __launch_bounds__(256) void embed_bag_forward_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const int* __restrict__ fids, const float* __restrict__ vals,
    const float* __restrict__ E, __bf16* __restrict__ out_bf, int nf,
    int pooling, int B) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * kBagWpb + wave;
  if (row >= B) return;
  bag_forward_row<K, false>(row_ptr, fields, fids, vals, nullptr, E, out_bf,
                            nullptr, nullptr, nf, pooling, row, lane,
                            bag_lds + (size_t)wave * nf * (K + 1));
}

template <int K>
__global__ __launch_bounds__(256) void deepfm_bag_forward_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const int* __restrict__ fids, const float* __restrict__ vals,
    const float* __restrict__ W, const float* __restrict__ E,
    __bf16* __restrict__ out_bf, float* __restrict__ sumVX,
    float* __restrict__ fm, int nf, int pooling, int B) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * kBagWpb + wave;
  if (row >= B) return;
  bag_forward_row<K, true>(row_ptr, fields, fids, vals, W, E, out_bf, sumVX,
                           fm, nf, pooling, row, lane,
                           bag_lds + (size_t)wave * nf * (K + 1));
}

// One row of the backward emit. Per entry j of row r, c = fields[j],
// D = dOut[r, c*K+k] (0 for a field outside [0, nf)), inv = 1 (sum) or
// 1/cnt(r,c) (mean):
//   FM:   gw[j] = d x_j,  gv[j,k] = (D inv + d (sumVX[r,k] - E[f_j,k] x_j)) x_j
//   else: gw[j] = d x_j,  gv[j,k] = D inv x_j          d = dpred / dwide [r]
// D inv is one correctly rounded multiply of its own (never contracted into
// the addition), so that with inv = 1 the arithmetic is the position
// kernels'.
template <int K, bool FM>
__device__ __forceinline__ void bag_backward_row(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const int* __restrict__ fids, const float* __restrict__ vals,
    const float* __restrict__ E, const float* __restrict__ sumVX,
    const float* __restrict__ dOut, const float* __restrict__ dscore,
    float* __restrict__ gw, float* __restrict__ gv, int nf, int pooling,
    int row, int lane, int* cnt) {
  constexpr int G = LCTR_WAVE / K;
  const int g = lane / K;
  const int k = lane % K;
  const float d = dscore[row];
  const float sv = FM ? sumVX[(size_t)row * K + k] : 0.f;
  const int beg = row_ptr[row], end = row_ptr[row + 1];
  const float* drow = dOut + (size_t)row * nf * K;
  const bool mean = pooling == 1;
  if (mean) bag_count(fields, beg, end, nf, lane, cnt);
  int j = beg + g;
  for (; j + 3 * G < end; j += 4 * G) {
    int f[4], c[4];
    float x[4], e[4], D[4], inv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (FM) f[u] = fids[j + u * G];
      x[u] = vals[j + u * G];
      c[u] = fields[j + u * G];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool in = (unsigned)c[u] < (unsigned)nf;
      e[u] = FM ? E[(size_t)f[u] * K + k] : 0.f;
      D[u] = in ? drow[(size_t)c[u] * K + k] : 0.f;
      inv[u] = (mean && in) ? __frcp_rn((float)cnt[c[u]]) : 1.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float Dm = __fmul_rn(D[u], inv[u]);
      if (FM)
        gv[(size_t)(j + u * G) * K + k] =
            (Dm + d * (sv - e[u] * x[u])) * x[u];
      else
        gv[(size_t)(j + u * G) * K + k] = Dm * x[u];
      if (k == 0) gw[j + u * G] = d * x[u];
    }
  }
  for (; j < end; j += G) {
    const float x = vals[j];
    const int c = fields[j];
    const bool in = (unsigned)c < (unsigned)nf;
    const float D = in ? drow[(size_t)c * K + k] : 0.f;
    const float inv = (mean && in) ? __frcp_rn((float)cnt[c]) : 1.f;
    const float Dm = __fmul_rn(D, inv);
    if (FM) {
      const float e = E[(size_t)fids[j] * K + k];
      gv[(size_t)j * K + k] = (Dm + d * (sv - e * x)) * x;
    } else {
      gv[(size_t)j * K + k] = Dm * x;
    }
    if (k == 0) gw[j] = d * x;
  }
}

template <int K>
__global__ __launch_bounds__(256) void embed_bag_backward_emit_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const float* __restrict__ vals, const float* __restrict__ dOut,
    const float* __restrict__ dwide, float* __restrict__ gw,
    float* __restrict__ gv, int nf, int pooling, int B) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * kBagWpb + wave;
  if (row >= B) return;
  bag_backward_row<K, false>(row_ptr, fields, nullptr, vals, nullptr, nullptr,
                             dOut, dwide, gw, gv, nf, pooling, row, lane,
                             (int*)bag_lds + (size_t)wave * nf);
}

template <int K>
__global__ __launch_bounds__(256) void deepfm_bag_backward_emit_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fields,
    const int* __restrict__ fids, const float* __restrict__ vals,
    const float* __restrict__ E, const float* __restrict__ sumVX,
    const float* __restrict__ dDeep, const float* __restrict__ dpred,
    float* __restrict__ gw, float* __restrict__ gv, int nf, int pooling,
    int B) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int row = blockIdx.x * kBagWpb + wave;
  if (row >= B) return;
  bag_backward_row<K, true>(row_ptr, fields, fids, vals, E, sumVX, dDeep,
                            dpred, gw, gv, nf, pooling, row, lane,
                            (int*)bag_lds + (size_t)wave * nf);
}

// requests above 64 KB of dynamic LDS have to be announced per kernel
template <typename Kern>
static void bag_raise_lds(Kern kernel, size_t lds) {
  if (lds > 64 * 1024)
    LCTR_CHECK_HIP(hipFuncSetAttribute(
        (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)lds));
}

void embed_bag_forward_launch(const int* row_ptr, const int* fields,
                              const int* fids, const float* vals,
                              const float* E, void* out_bf, int nf,
                              int pooling, int B, int K, hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(kBagWpb * LCTR_WAVE);
  dim3 grid((B + kBagWpb - 1) / kBagWpb);
  const size_t lds = (size_t)embed_bag_lds_bytes(nf, K);
  DISPATCH_K(K, bag_raise_lds(embed_bag_forward_kernel<KC>, lds);
             hipLaunchKernelGGL((embed_bag_forward_kernel<KC>), grid, block,
                                lds, stream, row_ptr, fields, fids, vals, E,
                                (__bf16*)out_bf, nf, pooling, B));
}

void deepfm_bag_forward_launch(const int* row_ptr, const int* fields,
                               const int* fids, const float* vals,
                               const float* W, const float* E, void* out_bf,
                               float* sumVX, float* fm, int nf, int pooling,
                               int B, int K, hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(kBagWpb * LCTR_WAVE);
  dim3 grid((B + kBagWpb - 1) / kBagWpb);
  const size_t lds = (size_t)embed_bag_lds_bytes(nf, K);
  DISPATCH_K(K, bag_raise_lds(deepfm_bag_forward_kernel<KC>, lds);
             hipLaunchKernelGGL((deepfm_bag_forward_kernel<KC>), grid, block,
                                lds, stream, row_ptr, fields, fids, vals, W,
                                E, (__bf16*)out_bf, sumVX, fm, nf, pooling,
                                B));
}

// the backward keeps only the nf counters per wave, and only for mean
static size_t bag_backward_lds(int nf, int pooling) {
  return pooling == 1 ? (size_t)kBagWpb * nf * sizeof(int) : 0;
}

void embed_bag_backward_emit_launch(const int* row_ptr, const int* fields,
                                    const float* vals, const float* dOut,
                                    const float* dwide, float* gw, float* gv,
                                    int nf, int pooling, int B, int K,
                                    hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(kBagWpb * LCTR_WAVE);
  dim3 grid((B + kBagWpb - 1) / kBagWpb);
  const size_t lds = bag_backward_lds(nf, pooling);
  DISPATCH_K(K, bag_raise_lds(embed_bag_backward_emit_kernel<KC>, lds);
             hipLaunchKernelGGL((embed_bag_backward_emit_kernel<KC>), grid,
                                block, lds, stream, row_ptr, fields, vals,
                                dOut, dwide, gw, gv, nf, pooling, B));
}

void deepfm_bag_backward_emit_launch(const int* row_ptr, const int* fields,
                                     const int* fids, const float* vals,
                                     const float* E, const float* sumVX,
                                     const float* dDeep, const float* dpred,
                                     float* gw, float* gv, int nf,
                                     int pooling, int B, int K,
                                     hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(kBagWpb * LCTR_WAVE);
  dim3 grid((B + kBagWpb - 1) / kBagWpb);
  const size_t lds = bag_backward_lds(nf, pooling);
  DISPATCH_K(K, bag_raise_lds(deepfm_bag_backward_emit_kernel<KC>, lds);
             hipLaunchKernelGGL((deepfm_bag_backward_emit_kernel<KC>), grid,
                                block, lds, stream, row_ptr, fields, fids,
                                vals, E, sumVX, dDeep, dpred, gw, gv, nf,
                                pooling, B));
}

}  // namespace lightctr
