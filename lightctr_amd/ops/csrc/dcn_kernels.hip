// Deep & Cross Network cross term (Wang et al., ADKDD 2017, vector form) for
// MI355X/gfx950, on the concat row x0[r, :] (bf16 [B, d], d = nf*K) that the
// MLP reads. Parameters Wc[L, d], bc[L, d], u[d], 1 <= L <= 8:
//
//   x_{l+1} = x0 (x_l . w_l) + b_l + x_l      l = 0 .. L-1
//   cross   = x_L . u
//
// Every x_l is sigma_l x0 + C_l with a per-row scalar sigma_l and a
// batch-independent vector C_l, so no x_l is ever formed. With w'_l = w_l
// (l < L), w'_L = u, C_0 = 0, C_{l+1} = C_l + b_l, sigma_0 = 1:
//
//   p_l = x0 . w'_l (per row)     q_l = C_l . w'_l (per step)
//   sigma_{l+1} = sigma_l + (sigma_l p_l + q_l)       cross = sigma_L p_L + q_L
//
// and backward, g = dpred[r]:
//
//   dsig_L = g p_L, a_L = g sigma_L, e_L = g
//   l = L-1 .. 0:  a_l = dsig_{l+1} sigma_l, e_l = dsig_{l+1},
//                  dsig_l = dsig_{l+1} (1 + p_l)
//   dx0[r, :] = sum_l a_l[r] w'_l         G[l, :] = sum_r a_l[r] x0[r, :]
//   dw'_l = G[l, :] + ebar_l C_l          ebar_l = sum_r e_l[r]
//   db_m  = sum_{l > m} ebar_l w'_l
//
// One pass over x0 each way at any L, against 3L elementwise passes over
// [B, d] for the layers composed from tensor ops.
//
// dcn_cross_prep: one block writes C[L+1, d] and q[L+1].
//
// Forward: w' is staged once per block in LDS ((L+1) d fp32, dynamic); a
// bounded grid of 4-wave blocks strides over the rows. A wave takes two rows
// at a time, so that each 16-byte LDS read of w' feeds 8 FMAs; lane j owns
// the 4-column groups 4 (j + 64 i) (one 8-byte bf16 load a row). The 2 (L+1)
// dots sit in registers (L is a template parameter), are summed by a
// butterfly over the wave, and the scalar recurrence runs on every lane.
// P[B, L+1] keeps the dots for the backward.
//
// Backward: a block owns a tile of 256 columns and a chunk of 256 rows.
// Thread t first runs the recurrence of row t of the chunk and leaves
// a_0..a_L in LDS (the blocks of column tile 0 also sum e over the chunk).
// Then the block walks the rows: threads 0..127 the even rows of the chunk,
// 128..255 the odd ones, a thread holding two adjacent columns (4-byte bf16
// and 8-byte fp32 accesses, four rows in flight). a is an LDS broadcast, w'
// and G live in 2 (L+1) registers each, dDeep is updated in place. The odd
// half hands its G over through LDS, and the block writes one partial
// [L+1, d] (and [L+1] of ebar). dcn_cross_finish adds the partials of a
// column in 16 interleaved slices, each in chunk order, the slices in slice
// order, and applies the ebar_l C_l and db terms. No float atomics anywhere:
// two runs are bit-identical.
#include "common.h"

// No packed fp32 instructions (v_pk_add_f32 / v_pk_fma_f32) in this file:
// the device code is generated with scalar fp32 arithmetic only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                     \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace lightctr {

static constexpr int kDcnMaxL = 8;
static constexpr int kDcnWpb = 4;         // forward: waves per block
static constexpr int kDcnRows = 2;        // forward: rows per wave and trip
static constexpr int kDcnFwdGrid = 1024;  // forward: 4 blocks per CU
static constexpr int kDcnTile = 256;      // backward: columns per block
static constexpr int kDcnChunk = 256;     // backward: rows per block
static constexpr int kDcnUnroll = 4;      // backward: rows in flight a thread
static constexpr int kDcnRedCols = 16;    // finish: columns per block
static constexpr int kDcnRedSlices = 16;  //         slices per column

extern __shared__ __align__(16) float dcn_lds[];

// dynamic LDS per block of the forward (w' staged whole); the backward's is
// static and below 20 KB at every L
long dcn_cross_lds_bytes(int L, int d) {
  return (long)(L + 1) * d * (long)sizeof(float);
}

// rows per backward block = rows per partial
int dcn_cross_backward_rows() { return kDcnChunk; }

int dcn_cross_backward_chunks(int B) {
  return B > 0 ? (B + kDcnChunk - 1) / kDcnChunk : 0;
}

// The runtime header's __shfl_xor and __syncthreads are compiled with packed
// fp32 on and would stay real calls from functions compiled without it, so
// the few this file needs are written on the builtins (as fwfm_kernels.hip).
__device__ __forceinline__ float dcn_shfl_xor(float v, int s) {
  const int lane =
      __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ s) << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ float dcn_wave_sum(float v) {
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) v += dcn_shfl_xor(v, s);
  return v;
}

__device__ __forceinline__ void dcn_block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// bf16 pair in a 32-bit word -> the two fp32 values (exact)
__device__ __forceinline__ float dcn_bf_lo(unsigned v) {
  return __builtin_bit_cast(float, v << 16);
}
__device__ __forceinline__ float dcn_bf_hi(unsigned v) {
  return __builtin_bit_cast(float, v & 0xffff0000u);
}

// w'_l[c]: row l of Wc, or u for l == L
__device__ __forceinline__ const float* dcn_wrow(const float* Wc,
                                                 const float* u, int l, int L,
                                                 int d) {
  return l < L ? Wc + (size_t)l * d : u;
}

// C[L+1, d] and q[L+1], one block. A thread sums its columns' products in
// column order; the 256 sums are added by the wave butterfly and then in
// wave order.
template <int L>
__global__ __launch_bounds__(256) void dcn_cross_prep_kernel(
    const float* __restrict__ Wc, const float* __restrict__ bc,
    const float* __restrict__ u, float* __restrict__ C,
    float* __restrict__ q, int d) {
  __shared__ float part[4][L + 1];
  float acc[L + 1];
#pragma unroll
  for (int l = 0; l <= L; ++l) acc[l] = 0.f;
  for (int c = threadIdx.x; c < d; c += blockDim.x) {
    float run = 0.f;
    C[c] = 0.f;
#pragma unroll
    for (int l = 1; l <= L; ++l) {
      run += bc[(size_t)(l - 1) * d + c];
      C[(size_t)l * d + c] = run;
      acc[l] = fmaf(run, dcn_wrow(Wc, u, l, L, d)[c], acc[l]);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int l = 0; l <= L; ++l) {
    const float s = dcn_wave_sum(acc[l]);
    if (lane == 0) part[wave][l] = s;
  }
  dcn_block_sync();
  if (threadIdx.x <= L)
    q[threadIdx.x] = ((part[0][threadIdx.x] + part[1][threadIdx.x]) +
                      part[2][threadIdx.x]) + part[3][threadIdx.x];
}

// sigma_0 .. sigma_L of a row from its dots
template <int L>
__device__ __forceinline__ void dcn_sigmas(const float p[L + 1],
                                           const float q[L + 1],
                                           float sig[L + 1]) {
  sig[0] = 1.f;
#pragma unroll
  for (int l = 0; l < L; ++l) sig[l + 1] = sig[l] + fmaf(sig[l], p[l], q[l]);
}

template <int L>
__global__ __launch_bounds__(256) void dcn_cross_forward_kernel(
    const unsigned short* __restrict__ x0, const float* __restrict__ Wc,
    const float* __restrict__ u, const float* __restrict__ q,
    float* __restrict__ cross, float* __restrict__ P, int d, int B) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  float* ws = dcn_lds;  // [L+1, d]
  {
    const int d4 = d >> 2;
    float4* dst = (float4*)ws;
    for (int i = threadIdx.x; i < (L + 1) * d4; i += blockDim.x) {
      const int l = i / d4, c4 = i - l * d4;
      dst[i] = ((const float4*)dcn_wrow(Wc, u, l, L, d))[c4];
    }
  }
  float ql[L + 1];
#pragma unroll
  for (int l = 0; l <= L; ++l) ql[l] = q[l];
  dcn_block_sync();

  const long step = (long)gridDim.x * kDcnWpb * kDcnRows;
  for (long row0 = ((long)blockIdx.x * kDcnWpb + wave) * kDcnRows; row0 < B;
       row0 += step) {
    float acc[kDcnRows][L + 1];
#pragma unroll
    for (int r = 0; r < kDcnRows; ++r)
#pragma unroll
      for (int l = 0; l <= L; ++l) acc[r][l] = 0.f;
    for (int c = lane * 4; c < d; c += LCTR_WAVE * 4) {
      float x[kDcnRows][4];
#pragma unroll
      for (int r = 0; r < kDcnRows; ++r) {
        uint2 v = make_uint2(0u, 0u);  // a row past the batch adds zeros
        if (row0 + r < B)
          v = *(const uint2*)(x0 + (size_t)(row0 + r) * d + c);
        x[r][0] = dcn_bf_lo(v.x);
        x[r][1] = dcn_bf_hi(v.x);
        x[r][2] = dcn_bf_lo(v.y);
        x[r][3] = dcn_bf_hi(v.y);
      }
#pragma unroll
      for (int l = 0; l <= L; ++l) {
        const float4 w = *(const float4*)(ws + (size_t)l * d + c);
#pragma unroll
        for (int r = 0; r < kDcnRows; ++r) {
          acc[r][l] = fmaf(x[r][0], w.x, acc[r][l]);
          acc[r][l] = fmaf(x[r][1], w.y, acc[r][l]);
          acc[r][l] = fmaf(x[r][2], w.z, acc[r][l]);
          acc[r][l] = fmaf(x[r][3], w.w, acc[r][l]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < kDcnRows; ++r) {
      float p[L + 1], sig[L + 1];
#pragma unroll
      for (int l = 0; l <= L; ++l) p[l] = dcn_wave_sum(acc[r][l]);
      if (row0 + r >= B) continue;  // uniform over the wave
      dcn_sigmas<L>(p, ql, sig);
      float* Pr = P + (size_t)(row0 + r) * (L + 1);
#pragma unroll
      for (int l = 0; l <= L; ++l)
        if (lane == l) Pr[l] = p[l];
      if (lane == 0) cross[row0 + r] = fmaf(sig[L], p[L], ql[L]);
    }
  }
}

template <int L>
__global__ __launch_bounds__(256) void dcn_cross_backward_kernel(
    const unsigned short* __restrict__ x0, const float* __restrict__ P,
    const float* __restrict__ Wc, const float* __restrict__ u,
    const float* __restrict__ q, const float* __restrict__ dpred,
    float* __restrict__ dDeep, float* __restrict__ partG,
    float* __restrict__ partE, int d, int B) {
  __shared__ __align__(16) float as[kDcnChunk][L + 1];
  __shared__ __align__(16) float gs[L + 1][kDcnTile];
  __shared__ float es[4][L + 1];
  const int t = threadIdx.x;
  const long r0 = (long)blockIdx.y * kDcnChunk;
  const int nrows = (int)(B - r0 < kDcnChunk ? B - r0 : kDcnChunk);

  // the chunk's scalars: thread t has row r0 + t
  {
    float a[L + 1], e[L + 1];
    if (t < nrows) {
      float p[L + 1], ql[L + 1], sig[L + 1];
#pragma unroll
      for (int l = 0; l <= L; ++l) {
        p[l] = P[(size_t)(r0 + t) * (L + 1) + l];
        ql[l] = q[l];
      }
      dcn_sigmas<L>(p, ql, sig);
      const float g = dpred[r0 + t];
      float dsig = g * p[L];
      a[L] = g * sig[L];
      e[L] = g;
#pragma unroll
      for (int l = L - 1; l >= 0; --l) {
        a[l] = dsig * sig[l];
        e[l] = dsig;
        dsig = fmaf(dsig, p[l], dsig);
      }
    } else {
#pragma unroll
      for (int l = 0; l <= L; ++l) a[l] = e[l] = 0.f;
    }
#pragma unroll
    for (int l = 0; l <= L; ++l) as[t][l] = a[l];
    if (blockIdx.x == 0) {  // uniform over the block
#pragma unroll
      for (int l = 0; l <= L; ++l) {
        const float s = dcn_wave_sum(e[l]);
        if ((t & 63) == 0) es[t >> 6][l] = s;
      }
    }
  }
  dcn_block_sync();
  if (blockIdx.x == 0 && t <= L)
    partE[(size_t)blockIdx.y * (L + 1) + t] =
        ((es[0][t] + es[1][t]) + es[2][t]) + es[3][t];

  // the walk: half h takes the rows h, h + 2, ... of the chunk
  const int h = t >> 7;
  const int tc = 2 * (t & 127);
  const int c = blockIdx.x * kDcnTile + tc;
  const bool active = c < d;  // d is even: c + 1 < d as well
  float w[L + 1][2], G[L + 1][2];
#pragma unroll
  for (int l = 0; l <= L; ++l) {
    const float2 v = active ? *(const float2*)(dcn_wrow(Wc, u, l, L, d) + c)
                            : make_float2(0.f, 0.f);
    w[l][0] = v.x;
    w[l][1] = v.y;
    G[l][0] = G[l][1] = 0.f;
  }
  if (active) {
    // i + 2 (kDcnUnroll - 1) stays below kDcnChunk: the chunk is a multiple
    // of 2 kDcnUnroll rows
    for (int i = h; i < nrows; i += 2 * kDcnUnroll) {
      unsigned xb[kDcnUnroll];
      float2 dd[kDcnUnroll];
#pragma unroll
      for (int k = 0; k < kDcnUnroll; ++k) {
        const int ii = i + 2 * k;
        xb[k] = 0u;  // a row past the chunk adds zeros and is not stored
        dd[k] = make_float2(0.f, 0.f);
        if (ii < nrows) {
          const size_t off = (size_t)(r0 + ii) * d + c;
          xb[k] = *(const unsigned*)(x0 + off);
          dd[k] = *(const float2*)(dDeep + off);
        }
      }
#pragma unroll
      for (int k = 0; k < kDcnUnroll; ++k) {
        const int ii = i + 2 * k;
        const float xa = dcn_bf_lo(xb[k]), xc = dcn_bf_hi(xb[k]);
#pragma unroll
        for (int l = 0; l <= L; ++l) {
          const float al = as[ii][l];
          dd[k].x = fmaf(al, w[l][0], dd[k].x);
          dd[k].y = fmaf(al, w[l][1], dd[k].y);
          G[l][0] = fmaf(al, xa, G[l][0]);
          G[l][1] = fmaf(al, xc, G[l][1]);
        }
        if (ii < nrows)
          *(float2*)(dDeep + (size_t)(r0 + ii) * d + c) = dd[k];
      }
    }
  }
  if (h == 1) {
#pragma unroll
    for (int l = 0; l <= L; ++l)
      *(float2*)&gs[l][tc] = make_float2(G[l][0], G[l][1]);
  }
  dcn_block_sync();
  if (h == 0 && active) {
#pragma unroll
    for (int l = 0; l <= L; ++l) {
      const float2 o = *(const float2*)&gs[l][tc];
      *(float2*)(partG + ((size_t)blockIdx.y * (L + 1) + l) * d + c) =
          make_float2(G[l][0] + o.x, G[l][1] + o.y);
    }
  }
}

// sum over the chunks of part[chunk * stride + j] for the 16 columns j of
// this block; thread (sl, cl) adds chunks sl, sl + 16, ... in that order,
// then the slices are added in slice order. Every thread of the block calls.
__device__ __forceinline__ float dcn_slice_sum(
    const float* __restrict__ part, size_t stride, int nchunks, bool in,
    int sl, int cl, float (*red)[kDcnRedCols]) {
  float s = 0.f;
  if (in)
    for (int k = sl; k < nchunks; k += kDcnRedSlices)
      s += part[(size_t)k * stride];
  dcn_block_sync();  // red is free again
  red[sl][cl] = s;
  dcn_block_sync();
  float tot = 0.f;
#pragma unroll
  for (int j = 0; j < kDcnRedSlices; ++j) tot += red[j][cl];
  return tot;
}

// dWc[L, d], dbc[L, d], du[d] from the partials; all zeros when nchunks == 0
template <int L>
__global__ __launch_bounds__(256) void dcn_cross_finish_kernel(
    const float* __restrict__ partG, const float* __restrict__ partE,
    const float* __restrict__ Wc, const float* __restrict__ u,
    const float* __restrict__ C, float* __restrict__ dWc,
    float* __restrict__ dbc, float* __restrict__ du, int d, int nchunks) {
  static_assert(L + 1 <= kDcnRedCols, "ebar is summed as one column group");
  __shared__ float red[kDcnRedSlices][kDcnRedCols];
  __shared__ float ebar[kDcnRedCols];
  const int cl = threadIdx.x % kDcnRedCols;
  const int sl = threadIdx.x / kDcnRedCols;
  const int c = blockIdx.x * kDcnRedCols + cl;
  const bool in = c < d;
  const float e = dcn_slice_sum(partE + cl, L + 1, nchunks, cl <= L, sl, cl,
                                red);
  if (sl == 0) ebar[cl] = e;
  dcn_block_sync();
  float suffix = 0.f;  // sum_{l > m} ebar_l w'_l[c], built from l = L down
#pragma unroll
  for (int l = L; l >= 0; --l) {
    const float g = dcn_slice_sum(partG + (size_t)l * d + (in ? c : 0),
                                  (size_t)(L + 1) * d, nchunks, in, sl, cl,
                                  red);
    if (sl == 0 && in) {
      const float el = ebar[l];
      const float dw = fmaf(el, C[(size_t)l * d + c], g);
      if (l == L) {
        du[c] = dw;
      } else {
        dWc[(size_t)l * d + c] = dw;
      }
      if (l >= 1) {
        suffix = fmaf(el, dcn_wrow(Wc, u, l, L, d)[c], suffix);
        dbc[(size_t)(l - 1) * d + c] = suffix;
      }
    }
  }
}

#define DISPATCH_DCN_L(LVAL, ...)                                     \
  switch (LVAL) {                                                     \
    case 1: { constexpr int LC = 1; __VA_ARGS__; break; }             \
    case 2: { constexpr int LC = 2; __VA_ARGS__; break; }             \
    case 3: { constexpr int LC = 3; __VA_ARGS__; break; }             \
    case 4: { constexpr int LC = 4; __VA_ARGS__; break; }             \
    case 5: { constexpr int LC = 5; __VA_ARGS__; break; }             \
    case 6: { constexpr int LC = 6; __VA_ARGS__; break; }             \
    case 7: { constexpr int LC = 7; __VA_ARGS__; break; }             \
    case 8: { constexpr int LC = 8; __VA_ARGS__; break; }             \
    default:                                                          \
      fprintf(stderr, "lightctr_amd: unsupported cross depth %d\n",   \
              LVAL);                                                  \
      abort();                                                        \
  }
static_assert(kDcnMaxL == 8, "DISPATCH_DCN_L covers 1..8");
static_assert(kDcnChunk % (2 * kDcnUnroll) == 0 && kDcnChunk == 256,
              "thread t of a 256-thread block has row t of the chunk");

void dcn_cross_prep_launch(const float* Wc, const float* bc, const float* u,
                           float* C, float* q, int L, int d,
                           hipStream_t stream) {
  DISPATCH_DCN_L(L, hipLaunchKernelGGL((dcn_cross_prep_kernel<LC>), dim3(1),
                                       dim3(256), 0, stream, Wc, bc, u, C, q,
                                       d));
}

void dcn_cross_forward_launch(const void* x0, const float* Wc, const float* u,
                              const float* q, float* cross, float* P, int L,
                              int d, int B, hipStream_t stream) {
  if (B <= 0) return;
  const int per = kDcnWpb * kDcnRows;
  const int want = (B + per - 1) / per;
  dim3 grid(want < kDcnFwdGrid ? want : kDcnFwdGrid);
  const size_t lds = (size_t)dcn_cross_lds_bytes(L, d);
  // requests above 64 KB of dynamic LDS have to be announced per kernel
  DISPATCH_DCN_L(
      L,
      if (lds > 64 * 1024) LCTR_CHECK_HIP(hipFuncSetAttribute(
          (const void*)dcn_cross_forward_kernel<LC>,
          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL((dcn_cross_forward_kernel<LC>), grid,
                         dim3(kDcnWpb * LCTR_WAVE), lds, stream,
                         (const unsigned short*)x0, Wc, u, q, cross, P, d,
                         B));
}

// partG: [dcn_cross_backward_chunks(B), L+1, d], partE: [chunks, L+1] of
// workspace. The three gradients are written for every B, as zeros for an
// empty batch.
void dcn_cross_backward_launch(const void* x0, const float* P,
                               const float* Wc, const float* u,
                               const float* q, const float* C,
                               const float* dpred, float* dDeep, float* partG,
                               float* partE, float* dWc, float* dbc,
                               float* du, int L, int d, int B,
                               hipStream_t stream) {
  const int nchunks = dcn_cross_backward_chunks(B);
  if (nchunks > 0) {
    dim3 grid((d + kDcnTile - 1) / kDcnTile, nchunks);
    DISPATCH_DCN_L(L, hipLaunchKernelGGL((dcn_cross_backward_kernel<LC>),
                                         grid, dim3(256), 0, stream,
                                         (const unsigned short*)x0, P, Wc, u,
                                         q, dpred, dDeep, partG, partE, d,
                                         B));
  }
  dim3 rgrid((d + kDcnRedCols - 1) / kDcnRedCols);
  DISPATCH_DCN_L(L, hipLaunchKernelGGL((dcn_cross_finish_kernel<LC>), rgrid,
                                       dim3(kDcnRedCols * kDcnRedSlices), 0,
                                       stream, partG, partE, Wc, u, C, dWc,
                                       dbc, du, d, nchunks));
}

}  // namespace lightctr

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
