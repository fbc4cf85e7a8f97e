// DCN-v2 cross term (Wang et al., "DCN V2", WWW 2021, low-rank matrix form)
// for MI355X/gfx950, on the concat row x0 (bf16 [B, d], d = nf*K) that the MLP
// reads. Parameters U[L, d, r], V[L, d, r], bc[L, d], u[d]:
//
//   T_l     = x_l V_l                 [B, r]
//   z_l     = T_l U_l^T + b_l         [B, d]
//   x_{l+1} = x0 . z_l + x_l          l = 0 .. L-1    (. elementwise)
//   cross   = x_L . u
//
// and backward, g_L = dpred (x) u, from the top layer down:
//
//   G_l  = g_{l+1} . x0               dbc_l = sum_rows G_l
//   dx0 += g_{l+1} . z_l              (z_l recomputed from the saved T_l)
//   S_l  = G_l U_l                    g_l = g_{l+1} + S_l V_l^T
//   dx0 += g_0                        du = sum_rows dpred X_L
//
// dU_l = G_l^T T_l and dV_l = X_l^T S_l are left to the GEMM (X_0 = x0).
//
// Tiling. A block of 4 waves owns 16 rows. The residual stream x_l (forward)
// and the row gradient g_l with dx0 (backward) are fp32 for the whole depth
// and live in MFMA accumulator fragments of v_mfma_f32_16x16x32_bf16: wave w
// owns the 16-column fragments 4 f + w, f < NF (NF = 4, 8, 12 or 16 by d, a
// template parameter; the depth L is a runtime loop). A fragment holds
// row 4 (lane >> 4) + i, column lane & 15 in element i of its lane. Neither
// ever goes to global memory in fp32.
//
// The two products of a layer alternate their roles: the wide one (K = d)
// reads its A operand, the bf16 image of the stream, from LDS and its B
// operand, 8 consecutive k of one column of V_l (U_l backward), straight
// from the transposed bf16 mirror [L, r, d] in L2; its [16, r] result is
// split over the waves by 16-column fragment, rounded to bf16 and left in
// LDS. The narrow one (K = r) reads that from LDS as A and rows of the
// row-major mirror [L, d, r] as B, and lands in the fragment layout of the
// stream, where the epilogue runs in registers. x0 stays in LDS as bf16 and
// is read per element by the epilogues. LDS rows are padded to the K step
// (32) with zeros, and by 8 more elements against bank conflicts; nothing
// in global memory is padded: loads past d or r are replaced by zeros.
//
// The backward is persistent (at most 1024 blocks walk the tiles), so that
// the column sums dbc and du are added tile after tile into an LDS vector by
// the lane that owns the column; each block leaves one partial [L+1, d] and
// dcn2_cross_finish adds the partials in 16 interleaved slices, each in block
// order, the slices in slice order. No float atomics: two runs are
// bit-identical in every output.
//
// Rounding points (everything else is fp32): T_l, as saved and as operand;
// X_l = x_l as saved and as operand of T_l = x_l V_l (x0 itself for l = 0);
// G_l and S_l, as saved and as operands. U and V are read from their bf16
// mirrors. dbc sums G_l before its rounding; du reads the saved X_L.
#include "common.h"

// No packed fp32 instructions (v_pk_add_f32 / v_pk_fma_f32) in this file:
// the device code is generated with scalar fp32 arithmetic only.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                     \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace lightctr {

typedef __attribute__((ext_vector_type(8))) __bf16 d2_bf16x8;
typedef __attribute__((ext_vector_type(4))) float d2_f32x4;
typedef unsigned short d2_bf;  // a bf16 as its bits

static constexpr int kD2Rows = 16;        // rows per tile
static constexpr int kD2RF = kD2Rows / 16;  // row fragments per tile
static constexpr int kD2Waves = 4;
static constexpr int kD2BwdGrid = 1024;   // backward: blocks at most
static constexpr int kD2RedCols = 16;     // finish: columns per block
static constexpr int kD2RedSlices = 16;   //         slices per column

extern __shared__ __align__(16) unsigned char d2_lds[];

static inline int d2_pad32(int n) { return (n + 31) & ~31; }

// dynamic LDS per block, the larger of the two kernels' (the backward's)
long dcn2_cross_lds_bytes(int L, int d, int r) {
  const long ds = d2_pad32(d) + 8, rs = d2_pad32(r) + 8;
  const long fwd = kD2Rows * (2 * ds + rs) * 2 + kD2Waves * kD2Rows * 4;
  const long bwd = kD2Rows * (2 * ds + 2 * rs) * 2 + (long)(L + 1) * d * 4;
  return fwd > bwd ? fwd : bwd;
}

int dcn2_cross_tile_rows() { return kD2Rows; }

int dcn2_cross_backward_blocks(int B) {
  const int tiles = B > 0 ? (B + kD2Rows - 1) / kD2Rows : 0;
  return tiles < kD2BwdGrid ? tiles : kD2BwdGrid;
}

// The runtime header's __shfl_xor and __syncthreads are compiled with packed
// fp32 on and would stay real calls from functions compiled without it, so
// the few this file needs are written on the builtins (as dcn_kernels.hip).
__device__ __forceinline__ float d2_shfl_xor(float v, int s) {
  const int lane =
      __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ s) << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ void d2_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float d2_bf2f(d2_bf v) {
  return __builtin_bit_cast(float, (unsigned)v << 16);
}

// round to nearest even; a NaN stays a NaN
__device__ __forceinline__ d2_bf d2_f2bf(float f) {
  const unsigned v = __builtin_bit_cast(unsigned, f);
  if ((v & 0x7fffffffu) > 0x7f800000u) return (d2_bf)((v >> 16) | 0x40u);
  return (d2_bf)((v + 0x7fffu + ((v >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ d2_bf16x8 d2_frag(uint4 v) {
  return __builtin_bit_cast(d2_bf16x8, v);
}

// B operand of a K = d product: elements ks .. ks+7 of a row of a [., d]
// mirror (d % 4 == 0, so a group of 4 is inside or outside), zeros past d
__device__ __forceinline__ d2_bf16x8 d2_load_kd(const d2_bf* __restrict__ row,
                                                int ks, int d) {
  uint2 lo = make_uint2(0u, 0u), hi = make_uint2(0u, 0u);
  if (ks < d) lo = *(const uint2*)(row + ks);
  if (ks + 4 < d) hi = *(const uint2*)(row + ks + 4);
  return d2_frag(make_uint4(lo.x, lo.y, hi.x, hi.y));
}

// B operand of a K = r product: elements ks .. ks+7 of row c of layer l of a
// [L, d, r] mirror (r % 16 == 0), zeros for c >= d or ks >= r
__device__ __forceinline__ d2_bf16x8 d2_load_kr(const d2_bf* __restrict__ W,
                                                int l, int c, int ks, int d,
                                                int r) {
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (c < d && ks < r)
    v = *(const uint4*)(W + ((size_t)l * d + c) * r + ks);
  return d2_frag(v);
}

// A operand: elements ks .. ks+7 of a row of an LDS image
__device__ __forceinline__ d2_bf16x8 d2_lds_frag(const d2_bf* s, int row,
                                                 int stride, int ks) {
  return d2_frag(*(const uint4*)(s + row * stride + ks));
}

// rows [0, nvalid) of a global [., w] bf16 matrix (w % 4 == 0) into the LDS
// image dst[16][stride]; the rest of the first wpad columns becomes zero
__device__ __forceinline__ void d2_load_tile(d2_bf* dst,
                                             const d2_bf* __restrict__ src,
                                             int nvalid, int w, int wpad,
                                             int stride) {
  const int g = wpad >> 2;
  for (int i = threadIdx.x; i < kD2Rows * g; i += blockDim.x) {
    const int m = i / g, c = (i - m * g) * 4;
    uint2 v = make_uint2(0u, 0u);
    if (m < nvalid && c < w) v = *(const uint2*)(src + (size_t)m * w + c);
    *(uint2*)(dst + m * stride + c) = v;
  }
}

// the first w columns of rows [0, nvalid) of an LDS image to global [., w]
__device__ __forceinline__ void d2_store_tile(d2_bf* __restrict__ dst,
                                              const d2_bf* src, int nvalid,
                                              int w, int stride) {
  const int g = w >> 2;
  for (int i = threadIdx.x; i < nvalid * g; i += blockDim.x) {
    const int m = i / g, c = (i - m * g) * 4;
    *(uint2*)(dst + (size_t)m * w + c) = *(const uint2*)(src + m * stride + c);
  }
}

__device__ __forceinline__ void d2_zero(d2_bf* dst, int n) {  // n % 4 == 0
  for (int i = threadIdx.x * 4; i < n; i += blockDim.x * 4)
    *(uint2*)(dst + i) = make_uint2(0u, 0u);
}

// The wide product: out[16, r] = A[16, d] W^T with W^T = Wt[l] ([r, d]); wave
// w takes the column fragments w, w + 4. A is the LDS image a; the result
// goes to the LDS image o as bf16.
__device__ __forceinline__ void d2_wide(const d2_bf* a, d2_bf* o,
                                        const d2_bf* __restrict__ Wt, int l,
                                        int d, int r, int dK, int ds, int rs,
                                        int wave, int lane) {
  const int lrow = lane & 15, lq = lane >> 4;
  for (int nt = wave; nt * 16 < r; nt += kD2Waves) {
    d2_f32x4 acc[kD2RF];
#pragma unroll
    for (int rf = 0; rf < kD2RF; ++rf) acc[rf] = d2_f32x4{0.f, 0.f, 0.f, 0.f};
    const d2_bf* wrow = Wt + ((size_t)l * r + nt * 16 + lrow) * d;
    for (int k0 = 0; k0 < dK; k0 += 32) {
      const int ks = k0 + lq * 8;
      const d2_bf16x8 b = d2_load_kd(wrow, ks, d);
#pragma unroll
      for (int rf = 0; rf < kD2RF; ++rf)
        acc[rf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            d2_lds_frag(a, rf * 16 + lrow, ds, ks), b, acc[rf], 0, 0, 0);
    }
#pragma unroll
    for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        o[(rf * 16 + lq * 4 + i) * rs + nt * 16 + lrow] = d2_f2bf(acc[rf][i]);
  }
}

// The narrow product on one column fragment: acc[16, 16] += A[16, r] W^T with
// W = Wm[l] ([d, r]) rows cb .. cb+15; A is the LDS image a
__device__ __forceinline__ void d2_narrow(d2_f32x4 (&acc)[kD2RF],
                                          const d2_bf* a,
                                          const d2_bf* __restrict__ Wm, int l,
                                          int cb, int d, int r, int rK,
                                          int rs, int lane) {
  const int lrow = lane & 15, lq = lane >> 4;
  for (int k0 = 0; k0 < rK; k0 += 32) {
    const int ks = k0 + lq * 8;
    const d2_bf16x8 b = d2_load_kr(Wm, l, cb + lrow, ks, d, r);
#pragma unroll
    for (int rf = 0; rf < kD2RF; ++rf)
      acc[rf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          d2_lds_frag(a, rf * 16 + lrow, rs, ks), b, acc[rf], 0, 0, 0);
  }
}

// sum over the 16 lanes of a fragment row (same lane >> 4)
__device__ __forceinline__ float d2_sum_cols(float v) {
#pragma unroll
  for (int s = 1; s < 16; s <<= 1) v += d2_shfl_xor(v, s);
  return v;
}

// sum over the 4 lanes of a fragment column (same lane & 15)
__device__ __forceinline__ float d2_sum_rows(float v) {
  v += d2_shfl_xor(v, 16);
  return v + d2_shfl_xor(v, 32);
}

template <int NF, bool SAVE>
__global__ __launch_bounds__(256) void dcn2_cross_forward_kernel(
    const d2_bf* __restrict__ x0, const d2_bf* __restrict__ Ubf,
    const d2_bf* __restrict__ Vtbf, const float* __restrict__ bc,
    const float* __restrict__ u, float* __restrict__ cross,
    d2_bf* __restrict__ X, d2_bf* __restrict__ T, int d, int r, int L,
    int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int dK = (d + 31) & ~31, ds = dK + 8;
  const int rK = (r + 31) & ~31, rs = rK + 8;
  d2_bf* x0s = (d2_bf*)d2_lds;        // [16][ds] x0
  d2_bf* xs = x0s + kD2Rows * ds;     // [16][ds] x_l, l >= 1
  d2_bf* ts = xs + kD2Rows * ds;      // [16][rs] T_l
  float* red = (float*)(ts + kD2Rows * rs);  // [4][16]
  const long row0 = (long)blockIdx.x * kD2Rows;
  const int nvalid = (int)(B - row0 < kD2Rows ? B - row0 : kD2Rows);

  d2_load_tile(x0s, x0 + (size_t)row0 * d, nvalid, d, dK, ds);
  d2_zero(xs, kD2Rows * ds);
  d2_zero(ts, kD2Rows * rs);
  d2_sync();

  d2_f32x4 x[kD2RF][NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int c = (f * kD2Waves + wave) * 16 + lrow;
#pragma unroll
    for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        x[rf][f][i] =
            c < d ? d2_bf2f(x0s[(rf * 16 + lq * 4 + i) * ds + c]) : 0.f;
  }

  for (int l = 0; l < L; ++l) {
    if (SAVE && l > 0)
      d2_store_tile(X + ((size_t)(l - 1) * B + row0) * d, xs, nvalid, d, ds);
    d2_wide(l == 0 ? x0s : xs, ts, Vtbf, l, d, r, dK, ds, rs, wave, lane);
    d2_sync();
    if (SAVE)
      d2_store_tile(T + ((size_t)l * B + row0) * r, ts, nvalid, r, rs);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int cb = (f * kD2Waves + wave) * 16, c = cb + lrow;
      if (cb >= d) continue;  // uniform over the wave
      d2_f32x4 z[kD2RF];
#pragma unroll
      for (int rf = 0; rf < kD2RF; ++rf) z[rf] = d2_f32x4{0.f, 0.f, 0.f, 0.f};
      d2_narrow(z, ts, Ubf, l, cb, d, r, rK, rs, lane);
      if (c < d) {
        const float bv = bc[(size_t)l * d + c];
#pragma unroll
        for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = rf * 16 + lq * 4 + i;
            const float v = fmaf(d2_bf2f(x0s[m * ds + c]), z[rf][i] + bv,
                                 x[rf][f][i]);
            x[rf][f][i] = v;
            xs[m * ds + c] = d2_f2bf(v);
          }
      }
    }
    d2_sync();
  }
  if (SAVE)
    d2_store_tile(X + ((size_t)(L - 1) * B + row0) * d, xs, nvalid, d, ds);

  // cross = x_L . u: a lane's columns in fragment order, then the 16 lanes of
  // a row, then the waves in wave order
  float p[kD2RF][4];
#pragma unroll
  for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) p[rf][i] = 0.f;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const int c = (f * kD2Waves + wave) * 16 + lrow;
    const float uv = c < d ? u[c] : 0.f;
#pragma unroll
    for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
      for (int i = 0; i < 4; ++i) p[rf][i] = fmaf(x[rf][f][i], uv, p[rf][i]);
  }
#pragma unroll
  for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = d2_sum_cols(p[rf][i]);
      if (lrow == 0) red[wave * kD2Rows + rf * 16 + lq * 4 + i] = s;
    }
  d2_sync();
  if ((int)threadIdx.x < nvalid) {
    const int m = threadIdx.x;
    cross[row0 + m] = ((red[m] + red[kD2Rows + m]) + red[2 * kD2Rows + m]) +
                      red[3 * kD2Rows + m];
  }
}

template <int NF>
__global__ __launch_bounds__(256) void dcn2_cross_backward_kernel(
    const d2_bf* __restrict__ x0, const d2_bf* __restrict__ X,
    const d2_bf* __restrict__ T, const d2_bf* __restrict__ Ubf,
    const d2_bf* __restrict__ Utbf, const d2_bf* __restrict__ Vbf,
    const float* __restrict__ bc, const float* __restrict__ u,
    const float* __restrict__ dpred, float* __restrict__ dDeep,
    d2_bf* __restrict__ G, d2_bf* __restrict__ S, float* __restrict__ part,
    int d, int r, int L, int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int dK = (d + 31) & ~31, ds = dK + 8;
  const int rK = (r + 31) & ~31, rs = rK + 8;
  d2_bf* x0s = (d2_bf*)d2_lds;        // [16][ds] x0
  d2_bf* gs = x0s + kD2Rows * ds;     // [16][ds] X_L, then G_l
  d2_bf* ts = gs + kD2Rows * ds;      // [16][rs] T_l
  d2_bf* ss = ts + kD2Rows * rs;      // [16][rs] S_l
  float* pacc = (float*)(ss + kD2Rows * rs);  // [L+1][d]: dbc, du of the block
  const int ntiles = (B + kD2Rows - 1) / kD2Rows;

  for (int i = threadIdx.x; i < (L + 1) * d; i += blockDim.x) pacc[i] = 0.f;
  d2_zero(ts, 2 * kD2Rows * rs);  // ts and ss: the columns past r stay zero

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long row0 = (long)tile * kD2Rows;
    const int nvalid = (int)(B - row0 < kD2Rows ? B - row0 : kD2Rows);
    d2_load_tile(x0s, x0 + (size_t)row0 * d, nvalid, d, dK, ds);
    d2_load_tile(gs, X + ((size_t)(L - 1) * B + row0) * d, nvalid, d, dK, ds);
    d2_sync();

    // g_L = dpred (x) u, dx0 = 0, du += dpred X_L. A wave reads and later
    // writes only its own columns of gs.
    float dp[kD2RF][4];
#pragma unroll
    for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = rf * 16 + lq * 4 + i;
        dp[rf][i] = m < nvalid ? dpred[row0 + m] : 0.f;
      }
    d2_f32x4 g[kD2RF][NF], dx[kD2RF][NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c = (f * kD2Waves + wave) * 16 + lrow;
      const float uv = c < d ? u[c] : 0.f;
      float s = 0.f;
#pragma unroll
      for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          g[rf][f][i] = dp[rf][i] * uv;
          dx[rf][f][i] = 0.f;
          if (c < d)
            s = fmaf(dp[rf][i],
                     d2_bf2f(gs[(rf * 16 + lq * 4 + i) * ds + c]), s);
        }
      s = d2_sum_rows(s);
      if (lq == 0 && c < d) pacc[(size_t)L * d + c] += s;
    }

    for (int l = L - 1; l >= 0; --l) {
      d2_load_tile(ts, T + ((size_t)l * B + row0) * r, nvalid, r, r, rs);
      // G_l = g . x0 into gs, its column sums into dbc_l
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int c = (f * kD2Waves + wave) * 16 + lrow;
        float s = 0.f;
        if (c < d) {
#pragma unroll
          for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int m = rf * 16 + lq * 4 + i;
              const float gv = g[rf][f][i] * d2_bf2f(x0s[m * ds + c]);
              gs[m * ds + c] = d2_f2bf(gv);
              s += gv;
            }
        }
        s = d2_sum_rows(s);
        if (lq == 0 && c < d) pacc[(size_t)l * d + c] += s;
      }
      d2_sync();
      d2_store_tile(G + ((size_t)l * B + row0) * d, gs, nvalid, d, ds);
      // S_l = G_l U_l into ss
      d2_wide(gs, ss, Utbf, l, d, r, dK, ds, rs, wave, lane);
      // dx0 += g . (T_l U_l^T + b_l)
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int cb = (f * kD2Waves + wave) * 16, c = cb + lrow;
        if (cb >= d) continue;  // uniform over the wave
        d2_f32x4 z[kD2RF];
#pragma unroll
        for (int rf = 0; rf < kD2RF; ++rf)
          z[rf] = d2_f32x4{0.f, 0.f, 0.f, 0.f};
        d2_narrow(z, ts, Ubf, l, cb, d, r, rK, rs, lane);
        const float bv = c < d ? bc[(size_t)l * d + c] : 0.f;
#pragma unroll
        for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            dx[rf][f][i] = fmaf(g[rf][f][i], z[rf][i] + bv, dx[rf][f][i]);
      }
      d2_sync();
      d2_store_tile(S + ((size_t)l * B + row0) * r, ss, nvalid, r, rs);
      // g_l = g_{l+1} + S_l V_l^T, accumulated onto the fragments of g
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const int cb = (f * kD2Waves + wave) * 16;
        if (cb >= d) continue;
        d2_f32x4 acc[kD2RF];
#pragma unroll
        for (int rf = 0; rf < kD2RF; ++rf) acc[rf] = g[rf][f];
        d2_narrow(acc, ss, Vbf, l, cb, d, r, rK, rs, lane);
#pragma unroll
        for (int rf = 0; rf < kD2RF; ++rf) g[rf][f] = acc[rf];
      }
    }

    // dDeep += dx0 + g_0
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int c = (f * kD2Waves + wave) * 16 + lrow;
      if (c >= d) continue;
#pragma unroll
      for (int rf = 0; rf < kD2RF; ++rf)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = rf * 16 + lq * 4 + i;
          if (m < nvalid) {
            float* p = dDeep + (size_t)(row0 + m) * d + c;
            *p += dx[rf][f][i] + g[rf][f][i];
          }
        }
    }
    d2_sync();  // the next tile refills x0s, gs and ts
  }
  d2_sync();
  float* out = part + (size_t)blockIdx.x * (L + 1) * d;
  for (int i = threadIdx.x; i < (L + 1) * d; i += blockDim.x) out[i] = pacc[i];
}

// out[j] = sum over the partials of part[k * n + j], j < n = (L+1) d: thread
// (sl, cl) adds partials sl, sl + 16, ... in that order, then the slices are
// added in slice order. j < nbc goes to dbc, the rest to du. Zeros when there
// are no partials.
__global__ __launch_bounds__(256) void dcn2_cross_finish_kernel(
    const float* __restrict__ part, float* __restrict__ dbc,
    float* __restrict__ du, int n, int nbc, int nparts) {
  __shared__ float red[kD2RedSlices][kD2RedCols];
  const int cl = threadIdx.x % kD2RedCols, sl = threadIdx.x / kD2RedCols;
  const int j = blockIdx.x * kD2RedCols + cl;
  float s = 0.f;
  if (j < n)
    for (int k = sl; k < nparts; k += kD2RedSlices)
      s += part[(size_t)k * n + j];
  red[sl][cl] = s;
  d2_sync();
  if (sl == 0 && j < n) {
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < kD2RedSlices; ++k) tot += red[k][cl];
    if (j < nbc) {
      dbc[j] = tot;
    } else {
      du[j - nbc] = tot;
    }
  }
}

// column fragments per wave that cover d: 4, 8, 12 or 16
#define DISPATCH_D2_NF(DVAL, ...)                                     \
  switch (((DVAL) + 255) / 256) {                                     \
    case 1: { constexpr int NFC = 4; __VA_ARGS__; break; }            \
    case 2: { constexpr int NFC = 8; __VA_ARGS__; break; }            \
    case 3: { constexpr int NFC = 12; __VA_ARGS__; break; }           \
    case 4: { constexpr int NFC = 16; __VA_ARGS__; break; }           \
    default:                                                          \
      fprintf(stderr, "lightctr_amd: unsupported cross width %d\n",   \
              DVAL);                                                  \
      abort();                                                        \
  }

// requests above 64 KB of dynamic LDS have to be announced per kernel
#define D2_ANNOUNCE_LDS(KERNEL, BYTES)                                \
  if ((BYTES) > 64 * 1024)                                            \
  LCTR_CHECK_HIP(hipFuncSetAttribute(                                 \
      (const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, \
      (int)(BYTES)))

// X [L, B, d] and T [L, B, r] are written when save is set and may be null
// otherwise
void dcn2_cross_forward_launch(const void* x0, const void* Ubf,
                               const void* Vtbf, const float* bc,
                               const float* u, float* cross, void* X, void* T,
                               bool save, int L, int d, int r, int B,
                               hipStream_t stream) {
  if (B <= 0) return;
  dim3 grid((B + kD2Rows - 1) / kD2Rows);
  const size_t lds = (size_t)dcn2_cross_lds_bytes(L, d, r);
#define D2_FWD(SAVE)                                                       \
  DISPATCH_D2_NF(                                                          \
      d, D2_ANNOUNCE_LDS((dcn2_cross_forward_kernel<NFC, SAVE>), lds);     \
      hipLaunchKernelGGL((dcn2_cross_forward_kernel<NFC, SAVE>), grid,     \
                         dim3(kD2Waves * LCTR_WAVE), lds, stream,          \
                         (const d2_bf*)x0, (const d2_bf*)Ubf,              \
                         (const d2_bf*)Vtbf, bc, u, cross, (d2_bf*)X,      \
                         (d2_bf*)T, d, r, L, B))
  if (save) {
    D2_FWD(true);
  } else {
    D2_FWD(false);
  }
#undef D2_FWD
}

// part: [dcn2_cross_backward_blocks(B), L+1, d] of workspace. dbc and du are
// written for every B, as zeros for an empty batch.
void dcn2_cross_backward_launch(const void* x0, const void* X, const void* T,
                                const void* Ubf, const void* Utbf,
                                const void* Vbf, const float* bc,
                                const float* u, const float* dpred,
                                float* dDeep, void* G, void* S, float* part,
                                float* dbc, float* du, int L, int d, int r,
                                int B, hipStream_t stream) {
  const int nblocks = dcn2_cross_backward_blocks(B);
  if (nblocks > 0) {
    const size_t lds = (size_t)dcn2_cross_lds_bytes(L, d, r);
    DISPATCH_D2_NF(
        d, D2_ANNOUNCE_LDS((dcn2_cross_backward_kernel<NFC>), lds);
        hipLaunchKernelGGL((dcn2_cross_backward_kernel<NFC>), dim3(nblocks),
                           dim3(kD2Waves * LCTR_WAVE), lds, stream,
                           (const d2_bf*)x0, (const d2_bf*)X, (const d2_bf*)T,
                           (const d2_bf*)Ubf, (const d2_bf*)Utbf,
                           (const d2_bf*)Vbf, bc, u, dpred, dDeep, (d2_bf*)G,
                           (d2_bf*)S, part, d, r, L, B));
  }
  const int n = (L + 1) * d;
  hipLaunchKernelGGL(dcn2_cross_finish_kernel,
                     dim3((n + kD2RedCols - 1) / kD2RedCols),
                     dim3(kD2RedCols * kD2RedSlices), 0, stream, part, dbc, du,
                     n, L * d, nblocks);
}

}  // namespace lightctr

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
