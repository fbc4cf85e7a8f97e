// Compressed Interaction Network of xDeepFM (Lian et al., KDD 2018) for
// MI355X/gfx950, on the concat row x0 (bf16 [B, nf*K]) that the MLP reads,
// viewed as X^0 [B, m = nf, D = K]. H_0 = m, H_l = H:
//
//   X^l[b,h,d] = sum_{i < H_{l-1}, j < m} W^l[h,i,j] X^{l-1}[b,i,d] x0[b,j,d]
//   cin[b]     = sum_l sum_h u[l,h] sum_d X^l[b,h,d]
//
// Rows. Every (b, d) pair is one row R = b K + d of a GEMM per layer,
// [B K, H_{l-1} m] x [H_{l-1} m, H], whose A operand is the outer product of
// two small per-row vectors and exists in registers only: a lane multiplies
// one stream scalar X^{l-1}[R, i] by 8 values x0[R, j], rounds the products
// to bf16 and hands them to v_mfma_f32_16x16x32_bf16.
//
// Reduction order ("kernel order") of a layer: j in groups of 8 (m padded to
// mp = 8 mg), i in blocks of 4 (H_{l-1} padded to 4 nib), so that one K step
// of 32 is (jg, ib) with the A fragment's lane group lq taking i = 4 ib + lq
// and its 8 elements j = 8 jg + jj:
//
//   kk = ((jg nib + ib) 4 + lq) 8 + jj        Kl = 32 mg nib columns
//
// The weights are held in that order, W^l as [H, Kl] (bf16 mirror Wbf) and
// transposed [Kl, H] (Wtbf), all layers in one flat buffer, pad columns at
// zero; their gradient is computed as zero, so the dense updaters keep them
// there.
//
// Forward: a block of 4 waves owns 128 rows, a wave 32 of them (2 row
// fragments) and all H columns (NT = H / 16 accumulator fragments, a template
// parameter). x0 and the stream stay in LDS as bf16 for the whole depth; W^l
// (330 KB at H = 64, m = 39) does not fit in LDS and is read as B fragments
// straight from L2, 16 bytes a lane, each fragment feeding both row
// fragments. The epilogue adds u[l,h] X^l[R,h] from the fp32 accumulators into
// a per-row sum, rounds X^l to bf16 into the LDS stream (and to global with
// SAVE); cin_rowsum adds the K row sums of a b in d order.
//
// Backward (data): the same tiles from the top layer down. dX^l (bf16, LDS)
// is the A operand of dZ = dX^l W^l (K = H, against Wtbf); a fragment of dZ
// is 2 values of i by 8 of j, and is contracted in the accumulators against
// x0 (summed over the j groups in the lane, then over the 8 lanes of an i)
// to dX^{l-1} and against X^{l-1} into per-lane dx0 partials that live in
// registers for the whole depth. dDeep += dx0 goes through LDS so that the
// global accesses run along d. du is a separate chunked column sum of
// dpred X^l over the saved X^l.
//
// Weight gradient: dW^l = dX^l^T Z with Z generated again from X^{l-1} and
// x0. A block owns a slab of 256 columns and a chunk of rows; 32 rows at a
// time go to LDS transposed, so that a lane reads its 8 rows of one column
// with one 16-byte load. Partials [chunks, H, Kl] are added in chunk order.
//
// No float atomics: every output is bit-identical from run to run.
//
// Rounding points (everything else is fp32): the generated product, once, to
// bf16; X^l and dX^l as saved and as operands; W from its bf16 mirrors. The
// row sums of cin read the fp32 accumulators; du reads the saved X^l.
#include "common.h"

// No packed fp32 instructions in this file (as dcn2_kernels.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                     \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace lightctr {

typedef __attribute__((ext_vector_type(8))) __bf16 cin_bf16x8;
typedef __attribute__((ext_vector_type(4))) float cin_f32x4;
typedef __attribute__((ext_vector_type(2))) __bf16 cin_bf16x2;
typedef __attribute__((ext_vector_type(2))) float cin_f32x2;
typedef unsigned short cin_bf;  // a bf16 as its bits

static constexpr int kCinRF = 2;      // row fragments per wave
static constexpr int kCinWaves = 4;
static constexpr int kCinWaveRows = 16 * kCinRF;
static constexpr int kCinRows = kCinWaveRows * kCinWaves;  // rows per tile
static constexpr int kCinWgRows = 32;    // wgrad: rows per step
static constexpr int kCinWgStride = 40;  //        LDS row stride (elements)
static constexpr int kCinWgFrags = 4;    //        column fragments per wave
static constexpr int kCinWgSlab = 16 * kCinWgFrags * kCinWaves;
static constexpr int kCinWgChunks = 128;  //       row chunks at most
static constexpr int kCinDuRows = 512;    // du: rows per block

extern __shared__ __align__(16) unsigned char cin_lds[];

int cin_tile_rows() { return kCinRows; }

static inline int cin_mp(int nf) { return (nf + 7) & ~7; }
static inline int cin_nib(int nf, int H, int l) {  // l = 1 .. L
  return l == 1 ? (nf + 3) / 4 : H / 4;
}

// columns of layer l's weight matrix in kernel order
long cin_layer_cols(int nf, int H, int l) {
  return 32L * (cin_mp(nf) / 8) * cin_nib(nf, H, l);
}

// elements of the flat weight buffer of L layers
long cin_weight_elems(int nf, int H, int L) {
  long n = 0;
  for (int l = 1; l <= L; ++l) n += (long)H * cin_layer_cols(nf, H, l);
  return n;
}

// dynamic LDS per block, the larger of the three kernels'
long cin_lds_bytes(int nf, int H) {
  const long mp = cin_mp(nf), s0 = mp + 8;
  const long hs = (H > mp ? H : mp) + 8, hk = ((H + 31) & ~31) + 8;
  const long fwd = kCinRows * (s0 + hs) * 2;
  const long bwd = kCinRows * (s0 + hs + hk) * 2 + kCinRows * (mp + 1) * 4;
  const long wg = (mp + 2L * H) * kCinWgStride * 2;
  return bwd > fwd ? (bwd > wg ? bwd : wg) : (fwd > wg ? fwd : wg);
}

int cin_wgrad_chunk_rows(long BK) {
  long per = (BK + kCinWgChunks - 1) / kCinWgChunks;
  per = (per + kCinWgRows - 1) / kCinWgRows * kCinWgRows;
  return (int)(per > 0 ? per : kCinWgRows);
}

int cin_wgrad_chunks(long BK) {
  const long c = cin_wgrad_chunk_rows(BK);
  return (int)((BK + c - 1) / c);
}

int cin_du_chunks(long BK) { return (int)((BK + kCinDuRows - 1) / kCinDuRows); }

__device__ __forceinline__ float cin_shfl_xor(float v, int s) {
  const int lane =
      __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ s) << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ void cin_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float cin_bf2f(cin_bf v) {
  return __builtin_bit_cast(float, (unsigned)v << 16);
}

// round to nearest even; a NaN stays a NaN
__device__ __forceinline__ cin_bf cin_f2bf(float f) {
  const unsigned v = __builtin_bit_cast(unsigned, f);
  if ((v & 0x7fffffffu) > 0x7f800000u) return (cin_bf)((v >> 16) | 0x40u);
  return (cin_bf)((v + 0x7fffu + ((v >> 16) & 1u)) >> 16);
}

// the 8 bf16 of a 16-byte load as floats
__device__ __forceinline__ void cin_unpack(uint4 v, float (&f)[8]) {
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f[2 * t] = __builtin_bit_cast(float, w[t] << 16);
    f[2 * t + 1] = __builtin_bit_cast(float, w[t] & 0xffff0000u);
  }
}

// two floats to a bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned cin_pack2(float lo, float hi) {
  const cin_f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, cin_bf16x2));
}

// the generated operand: s * x[0..7], each product rounded once to bf16
__device__ __forceinline__ cin_bf16x8 cin_outer(float s, const float (&x)[8]) {
  unsigned w[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) w[t] = cin_pack2(s * x[2 * t], s * x[2 * t + 1]);
  return __builtin_bit_cast(cin_bf16x8, make_uint4(w[0], w[1], w[2], w[3]));
}

// the same for two vectors of 8: a[t] * b[t]
__device__ __forceinline__ cin_bf16x8 cin_prod(const float (&a)[8],
                                               const float (&b)[8]) {
  unsigned w[4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
    w[t] = cin_pack2(a[2 * t] * b[2 * t], a[2 * t + 1] * b[2 * t + 1]);
  return __builtin_bit_cast(cin_bf16x8, make_uint4(w[0], w[1], w[2], w[3]));
}

__device__ __forceinline__ cin_bf16x8 cin_frag(uint4 v) {
  return __builtin_bit_cast(cin_bf16x8, v);
}

// x0[b, j K + d] of rows R = row0 .. row0 + nrows - 1 (R = b K + d, R < rend)
// into dst[row * rs + j * js], j < mp; zeros for j >= nf and rows past rend
__device__ __forceinline__ void cin_load_x0(cin_bf* dst,
                                            const cin_bf* __restrict__ x0,
                                            long row0, long rend, int nrows,
                                            int nf, int K, int mp, int rs,
                                            int js) {
  for (int idx = threadIdx.x; idx < mp * nrows; idx += blockDim.x) {
    const int j = idx / nrows, row = idx - j * nrows;
    const long R = row0 + row;
    cin_bf v = 0;
    if (R < rend && j < nf) {
      const int b = (int)R / K;  // R < 2^24
      v = x0[(size_t)b * nf * K + (size_t)j * K + ((int)R - b * K)];
    }
    dst[row * rs + j * js] = v;
  }
}

template <int NT, bool SAVE>
__global__ __launch_bounds__(256) void cin_forward_kernel(
    const cin_bf* __restrict__ x0, const cin_bf* __restrict__ Wbf,
    const float* __restrict__ u, float* __restrict__ crow,
    cin_bf* __restrict__ X, int nf, int K, int L, long BK) {
  constexpr int H = 16 * NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int mp = (nf + 7) & ~7, mg = mp >> 3, s0 = mp + 8;
  const int hs = (H > mp ? H : mp) + 8;
  cin_bf* x0s = (cin_bf*)cin_lds;       // [128][s0] x0
  cin_bf* st = x0s + kCinRows * s0;     // [128][hs] X^l, l >= 1
  const long row0 = (long)blockIdx.x * kCinRows;
  const int nvalid = (int)(BK - row0 < kCinRows ? BK - row0 : kCinRows);
  const int wbase = wave * kCinWaveRows;

  cin_load_x0(x0s, x0, row0, BK, kCinRows, nf, K, mp, s0, 1);
  cin_sync();

  float c[kCinRF][4];
#pragma unroll
  for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) c[rf][i] = 0.f;

  const cin_bf* Wl = Wbf;
  for (int l = 1; l <= L; ++l) {
    const cin_bf* src = l == 1 ? x0s : st;
    const int ss = l == 1 ? s0 : hs;
    const int nib = l == 1 ? (nf + 3) >> 2 : H >> 2;
    const int Kl = 32 * mg * nib;
    cin_f32x4 acc[kCinRF][NT];
#pragma unroll
    for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[rf][nt] = cin_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int jg = 0; jg < mg; ++jg) {
      float xf[kCinRF][8];
#pragma unroll
      for (int rf = 0; rf < kCinRF; ++rf)
        cin_unpack(*(const uint4*)(x0s + (wbase + rf * 16 + lrow) * s0 +
                                   jg * 8), xf[rf]);
      const cin_bf* wk = Wl + (size_t)lrow * Kl + (size_t)jg * nib * 32 +
                         lq * 8;
      for (int ib = 0; ib < nib; ++ib) {
        cin_bf16x8 a[kCinRF];
#pragma unroll
        for (int rf = 0; rf < kCinRF; ++rf)
          a[rf] = cin_outer(
              cin_bf2f(src[(wbase + rf * 16 + lrow) * ss + ib * 4 + lq]),
              xf[rf]);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const cin_bf16x8 b = cin_frag(
              *(const uint4*)(wk + (size_t)nt * 16 * Kl + ib * 32));
#pragma unroll
          for (int rf = 0; rf < kCinRF; ++rf)
            acc[rf][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a[rf], b, acc[rf][nt], 0, 0, 0);
        }
      }
    }
    cin_sync();  // every read of the stream is done before it is replaced
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const float uv = u[(l - 1) * H + nt * 16 + lrow];
#pragma unroll
      for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = acc[rf][nt][i];
          c[rf][i] = fmaf(v, uv, c[rf][i]);
          st[(wbase + rf * 16 + lq * 4 + i) * hs + nt * 16 + lrow] =
              cin_f2bf(v);
        }
    }
    cin_sync();
    if (SAVE) {
      cin_bf* out = X + ((size_t)(l - 1) * BK + row0) * H;
      for (int idx = threadIdx.x; idx < nvalid * (H / 8); idx += blockDim.x) {
        const int row = idx / (H / 8), g = idx - row * (H / 8);
        *(uint4*)(out + (size_t)row * H + g * 8) =
            *(const uint4*)(st + row * hs + g * 8);
      }
    }
    Wl += (size_t)H * Kl;
  }

  // the row's sum over the 16 lanes of a fragment row
#pragma unroll
  for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float s = c[rf][i];
#pragma unroll
      for (int sh = 1; sh < 16; sh <<= 1) s += cin_shfl_xor(s, sh);
      const long R = row0 + wbase + rf * 16 + lq * 4 + i;
      if (lrow == 0 && R < BK) crow[R] = s;
    }
}

// cin[b] = sum_d crow[b K + d], in d order
__global__ __launch_bounds__(256) void cin_rowsum_kernel(
    const float* __restrict__ crow, float* __restrict__ cin, int K, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float s = 0.f;
  for (int d = 0; d < K; ++d) s += crow[(size_t)b * K + d];
  cin[b] = s;
}

template <int NT>
__global__ __launch_bounds__(256) void cin_backward_kernel(
    const cin_bf* __restrict__ x0, const cin_bf* __restrict__ X,
    const cin_bf* __restrict__ Wtbf, const float* __restrict__ u,
    const float* __restrict__ dpred, float* __restrict__ dDeep,
    cin_bf* __restrict__ dX, int nf, int K, int L, long BK) {
  constexpr int H = 16 * NT, KS = (NT + 1) / 2, HK = 32 * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int mp = (nf + 7) & ~7, mg = mp >> 3, s0 = mp + 8;
  const int hs = (H > mp ? H : mp) + 8, hk = HK + 8, fs = mp + 1;
  cin_bf* x0s = (cin_bf*)cin_lds;       // [128][s0] x0
  cin_bf* xs = x0s + kCinRows * s0;     // [128][hs] X^{l-1}, l >= 2
  cin_bf* dxs = xs + kCinRows * hs;     // [128][hk] dX^l
  float* dx0s = (float*)(dxs + kCinRows * hk);  // [128][fs] dX^0, then dx0
  const long row0 = (long)blockIdx.x * kCinRows;
  const int nvalid = (int)(BK - row0 < kCinRows ? BK - row0 : kCinRows);
  const int wbase = wave * kCinWaveRows;

  cin_load_x0(x0s, x0, row0, BK, kCinRows, nf, K, mp, s0, 1);
  for (int idx = threadIdx.x; idx < kCinRows * fs; idx += blockDim.x)
    dx0s[idx] = 0.f;
  // dX^L = dpred (x) u[L]; the columns past H stay zero for the whole depth
  for (int idx = threadIdx.x; idx < kCinRows * HK; idx += blockDim.x) {
    const int row = idx / HK, h = idx - row * HK;
    const long R = row0 + row;
    float v = 0.f;
    if (R < BK && h < H) v = dpred[(int)R / K] * u[(L - 1) * H + h];
    dxs[row * hk + h] = cin_f2bf(v);
  }
  float dp[kCinRF][4];
#pragma unroll
  for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long R = row0 + wbase + rf * 16 + lq * 4 + i;
      dp[rf][i] = R < BK ? dpred[(int)R / K] : 0.f;
    }
  float tx0[8][kCinRF][4];
#pragma unroll
  for (int jg = 0; jg < 8; ++jg)
#pragma unroll
    for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
      for (int i = 0; i < 4; ++i) tx0[jg][rf][i] = 0.f;

  // offset of layer L's [Kl, H] block in the flat transposed mirror
  size_t woff = 0;
  for (int l = 1; l < L; ++l)
    woff += (size_t)H * 32 * mg * (l == 1 ? (nf + 3) >> 2 : H >> 2);

  for (int l = L; l >= 1; --l) {
    const int nib = l == 1 ? (nf + 3) >> 2 : H >> 2;
    cin_sync();  // dxs holds dX^l
    {
      cin_bf* out = dX + ((size_t)(l - 1) * BK + row0) * H;
      for (int idx = threadIdx.x; idx < nvalid * (H / 8); idx += blockDim.x) {
        const int row = idx / (H / 8), g = idx - row * (H / 8);
        *(uint4*)(out + (size_t)row * H + g * 8) =
            *(const uint4*)(dxs + row * hk + g * 8);
      }
    }
    if (l >= 2) {
      const cin_bf* in = X + ((size_t)(l - 2) * BK + row0) * H;
      for (int idx = threadIdx.x; idx < kCinRows * (H / 8);
           idx += blockDim.x) {
        const int row = idx / (H / 8), g = idx - row * (H / 8);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (row < nvalid) v = *(const uint4*)(in + (size_t)row * H + g * 8);
        *(uint4*)(xs + row * hs + g * 8) = v;
      }
    }
    cin_sync();
    const cin_bf* src = l == 1 ? x0s : xs;
    const int ss = l == 1 ? s0 : hs;
    cin_bf16x8 a[kCinRF][KS];
#pragma unroll
    for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        a[rf][ks] = cin_frag(*(const uint4*)(
            dxs + (wbase + rf * 16 + lrow) * hk + ks * 32 + lq * 8));
    const cin_bf* Wt = Wtbf + woff;  // [Kl, H]
    for (int ib = 0; ib < nib; ++ib)
      for (int half = 0; half < 2; ++half) {
        const int li = ib * 4 + half * 2 + (lrow >> 3);  // the lane's i
        float xv[kCinRF][4], tX[kCinRF][4];
#pragma unroll
        for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            xv[rf][i] =
                cin_bf2f(src[(wbase + rf * 16 + lq * 4 + i) * ss + li]);
            tX[rf][i] = 0.f;
          }
#pragma unroll
        for (int jg = 0; jg < 8; ++jg) {
          if (jg >= mg) break;  // uniform
          const size_t n = (size_t)(jg * nib + ib) * 32 + half * 16 + lrow;
          cin_f32x4 acc[kCinRF];
#pragma unroll
          for (int rf = 0; rf < kCinRF; ++rf)
            acc[rf] = cin_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            uint4 bv = make_uint4(0u, 0u, 0u, 0u);
            if (ks * 32 + lq * 8 < H)
              bv = *(const uint4*)(Wt + n * H + ks * 32 + lq * 8);
#pragma unroll
            for (int rf = 0; rf < kCinRF; ++rf)
              acc[rf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  a[rf][ks], cin_frag(bv), acc[rf], 0, 0, 0);
          }
#pragma unroll
          for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float xj = cin_bf2f(x0s[(wbase + rf * 16 + lq * 4 + i) *
                                                s0 + jg * 8 + (lrow & 7)]);
              tX[rf][i] = fmaf(acc[rf][i], xj, tX[rf][i]);
              tx0[jg][rf][i] = fmaf(acc[rf][i], xv[rf][i], tx0[jg][rf][i]);
            }
        }
#pragma unroll
        for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float s = tX[rf][i];
#pragma unroll
            for (int sh = 1; sh < 8; sh <<= 1) s += cin_shfl_xor(s, sh);
            const int row = wbase + rf * 16 + lq * 4 + i;
            if ((lrow & 7) == 0) {
              if (l >= 2) {  // dX^{l-1}, over the A fragments read above
                dxs[row * hk + li] =
                    cin_f2bf(fmaf(dp[rf][i], u[(l - 2) * H + li], s));
              } else if (li < mp) {  // layer 1's other factor is x0 too
                dx0s[row * fs + li] = s;
              }
            }
          }
      }
    if (l >= 2)
      woff -= (size_t)H * 32 * mg * (l == 2 ? (nf + 3) >> 2 : H >> 2);
  }

  cin_sync();
#pragma unroll
  for (int jg = 0; jg < 8; ++jg) {
    if (jg >= mg) break;
#pragma unroll
    for (int rf = 0; rf < kCinRF; ++rf)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float v = tx0[jg][rf][i];
        v += cin_shfl_xor(v, 8);  // the two parities of i
        if (lrow < 8)
          dx0s[(wbase + rf * 16 + lq * 4 + i) * fs + jg * 8 + lrow] += v;
      }
  }
  cin_sync();
  for (int idx = threadIdx.x; idx < nf * kCinRows; idx += blockDim.x) {
    const int j = idx / kCinRows, row = idx - j * kCinRows;
    const long R = row0 + row;
    if (R < BK) {
      const int b = (int)R / K;
      dDeep[(size_t)b * nf * K + (size_t)j * K + ((int)R - b * K)] +=
          dx0s[row * fs + j];
    }
  }
}

// part[chunk, l, h] = sum over the chunk's rows of dpred[b] X^l[R, h]
__global__ __launch_bounds__(128) void cin_du_kernel(
    const cin_bf* __restrict__ X, const float* __restrict__ dpred,
    float* __restrict__ part, int K, int H, int L, long BK) {
  const int h = threadIdx.x;
  if (h >= H) return;
  const long r0 = (long)blockIdx.x * kCinDuRows;
  const long r1 = r0 + kCinDuRows < BK ? r0 + kCinDuRows : BK;
  for (int l = 0; l < L; ++l) {
    float s = 0.f;
    for (long R = r0; R < r1; ++R)
      s = fmaf(dpred[(int)R / K], cin_bf2f(X[((size_t)l * BK + R) * H + h]), s);
    part[((size_t)blockIdx.x * L + l) * H + h] = s;
  }
}

// out[j] = sum_k part[k n + j], k = 0 .. nparts - 1 in that order
__global__ __launch_bounds__(256) void cin_sum_parts_kernel(
    const float* __restrict__ part, float* __restrict__ out, long n,
    int nparts) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(size_t)k * n + j];
  out[j] = s;
}

// One layer's weight gradient: part[chunk, h, kk] over the chunk's rows.
// Xp is X^{l-1} [BK, H] for l >= 2 and null for l = 1 (X^0 = x0).
template <int NT>
__global__ __launch_bounds__(256) void cin_wgrad_kernel(
    const cin_bf* __restrict__ x0, const cin_bf* __restrict__ Xp,
    const cin_bf* __restrict__ dXl, float* __restrict__ part, int nf, int K,
    int nib, long BK, int chunk_rows) {
  constexpr int H = 16 * NT, WS = kCinWgStride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int mp = (nf + 7) & ~7, mg = mp >> 3;
  const int Kl = 32 * mg * nib;
  cin_bf* x0T = (cin_bf*)cin_lds;   // [mp][WS]
  cin_bf* dXT = x0T + mp * WS;      // [H][WS]
  cin_bf* XT = dXT + H * WS;        // [H][WS], l >= 2
  const cin_bf* iT = Xp ? XT : x0T;
  const long rbeg = (long)blockIdx.y * chunk_rows;
  const long rend = rbeg + chunk_rows < BK ? rbeg + chunk_rows : BK;

  // the lane's column of each of the wave's fragments: its i and j rows
  int ioff[kCinWgFrags], joff[kCinWgFrags];
#pragma unroll
  for (int f = 0; f < kCinWgFrags; ++f) {
    int n = blockIdx.x * kCinWgSlab + (wave * kCinWgFrags + f) * 16 + lrow;
    if (n >= Kl) n = 0;  // the fragment is skipped below
    const int rest = n >> 5, jg = rest / nib, ib = rest - jg * nib;
    ioff[f] = (ib * 4 + ((n >> 3) & 3)) * WS + lq * 8;
    joff[f] = (jg * 8 + (n & 7)) * WS + lq * 8;
  }
  cin_f32x4 acc[kCinWgFrags][NT];
#pragma unroll
  for (int f = 0; f < kCinWgFrags; ++f)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      acc[f][nt] = cin_f32x4{0.f, 0.f, 0.f, 0.f};

  for (long r0 = rbeg; r0 < rend; r0 += kCinWgRows) {
    cin_sync();  // the last step's reads are done
    cin_load_x0(x0T, x0, r0, rend, kCinWgRows, nf, K, mp, 1, WS);
    for (int idx = threadIdx.x; idx < kCinWgRows * H; idx += blockDim.x) {
      const int row = idx / H, h = idx - row * H;
      const long R = r0 + row;
      dXT[h * WS + row] = R < rend ? dXl[(size_t)R * H + h] : (cin_bf)0;
      if (Xp) XT[h * WS + row] = R < rend ? Xp[(size_t)R * H + h] : (cin_bf)0;
    }
    cin_sync();
    cin_bf16x8 a[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      a[nt] = cin_frag(
          *(const uint4*)(dXT + (nt * 16 + lrow) * WS + lq * 8));
#pragma unroll
    for (int f = 0; f < kCinWgFrags; ++f) {
      const int n0 = blockIdx.x * kCinWgSlab + (wave * kCinWgFrags + f) * 16;
      if (n0 >= Kl) continue;  // uniform over the wave
      float xi[8], xj[8];
      cin_unpack(*(const uint4*)(iT + ioff[f]), xi);
      cin_unpack(*(const uint4*)(x0T + joff[f]), xj);
      const cin_bf16x8 b = cin_prod(xi, xj);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
        acc[f][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            a[nt], b, acc[f][nt], 0, 0, 0);
    }
  }
  float* out = part + (size_t)blockIdx.y * H * Kl;
#pragma unroll
  for (int f = 0; f < kCinWgFrags; ++f) {
    const int n0 = blockIdx.x * kCinWgSlab + (wave * kCinWgFrags + f) * 16;
    if (n0 >= Kl) continue;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        out[(size_t)(nt * 16 + lq * 4 + i) * Kl + n0 + lrow] = acc[f][nt][i];
  }
}

// accumulator fragments that cover H: 1 .. 8
#define DISPATCH_CIN_NT(HVAL, ...)                                    \
  switch ((HVAL) / 16) {                                              \
    case 1: { constexpr int NTC = 1; __VA_ARGS__; break; }            \
    case 2: { constexpr int NTC = 2; __VA_ARGS__; break; }            \
    case 3: { constexpr int NTC = 3; __VA_ARGS__; break; }            \
    case 4: { constexpr int NTC = 4; __VA_ARGS__; break; }            \
    case 5: { constexpr int NTC = 5; __VA_ARGS__; break; }            \
    case 6: { constexpr int NTC = 6; __VA_ARGS__; break; }            \
    case 7: { constexpr int NTC = 7; __VA_ARGS__; break; }            \
    case 8: { constexpr int NTC = 8; __VA_ARGS__; break; }            \
    default:                                                          \
      fprintf(stderr, "lightctr_amd: unsupported cin maps %d\n",      \
              HVAL);                                                  \
      abort();                                                        \
  }

// requests above 64 KB of dynamic LDS have to be announced per kernel
#define CIN_ANNOUNCE_LDS(KERNEL, BYTES)                               \
  if ((BYTES) > 64 * 1024)                                            \
  LCTR_CHECK_HIP(hipFuncSetAttribute(                                 \
      (const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, \
      (int)(BYTES)))

// crow: [B K] of workspace. X [L, B K, H] is written when save is set and may
// be null otherwise.
void cin_forward_launch(const void* x0, const void* Wbf, const float* u,
                        float* crow, float* cin, void* X, bool save, int nf,
                        int K, int H, int L, int B, hipStream_t stream) {
  if (B <= 0) return;
  const long BK = (long)B * K;
  dim3 grid((unsigned)((BK + kCinRows - 1) / kCinRows));
  const size_t lds = (size_t)cin_lds_bytes(nf, H);
#define CIN_FWD(SAVE)                                                     \
  DISPATCH_CIN_NT(                                                        \
      H, CIN_ANNOUNCE_LDS((cin_forward_kernel<NTC, SAVE>), lds);          \
      hipLaunchKernelGGL((cin_forward_kernel<NTC, SAVE>), grid,           \
                         dim3(kCinWaves * LCTR_WAVE), lds, stream,        \
                         (const cin_bf*)x0, (const cin_bf*)Wbf, u, crow,  \
                         (cin_bf*)X, nf, K, L, BK))
  if (save) {
    CIN_FWD(true);
  } else {
    CIN_FWD(false);
  }
#undef CIN_FWD
  hipLaunchKernelGGL(cin_rowsum_kernel, dim3((B + 255) / 256), dim3(256), 0,
                     stream, crow, cin, K, B);
}

// part: [cin_du_chunks(B K), L, H] of workspace. du is written for every B,
// as zeros for an empty batch.
void cin_backward_launch(const void* x0, const void* X, const void* Wtbf,
                         const float* u, const float* dpred, float* dDeep,
                         void* dX, float* part, float* du, int nf, int K,
                         int H, int L, int B, hipStream_t stream) {
  const long BK = (long)B * K;
  const int nparts = cin_du_chunks(BK);
  if (B > 0) {
    dim3 grid((unsigned)((BK + kCinRows - 1) / kCinRows));
    const size_t lds = (size_t)cin_lds_bytes(nf, H);
    DISPATCH_CIN_NT(
        H, CIN_ANNOUNCE_LDS((cin_backward_kernel<NTC>), lds);
        hipLaunchKernelGGL((cin_backward_kernel<NTC>), grid,
                           dim3(kCinWaves * LCTR_WAVE), lds, stream,
                           (const cin_bf*)x0, (const cin_bf*)X,
                           (const cin_bf*)Wtbf, u, dpred, dDeep, (cin_bf*)dX,
                           nf, K, L, BK));
    hipLaunchKernelGGL(cin_du_kernel, dim3(nparts), dim3(128), 0, stream,
                       (const cin_bf*)X, dpred, part, K, H, L, BK);
  }
  const long n = (long)L * H;
  hipLaunchKernelGGL(cin_sum_parts_kernel, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, stream, part, du, n, nparts);
}

// part: [cin_wgrad_chunks(B K), H, max Kl] of workspace; dW: the flat
// gradient in kernel order, zeros for an empty batch
void cin_wgrad_launch(const void* x0, const void* X, const void* dX,
                      float* part, float* dW, int nf, int K, int H, int L,
                      int B, hipStream_t stream) {
  const long BK = (long)B * K;
  const int nchunks = B > 0 ? cin_wgrad_chunks(BK) : 0;
  const int chunk_rows = cin_wgrad_chunk_rows(BK);
  const size_t lds = (size_t)cin_lds_bytes(nf, H);
  for (int l = 1; l <= L; ++l) {
    const int nib = cin_nib(nf, H, l);
    const long Kl = cin_layer_cols(nf, H, l), n = (long)H * Kl;
    if (nchunks > 0) {
      dim3 grid((unsigned)((Kl + kCinWgSlab - 1) / kCinWgSlab), nchunks);
      const cin_bf* Xp =
          l == 1 ? nullptr : (const cin_bf*)X + (size_t)(l - 2) * BK * H;
      const cin_bf* dXl = (const cin_bf*)dX + (size_t)(l - 1) * BK * H;
      DISPATCH_CIN_NT(
          H, CIN_ANNOUNCE_LDS((cin_wgrad_kernel<NTC>), lds);
          hipLaunchKernelGGL((cin_wgrad_kernel<NTC>), grid,
                             dim3(kCinWaves * LCTR_WAVE), lds, stream,
                             (const cin_bf*)x0, Xp, dXl, part, nf, K, nib, BK,
                             chunk_rows));
    }
    hipLaunchKernelGGL(cin_sum_parts_kernel,
                       dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       stream, part, dW, n, nchunks);
    dW += n;
  }
}

}  // namespace lightctr

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
