// AutoInt (Song et al., CIKM 2019) for MI355X/gfx950: multi-head self-attention
// over the field embeddings of the concat row x0 (bf16 [B, nf*K]) that the MLP
// reads, viewed as X^0 [B, nf, K]. D = heads * head_dim, d_0 = K, d_l = D:
//
//   P   = X^{l-1} W^l          W^l [d_{l-1}, 4D], columns [Q | K | V | R]
//   S_h = Q_h K_h^T            per head, unscaled
//   A_h = softmax over keys (S_h)
//   X^l = relu(concat_h(A_h V_h) + R)
//   ai[b] = sum_{m,c} u[m,c] X^L[b,m,c]
//
// Work split. An example is nf <= 64 tokens, MT = ceil(nf / 16) MFMA row
// fragments (a template parameter); a wave owns whole examples and never
// synchronises with the other waves of its block after the weights are
// staged. A block takes tiles of 16 consecutive examples, its waves the
// examples of a tile in turn. The number of waves (1 .. 4) is what the LDS
// holds beside the weights.
//
// Every product is v_mfma_f32_16x16x32_bf16 on two LDS operands held with the
// contraction index contiguous (ai_mma): 16 bytes a lane and operand, the
// groups of 8 past the contraction length given as zeros.
//
// Forward, one launch for all L layers: every W^l is staged once per block,
// transposed ([4D][d_in], d_in padded with zeros to a multiple of 8). Per
// example and layer: Q, K (token rows) and V (transposed, keys contiguous)
// are rounded to bf16 into the wave's LDS; per row fragment the accumulators
// start from the R projection, and per head the scores S[q][key] of the 16
// queries against all keys sit in MT accumulator fragments of the lane (keys
// across the 16 lanes of a row, MT key fragments in the lane), so the softmax
// is MT values in the lane plus 4 cross-lane steps. Keys >= nf are -inf,
// A goes as bf16 through a [16][nf] LDS tile into A V, which lands in the same
// accumulators as R. ReLU, the product with u (top layer) and the rounding
// of X^l happen there; X^l replaces X^{l-1} in place (rows >= nf as zeros).
//
// Backward, one launch a layer from the top down (a layer's W in both
// orientations in LDS): Q, K, V, S and A are recomputed from the saved
// X^{l-1}; dY = dX^l masked by X^l > 0 (the top layer's dX^L = dpred u is
// formed here, a lower layer's comes from the launch above as bf16);
// dA = dY V^T, dS = A (dA - rowsum(A dA)), dQ = dS K, dK = dS^T Q,
// dV = A^T dY, each overwriting the operand it no longer needs, then
// [dQ | dK | dV | dY] goes to global as bf16 (the weight gradient's operand)
// and dX^{l-1} = [dQ | dK | dV | dY] W^T either adds into dDeep (l = 1, fp32)
// or is masked by X^{l-1} > 0, rounded and handed to the next launch.
//
// Weight gradient: dW^l = X^{l-1 T} [dQ | dK | dV | dY] over all B nf tokens,
// 32 tokens at a time transposed through LDS, a chunk of tokens a block,
// partials [chunks, d_in, 4D] added in chunk order. du the same way over
// chunks of 64 examples. No float atomics: every output is bit-identical
// from run to run.
//
// Rounding points (everything else is fp32): x0, X^l, W; Q, K, V, A, dY, dS,
// dQ, dK, dV once each. ai reads the fp32 top layer, du the saved one.
#include "common.h"

// No packed fp32 instructions in this file (as cin_kernels.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                     \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace lightctr {

typedef __attribute__((ext_vector_type(8))) __bf16 ai_bf16x8;
typedef __attribute__((ext_vector_type(4))) float ai_f32x4;
typedef unsigned short ai_bf;  // a bf16 as its bits

static constexpr int kAiTile = 16;       // examples per block tile
static constexpr int kAiMaxWaves = 4;
static constexpr int kAiMaxBlocks = 1024;
static constexpr int kAiWgRows = 32;     // wgrad: tokens per step
static constexpr int kAiWgStride = 40;   //        LDS row stride (elements)
static constexpr int kAiWgChunks = 256;  //        token chunks at most
static constexpr int kAiDuRows = 64;     // du: examples per block
static constexpr long kAiLdsMax = 160 * 1024;

extern __shared__ __align__(16) unsigned char ai_lds[];

int autoint_tile_rows() { return kAiTile; }

static inline int ai_up(int v, int m) { return (v + m - 1) / m * m; }
static inline int ai_kv(int K, int D, int l) {  // l = 0 .. L-1
  return l == 0 ? ai_up(K, 8) : D;
}
static inline int ai_sx(int K, int D) {
  const int a = ai_up(K, 8);
  return (a > D ? a : D) + 8;
}

// bf16 elements of the forward's staged weights / of one wave's buffers
static long ai_fwd_w(int K, int D, int L) {
  long n = 0;
  for (int l = 0; l < L; ++l) n += 4L * D * (ai_kv(K, D, l) + 8);
  return n;
}
static long ai_fwd_wave(int nf, int K, int D) {
  const long NP = ai_up(nf, 16);
  return NP * ai_sx(K, D) + 2 * NP * (D + 8) + D * (NP + 8) + 16 * (NP + 8);
}
static long ai_bwd_w(int K, int D, int l) {
  const int din = l == 0 ? K : D;
  return 4L * D * (ai_kv(K, D, l) + 8) + (long)ai_up(din, 16) * (4 * D + 8);
}
static long ai_bwd_wave(int nf, int K, int D, int hd) {
  const long NP = ai_up(nf, 16);
  return NP * ai_sx(K, D) + 4 * NP * (D + 8) + 3L * hd * (NP + 8) +
         16 * (NP + 8) + 2 * NP * (NP + 8);
}
static int ai_waves(long w, long per) {
  const long n = (kAiLdsMax / 2 - w) / per;
  return (int)(n > kAiMaxWaves ? kAiMaxWaves : n);
}

// dynamic LDS of the largest kernel with one wave a block: the least the
// shape needs
long autoint_lds_bytes(int nf, int K, int heads, int hd, int L) {
  const int D = heads * hd;
  long need = 2 * (ai_fwd_w(K, D, L) + ai_fwd_wave(nf, K, D));
  for (int l = 0; l < L; ++l) {
    const long b = 2 * (ai_bwd_w(K, D, l) + ai_bwd_wave(nf, K, D, hd));
    if (b > need) need = b;
  }
  const long wg = 2L * (ai_up(K > D ? K : D, 16) + 4 * D) * kAiWgStride;
  return wg > need ? wg : need;
}

int autoint_wgrad_chunk_rows(long T) {
  long per = (T + kAiWgChunks - 1) / kAiWgChunks;
  per = (per + kAiWgRows - 1) / kAiWgRows * kAiWgRows;
  return (int)(per > 0 ? per : kAiWgRows);
}
int autoint_wgrad_chunks(long T) {
  const long c = autoint_wgrad_chunk_rows(T);
  return (int)((T + c - 1) / c);
}
int autoint_du_chunks(int B) { return (B + kAiDuRows - 1) / kAiDuRows; }

__device__ __forceinline__ float ai_shfl_xor(float v, int s) {
  const int lane =
      __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute((lane ^ s) << 2,
                                          __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ void ai_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// orders the wave's own LDS traffic: what its lanes wrote before is what
// they read after (a wave's LDS operations complete in order)
__device__ __forceinline__ void ai_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float ai_bf2f(ai_bf v) {
  return __builtin_bit_cast(float, (unsigned)v << 16);
}

// round to nearest even; a NaN stays a NaN
__device__ __forceinline__ ai_bf ai_f2bf(float f) {
  const unsigned v = __builtin_bit_cast(unsigned, f);
  if ((v & 0x7fffffffu) > 0x7f800000u) return (ai_bf)((v >> 16) | 0x40u);
  return (ai_bf)((v + 0x7fffu + ((v >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ bool ai_pos(ai_bf v) {  // v > 0
  return (v & 0x8000u) == 0 && (v & 0x7fffu) != 0 && (v & 0x7fffu) <= 0x7f80u;
}

// acc[i] += sum_{k < kv} A[lq*4+i][k] B[lrow][k]: A and B are 16 rows of bf16
// in LDS with strides lda, ldb (multiples of 8, bases 16-byte aligned), kv a
// multiple of 8
__device__ __forceinline__ ai_f32x4 ai_mma(ai_f32x4 acc, const ai_bf* A,
                                           int lda, const ai_bf* B, int ldb,
                                           int kv, int lrow, int lq) {
  for (int k = lq * 8; k - lq * 8 < kv; k += 32) {
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (k < kv) {
      a = *(const uint4*)(A + lrow * lda + k);
      b = *(const uint4*)(B + lrow * ldb + k);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        __builtin_bit_cast(ai_bf16x8, a), __builtin_bit_cast(ai_bf16x8, b),
        acc, 0, 0, 0);
  }
  return acc;
}

// W^l [din, N4] (global, row-major) transposed into dst [N4][kv + 8], the
// columns din .. kv - 1 as zeros
__device__ __forceinline__ void ai_stage_wt(ai_bf* dst,
                                            const ai_bf* __restrict__ W,
                                            int din, int kv, int N4) {
  const int sw = kv + 8;
  for (int idx = threadIdx.x; idx < N4 * kv; idx += blockDim.x) {
    const int k = idx / N4, n = idx - k * N4;
    dst[n * sw + k] = k < din ? W[(size_t)k * N4 + n] : (ai_bf)0;
  }
}

// the wave's X buffer [NP][sx]: zeros, then the nf rows of din values at src
__device__ __forceinline__ void ai_load_rows(ai_bf* xs,
                                             const ai_bf* __restrict__ src,
                                             int NP, int sx, int nf, int din,
                                             int lane) {
  for (int idx = lane; idx < NP * sx / 8; idx += 64)
    ((uint4*)xs)[idx] = make_uint4(0u, 0u, 0u, 0u);
  ai_wsync();
  for (int idx = lane; idx < nf * din; idx += 64) {
    const int tok = idx / din;
    xs[tok * sx + idx - tok * din] = src[idx];
  }
}

// Q, K, V of every token from xs and the staged W^T: Q and K as token rows
// [NP][sd]; V as token rows too (vt_stride = 0) or transposed [D][vt_stride]
template <int MT>
__device__ __forceinline__ void ai_project(const ai_bf* xs, int sx,
                                           const ai_bf* Wt, int sw, int kv,
                                           ai_bf* qs, ai_bf* ks, ai_bf* vs,
                                           int sd, int vt_stride, int D,
                                           int lrow, int lq) {
  const int DT = D >> 4;
  for (int nt = 0; nt < 3 * DT; ++nt) {
    const int blk = nt / DT, c = (nt - blk * DT) * 16 + lrow;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const ai_f32x4 acc =
          ai_mma(ai_f32x4{0.f, 0.f, 0.f, 0.f}, xs + mt * 16 * sx, sx,
                 Wt + nt * 16 * sw, sw, kv, lrow, lq);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int tok = mt * 16 + lq * 4 + i;
        const ai_bf v = ai_f2bf(acc[i]);
        if (blk == 0) qs[tok * sd + c] = v;
        else if (blk == 1) ks[tok * sd + c] = v;
        else if (vt_stride) vs[c * vt_stride + tok] = v;
        else vs[tok * sd + c] = v;
      }
    }
  }
}

// p[kt][i] = softmax over keys of S[q = lq*4+i][key = kt*16+lrow], for the 16
// queries at q (rows of head columns, stride sd) against the keys at k
template <int MT>
__device__ __forceinline__ void ai_probs(float (&p)[MT][4], const ai_bf* q,
                                         const ai_bf* k, int sd, int hd,
                                         int nf, int lrow, int lq) {
#pragma unroll
  for (int kt = 0; kt < MT; ++kt) {
    const ai_f32x4 acc = ai_mma(ai_f32x4{0.f, 0.f, 0.f, 0.f}, q, sd,
                                k + kt * 16 * sd, sd, hd, lrow, lq);
    const bool live = kt * 16 + lrow < nf;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      p[kt][i] = live ? acc[i] : -__builtin_inff();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float m = p[0][i];
#pragma unroll
    for (int kt = 1; kt < MT; ++kt) m = fmaxf(m, p[kt][i]);
#pragma unroll
    for (int sh = 1; sh < 16; sh <<= 1) m = fmaxf(m, ai_shfl_xor(m, sh));
    float s = 0.f;
#pragma unroll
    for (int kt = 0; kt < MT; ++kt) {
      p[kt][i] = __expf(p[kt][i] - m);
      s += p[kt][i];
    }
#pragma unroll
    for (int sh = 1; sh < 16; sh <<= 1) s += ai_shfl_xor(s, sh);
    const float inv = 1.f / s;
#pragma unroll
    for (int kt = 0; kt < MT; ++kt) p[kt][i] *= inv;
  }
}

template <int MT, bool SAVE>
__global__ __launch_bounds__(256) void autoint_forward_kernel(
    const ai_bf* __restrict__ x0, const ai_bf* __restrict__ Wbf,
    const float* __restrict__ u, float* __restrict__ ai,
    ai_bf* __restrict__ X, int nf, int K, int heads, int hd, int L, int B) {
  constexpr int NP = 16 * MT;
  const int D = heads * hd, DT = D >> 4, hdf = hd >> 4, N4 = 4 * D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int sx = (((K + 7) & ~7) > D ? ((K + 7) & ~7) : D) + 8;
  const int sd = D + 8, sp = NP + 8;
  ai_bf* wl = (ai_bf*)ai_lds;
  int wtot = 0;
  {
    size_t goff = 0;
    for (int l = 0; l < L; ++l) {
      const int din = l ? D : K, kv = l ? D : (K + 7) & ~7;
      ai_stage_wt(wl + wtot, Wbf + goff, din, kv, N4);
      goff += (size_t)din * N4;
      wtot += N4 * (kv + 8);
    }
  }
  ai_sync();
  ai_bf* xs = wl + wtot + wave * (NP * sx + 2 * NP * sd + D * sp + 16 * sp);
  ai_bf* qs = xs + NP * sx;   // [NP][sd]
  ai_bf* ks = qs + NP * sd;   // [NP][sd]
  ai_bf* vt = ks + NP * sd;   // [D][sp]
  ai_bf* ps = vt + D * sp;    // [16][sp]
  const int ntiles = (B + kAiTile - 1) / kAiTile;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int eend = tile * kAiTile + kAiTile < B ? tile * kAiTile + kAiTile
                                                  : B;
    for (int e = tile * kAiTile + wave; e < eend; e += nw) {
      ai_load_rows(xs, x0 + (size_t)e * nf * K, NP, sx, nf, K, lane);
      ai_wsync();
      float aisum = 0.f;
      int woff = 0;
      for (int l = 0; l < L; ++l) {
        const int kv = l ? D : (K + 7) & ~7, sw = kv + 8;
        const ai_bf* Wt = wl + woff;
        ai_project<MT>(xs, sx, Wt, sw, kv, qs, ks, vt, sd, sp, D, lrow, lq);
        ai_wsync();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          ai_f32x4 o[4];
#pragma unroll
          for (int f = 0; f < 4; ++f) {
            o[f] = ai_f32x4{0.f, 0.f, 0.f, 0.f};
            if (f < DT)
              o[f] = ai_mma(o[f], xs + mt * 16 * sx, sx,
                            Wt + (3 * D + f * 16) * sw, sw, kv, lrow, lq);
          }
          for (int h = 0; h < heads; ++h) {
            float p[MT][4];
            ai_probs<MT>(p, qs + mt * 16 * sd + h * hd, ks + h * hd, sd, hd,
                         nf, lrow, lq);
#pragma unroll
            for (int kt = 0; kt < MT; ++kt)
#pragma unroll
              for (int i = 0; i < 4; ++i)
                ps[(lq * 4 + i) * sp + kt * 16 + lrow] = ai_f2bf(p[kt][i]);
            ai_wsync();
#pragma unroll
            for (int f = 0; f < 4; ++f)
              if (f < DT && f / hdf == h)
                o[f] = ai_mma(o[f], ps, sp, vt + f * 16 * sp, sp, NP, lrow,
                              lq);
            ai_wsync();
          }
          // X^l replaces the rows of X^{l-1} that only this fragment read
#pragma unroll
          for (int f = 0; f < 4; ++f)
            if (f < DT) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int tok = mt * 16 + lq * 4 + i, c = f * 16 + lrow;
                float v = 0.f;
                if (tok < nf) {
                  v = fmaxf(o[f][i], 0.f);
                  if (l == L - 1) aisum = fmaf(v, u[tok * D + c], aisum);
                }
                xs[tok * sx + c] = ai_f2bf(v);
              }
            }
        }
        ai_wsync();
        if (SAVE) {
          ai_bf* out = X + ((size_t)l * B + e) * nf * D;
          for (int idx = lane; idx < nf * (D / 8); idx += 64) {
            const int tok = idx / (D / 8), g = idx - tok * (D / 8);
            *(uint4*)(out + (size_t)tok * D + g * 8) =
                *(const uint4*)(xs + tok * sx + g * 8);
          }
        }
        woff += N4 * sw;
      }
#pragma unroll
      for (int sh = 1; sh < 64; sh <<= 1) aisum += ai_shfl_xor(aisum, sh);
      if (lane == 0) ai[e] = aisum;
      ai_wsync();
    }
  }
}

// One layer of the backward (l = 0 .. L-1 is the layer's index, W its
// [din, 4D] block of the mirror). Xp: X^{l-1} [B, nf, din]; Xl: X^l, read
// when top; G: [B nf, 4D] of this layer, its dY block read unless top;
// Gp: the layer below's, whose dY block is written unless first.
template <int MT>
__global__ __launch_bounds__(256) void autoint_backward_kernel(
    const ai_bf* __restrict__ Xp, const ai_bf* __restrict__ Xl,
    const ai_bf* __restrict__ W, const float* __restrict__ u,
    const float* __restrict__ dpred, float* __restrict__ dDeep,
    ai_bf* __restrict__ G, ai_bf* __restrict__ Gp, int nf, int K, int din,
    int heads, int hd, int B, int top, int first) {
  constexpr int NP = 16 * MT;
  const int D = heads * hd, hdf = hd >> 4, N4 = 4 * D;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nw = blockDim.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int sx = (((K + 7) & ~7) > D ? ((K + 7) & ~7) : D) + 8;
  const int sd = D + 8, sp = NP + 8;
  const int kv = (din + 7) & ~7, sw = kv + 8;
  const int dinp = (din + 15) & ~15, JT = dinp >> 4, sr = N4 + 8;
  ai_bf* Wt = (ai_bf*)ai_lds;   // [4D][sw]   W^T
  ai_bf* Wr = Wt + N4 * sw;     // [dinp][sr] W, rows past din as zeros
  ai_stage_wt(Wt, W, din, kv, N4);
  for (int idx = threadIdx.x; idx < dinp * N4; idx += blockDim.x) {
    const int k = idx / N4, n = idx - k * N4;
    Wr[k * sr + n] = k < din ? W[(size_t)k * N4 + n] : (ai_bf)0;
  }
  ai_sync();
  ai_bf* xs = Wr + dinp * sr +
              wave * (NP * sx + 4 * NP * sd + 3 * hd * sp + 16 * sp +
                      2 * NP * sp);
  ai_bf* qs = xs + NP * sx;    // [NP][sd] Q, then dQ
  ai_bf* ks = qs + NP * sd;    //          K, then dK
  ai_bf* vs = ks + NP * sd;    //          V, then dV
  ai_bf* ys = vs + NP * sd;    //          dY
  ai_bf* qt = ys + NP * sd;    // [hd][sp] the head's Q^T
  ai_bf* kt_ = qt + hd * sp;   //          K^T
  ai_bf* yt = kt_ + hd * sp;   //          dY^T
  ai_bf* dsq = yt + hd * sp;   // [16][sp] dS of 16 queries
  ai_bf* dst = dsq + 16 * sp;  // [NP][sp] dS^T
  ai_bf* pt = dst + NP * sp;   // [NP][sp] A^T
  const int ntiles = (B + kAiTile - 1) / kAiTile;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int eend = tile * kAiTile + kAiTile < B ? tile * kAiTile + kAiTile
                                                  : B;
    for (int e = tile * kAiTile + wave; e < eend; e += nw) {
      ai_load_rows(xs, Xp + (size_t)e * nf * din, NP, sx, nf, din, lane);
      const float dp = dpred[e];
      for (int idx = lane; idx < NP * D; idx += 64) {
        const int tok = idx / D, c = idx - tok * D;
        ai_bf v = 0;
        if (tok < nf) {
          if (top) {
            if (ai_pos(Xl[((size_t)e * nf + tok) * D + c]))
              v = ai_f2bf(dp * u[tok * D + c]);
          } else {
            v = G[((size_t)e * nf + tok) * N4 + 3 * D + c];
          }
        }
        ys[tok * sd + c] = v;
      }
      ai_wsync();
      ai_project<MT>(xs, sx, Wt, sw, kv, qs, ks, vs, sd, 0, D, lrow, lq);
      ai_wsync();
      for (int h = 0; h < heads; ++h) {
        for (int idx = lane; idx < NP * hd; idx += 64) {
          const int tok = idx / hd, c = idx - tok * hd;
          qt[c * sp + tok] = qs[tok * sd + h * hd + c];
          kt_[c * sp + tok] = ks[tok * sd + h * hd + c];
          yt[c * sp + tok] = ys[tok * sd + h * hd + c];
        }
        ai_wsync();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          float p[MT][4], da[MT][4];
          ai_probs<MT>(p, qs + mt * 16 * sd + h * hd, ks + h * hd, sd, hd, nf,
                       lrow, lq);
#pragma unroll
          for (int kt = 0; kt < MT; ++kt) {
            const ai_f32x4 acc = ai_mma(
                ai_f32x4{0.f, 0.f, 0.f, 0.f}, ys + mt * 16 * sd + h * hd, sd,
                vs + kt * 16 * sd + h * hd, sd, hd, lrow, lq);
#pragma unroll
            for (int i = 0; i < 4; ++i) da[kt][i] = acc[i];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float r = 0.f;
#pragma unroll
            for (int kt = 0; kt < MT; ++kt) r = fmaf(p[kt][i], da[kt][i], r);
#pragma unroll
            for (int sh = 1; sh < 16; sh <<= 1) r += ai_shfl_xor(r, sh);
#pragma unroll
            for (int kt = 0; kt < MT; ++kt) {
              const ai_bf ds = ai_f2bf(p[kt][i] * (da[kt][i] - r));
              const int q = lq * 4 + i, key = kt * 16 + lrow;
              dsq[q * sp + key] = ds;
              dst[key * sp + mt * 16 + q] = ds;
              pt[key * sp + mt * 16 + q] = ai_f2bf(p[kt][i]);
            }
          }
          ai_wsync();
          // dQ = dS K over the head's columns, in place of Q
#pragma unroll
          for (int f = 0; f < 2; ++f)
            if (f < hdf) {
              const ai_f32x4 acc =
                  ai_mma(ai_f32x4{0.f, 0.f, 0.f, 0.f}, dsq, sp,
                         kt_ + f * 16 * sp, sp, NP, lrow, lq);
#pragma unroll
              for (int i = 0; i < 4; ++i)
                qs[(mt * 16 + lq * 4 + i) * sd + h * hd + f * 16 + lrow] =
                    ai_f2bf(acc[i]);
            }
          ai_wsync();
        }
        // dK = dS^T Q and dV = A^T dY, in place of the head's K and V
#pragma unroll
        for (int kt = 0; kt < MT; ++kt)
#pragma unroll
          for (int f = 0; f < 2; ++f)
            if (f < hdf) {
              const ai_f32x4 z = {0.f, 0.f, 0.f, 0.f};
              const ai_f32x4 dk = ai_mma(z, dst + kt * 16 * sp, sp,
                                         qt + f * 16 * sp, sp, NP, lrow, lq);
              const ai_f32x4 dv = ai_mma(z, pt + kt * 16 * sp, sp,
                                         yt + f * 16 * sp, sp, NP, lrow, lq);
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int o = (kt * 16 + lq * 4 + i) * sd + h * hd + f * 16 +
                              lrow;
                ks[o] = ai_f2bf(dk[i]);
                vs[o] = ai_f2bf(dv[i]);
              }
            }
        ai_wsync();
      }
      // [dQ | dK | dV | dY] of the nf tokens, the weight gradient's operand
      for (int idx = lane; idx < nf * (N4 / 8); idx += 64) {
        const int tok = idx / (N4 / 8), g = idx - tok * (N4 / 8);
        const int blk = g / (D / 8), gg = g - blk * (D / 8);
        *(uint4*)(G + ((size_t)e * nf + tok) * N4 + g * 8) =
            *(const uint4*)(qs + blk * NP * sd + tok * sd + gg * 8);
      }
      // dX^{l-1} = [dQ | dK | dV | dY] W^T
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        for (int jt = 0; jt < JT; ++jt) {
          ai_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int blk = 0; blk < 4; ++blk)
            acc = ai_mma(acc, qs + blk * NP * sd + mt * 16 * sd, sd,
                         Wr + jt * 16 * sr + blk * D, sr, D, lrow, lq);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int tok = mt * 16 + lq * 4 + i, j = jt * 16 + lrow;
            if (tok < nf && j < din) {
              if (first)
                dDeep[((size_t)e * nf + tok) * din + j] += acc[i];
              else
                Gp[((size_t)e * nf + tok) * N4 + 3 * D + j] =
                    ai_pos(xs[tok * sx + j]) ? ai_f2bf(acc[i]) : (ai_bf)0;
            }
          }
        }
      ai_wsync();
    }
  }
}

// part[chunk, j] = sum over the chunk's examples of dpred[b] X^L[b, j]
__global__ __launch_bounds__(256) void autoint_du_kernel(
    const ai_bf* __restrict__ XL, const float* __restrict__ dpred,
    float* __restrict__ part, int n, int B) {
  const int b0 = blockIdx.x * kAiDuRows;
  const int b1 = b0 + kAiDuRows < B ? b0 + kAiDuRows : B;
  for (int j = threadIdx.x; j < n; j += blockDim.x) {
    float s = 0.f;
    for (int b = b0; b < b1; ++b)
      s = fmaf(dpred[b], ai_bf2f(XL[(size_t)b * n + j]), s);
    part[(size_t)blockIdx.x * n + j] = s;
  }
}

// out[j] = sum_k part[k n + j], k = 0 .. nparts - 1 in that order
__global__ __launch_bounds__(256) void autoint_sum_parts_kernel(
    const float* __restrict__ part, float* __restrict__ out, long n,
    int nparts) {
  const long j = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(size_t)k * n + j];
  out[j] = s;
}

// part[chunk, k, n] = sum over the chunk's tokens t of Xp[t, k] G[t, n];
// 4 waves, wave w the columns [w D, (w + 1) D)
__global__ __launch_bounds__(256) void autoint_wgrad_kernel(
    const ai_bf* __restrict__ Xp, const ai_bf* __restrict__ G,
    float* __restrict__ part, int din, int D, long T, int chunk_rows) {
  constexpr int WS = kAiWgStride;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int N4 = 4 * D, DT = D >> 4, dinp = (din + 15) & ~15, JT = dinp >> 4;
  ai_bf* xT = (ai_bf*)ai_lds;  // [dinp][WS]
  ai_bf* gT = xT + dinp * WS;  // [4D][WS]
  const long rbeg = (long)blockIdx.x * chunk_rows;
  const long rend = rbeg + chunk_rows < T ? rbeg + chunk_rows : T;
  for (int idx = threadIdx.x; idx < dinp * WS; idx += blockDim.x)
    xT[idx] = 0;  // the rows past din stay zero
  ai_f32x4 acc[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[j][f] = ai_f32x4{0.f, 0.f, 0.f, 0.f};
  for (long r0 = rbeg; r0 < rend; r0 += kAiWgRows) {
    ai_sync();  // the last step's reads are done
    for (int idx = threadIdx.x; idx < kAiWgRows * din; idx += blockDim.x) {
      const int row = idx / din, k = idx - row * din;
      const long t = r0 + row;
      xT[k * WS + row] = t < rend ? Xp[(size_t)t * din + k] : (ai_bf)0;
    }
    for (int idx = threadIdx.x; idx < kAiWgRows * N4; idx += blockDim.x) {
      const int row = idx / N4, n = idx - row * N4;
      const long t = r0 + row;
      gT[n * WS + row] = t < rend ? G[(size_t)t * N4 + n] : (ai_bf)0;
    }
    ai_sync();
    ai_bf16x8 b[4];
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (f < DT)
        b[f] = __builtin_bit_cast(
            ai_bf16x8,
            *(const uint4*)(gT + ((wave * DT + f) * 16 + lrow) * WS + lq * 8));
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < JT) {
        const ai_bf16x8 a = __builtin_bit_cast(
            ai_bf16x8, *(const uint4*)(xT + (j * 16 + lrow) * WS + lq * 8));
#pragma unroll
        for (int f = 0; f < 4; ++f)
          if (f < DT)
            acc[j][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                a, b[f], acc[j][f], 0, 0, 0);
      }
  }
  float* out = part + (size_t)blockIdx.x * din * N4;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int f = 0; f < 4; ++f)
      if (j < JT && f < DT) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k = j * 16 + lq * 4 + i;
          if (k < din)
            out[(size_t)k * N4 + (wave * DT + f) * 16 + lrow] = acc[j][f][i];
        }
      }
}

#define DISPATCH_AI_MT(NF, ...)                                       \
  switch (((NF) + 15) / 16) {                                         \
    case 1: { constexpr int MTC = 1; __VA_ARGS__; break; }            \
    case 2: { constexpr int MTC = 2; __VA_ARGS__; break; }            \
    case 3: { constexpr int MTC = 3; __VA_ARGS__; break; }            \
    case 4: { constexpr int MTC = 4; __VA_ARGS__; break; }            \
    default:                                                          \
      fprintf(stderr, "lightctr_amd: unsupported autoint nf %d\n",    \
              NF);                                                    \
      abort();                                                        \
  }

// requests above 64 KB of dynamic LDS have to be announced per kernel
#define AI_ANNOUNCE_LDS(KERNEL, BYTES)                                \
  if ((BYTES) > 64 * 1024)                                            \
  LCTR_CHECK_HIP(hipFuncSetAttribute(                                 \
      (const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, \
      (int)(BYTES)))

static unsigned ai_grid(int B) {
  const int t = (B + kAiTile - 1) / kAiTile;
  return (unsigned)(t < kAiMaxBlocks ? t : kAiMaxBlocks);
}

// X [L, B, nf, D] is written when save is set and may be null otherwise
void autoint_forward_launch(const void* x0, const void* Wbf, const float* u,
                            float* ai, void* X, bool save, int nf, int K,
                            int heads, int hd, int L, int B,
                            hipStream_t stream) {
  if (B <= 0) return;
  const int D = heads * hd;
  const long w = ai_fwd_w(K, D, L), per = ai_fwd_wave(nf, K, D);
  const int nw = ai_waves(w, per);
  const size_t lds = (size_t)(2 * (w + nw * per));
#define AI_FWD(SAVE)                                                       \
  DISPATCH_AI_MT(                                                          \
      nf, AI_ANNOUNCE_LDS((autoint_forward_kernel<MTC, SAVE>), lds);       \
      hipLaunchKernelGGL((autoint_forward_kernel<MTC, SAVE>),              \
                         dim3(ai_grid(B)), dim3(nw * LCTR_WAVE), lds,      \
                         stream, (const ai_bf*)x0, (const ai_bf*)Wbf, u,   \
                         ai, (ai_bf*)X, nf, K, heads, hd, L, B))
  if (save) {
    AI_FWD(true);
  } else {
    AI_FWD(false);
  }
#undef AI_FWD
}

// G: [L, B nf, 4D] bf16 of workspace; part: floats for the larger of
// [autoint_wgrad_chunks(B nf), max d_in, 4D] and [autoint_du_chunks(B), nf D].
// dW (flat, the layout of W) and du are written for every B, as zeros for
// an empty batch.
void autoint_backward_launch(const void* x0, const void* X, const void* Wbf,
                             const float* u, const float* dpred,
                             float* dDeep, void* G, float* part, float* dW,
                             float* du, int nf, int K, int heads, int hd,
                             int L, int B, hipStream_t stream) {
  const int D = heads * hd, N4 = 4 * D;
  const long T = (long)B * nf;
  const ai_bf* Xb = (const ai_bf*)X;
  ai_bf* Gb = (ai_bf*)G;
  const size_t xl = (size_t)T * D, gl = (size_t)T * N4;
  const long nu = (long)nf * D;
  const int nparts = B > 0 ? autoint_du_chunks(B) : 0;
  if (B > 0)
    hipLaunchKernelGGL(autoint_du_kernel, dim3(nparts), dim3(256), 0, stream,
                       Xb + (L - 1) * xl, dpred, part, (int)nu, B);
  hipLaunchKernelGGL(autoint_sum_parts_kernel,
                     dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, stream,
                     part, du, nu, nparts);
  size_t woff = 0;
  for (int l = 0; l < L; ++l) woff += (size_t)(l ? D : K) * N4;
  for (int l = L - 1; l >= 0; --l) {
    const int din = l ? D : K;
    woff -= (size_t)din * N4;
    if (B <= 0) continue;
    const long w = ai_bwd_w(K, D, l), per = ai_bwd_wave(nf, K, D, hd);
    const int nw = ai_waves(w, per);
    const size_t lds = (size_t)(2 * (w + nw * per));
    const ai_bf* Xp = l ? Xb + (l - 1) * xl : (const ai_bf*)x0;
    DISPATCH_AI_MT(
        nf, AI_ANNOUNCE_LDS((autoint_backward_kernel<MTC>), lds);
        hipLaunchKernelGGL((autoint_backward_kernel<MTC>), dim3(ai_grid(B)),
                           dim3(nw * LCTR_WAVE), lds, stream, Xp,
                           Xb + l * xl, (const ai_bf*)Wbf + woff, u, dpred,
                           dDeep, Gb + l * gl, l ? Gb + (l - 1) * gl : Gb,
                           nf, K, din, heads, hd, B, (int)(l == L - 1),
                           (int)(l == 0)));
  }
  const int nchunks = B > 0 ? autoint_wgrad_chunks(T) : 0;
  const int chunk_rows = autoint_wgrad_chunk_rows(T);
  for (int l = 0; l < L; ++l) {
    const int din = l ? D : K;
    const long n = (long)din * N4;
    if (nchunks > 0) {
      const size_t lds =
          (size_t)(2L * (ai_up(din, 16) + N4) * kAiWgStride);
      hipLaunchKernelGGL(autoint_wgrad_kernel, dim3(nchunks),
                         dim3(4 * LCTR_WAVE), lds, stream,
                         l ? Xb + (l - 1) * xl : (const ai_bf*)x0,
                         Gb + l * gl, part, din, D, T, chunk_rows);
    }
    hipLaunchKernelGGL(autoint_sum_parts_kernel,
                       dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       stream, part, dW, n, nchunks);
    dW += n;
  }
}

}  // namespace lightctr

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
