// PNN's inner-product layer (Qu et al., ICDM 2016; DLRM's dot interaction) for
// MI355X/gfx950. The concat row x0 (bf16 [B, nf*K]) that Wide&Deep's MLP reads
// is viewed as e[b, i, :], i < nf, and the MLP's input becomes
//
//   z[b]       = [ x0[b] , g[b] , 0 .. 0 ]              bf16 [B, Dz]
//   g[b, p(i,j)] = e_i . e_j,   i < j,  p(i,j) = i (2 nf - i - 1) / 2 + j - i - 1
//   P = nf (nf - 1) / 2,   Dz = nf K + P rounded up to a multiple of 8
//
// (the row-major strict upper triangle of the Gram E E^T). Backward, from the
// MLP's input gradient dz (fp32 [B, Dz]), Gs the symmetric matrix of the pair
// gradients with a zero diagonal:
//
//   dDeep[b, i K + k] = dz[b, i K + k] + sum_j Gs[b, i, j] e[b, j, k]
//
// Work split, both kernels: a wave owns whole examples and never synchronises
// with the other waves of its block; a block of 4 waves takes 4 consecutive
// examples a sweep and strides over the batch.
//
// Forward. The Gram is cut into 16 x 16 field tiles, ti <= tj only (6 of 9 at
// 39 fields). The A fragment of tile ti and the B fragment of tile tj have the
// same per-lane pattern, field 16 t + lane % 16 and a run of consecutive k
// (4 (lane / 16) .. +4 for v_mfma_f32_16x16x16_bf16 at K <= 16, 8 (lane / 16)
// .. +8 for v_mfma_f32_16x16x32_bf16 at K = 32 and twice that at K = 64), so a
// lane loads one fragment a tile straight from global memory, 8 or 16 bytes,
// zeros for a field >= nf or a k >= K, and every tile pair is one (K = 64:
// two) MFMA on two of these. The C fragment gives the lane g[i = 16 ti +
// 4 (lane / 16) + c][j = 16 tj + lane % 16], c < 4. The packed triangle is
// put together in the wave's row buffer in LDS (Dz bf16): the x0 words as read
// (8 bytes a lane), the strict upper triangle at p(i, j), rounded to bf16 once
// (nearest even), +0 in the pad; the row then goes out in 16-byte vectors.
// Every element of z is written.
//
// Backward. The transposed product dDeep^T = E^T Gs (Gs is symmetric) runs on
// v_mfma_f32_16x16x32_bf16 with the contraction over the fields, padded with
// zeros to 32 or 64: the C fragment then holds 4 consecutive k of one field,
// which is a 16-byte vector of dz and of dDeep. Both operands want a run of
// 8 consecutive j a lane, so the wave keeps in LDS Gs [16 NT][SG] (the pair
// gradients unpacked, each rounded to bf16 once, written at (i, j) and (j, i))
// and E^T [max(K, 16)][SG] (from the first nf K columns of z, row stride Dz),
// SG = 32 JS + 8 so that rows stay 16-byte aligned and 16 rows spread over the
// banks. The diagonal, the rows and columns >= nf and the k >= K are zeroed
// once a launch and never written again. The pair gradients are read as
// float4; (i, j) of the first comes from the inverse of p (a square root and
// an integer fix-up), the other three by stepping.
//
// No atomics, one writer an element: bit-identical from run to run.
#include "common.h"

namespace lightctr {

typedef __attribute__((ext_vector_type(4))) short pnn_bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 pnn_bf16x8;
typedef __attribute__((ext_vector_type(4))) float pnn_f32x4;
typedef unsigned short pnn_bf;  // a bf16 as its bits

static constexpr int kPnnWaves = 4;  // one example a wave and sweep
static constexpr int kPnnMaxBlocks = 4096;

extern __shared__ __align__(16) unsigned char pnn_lds[];

int pnn_tile_rows() { return kPnnWaves; }

int pnn_out_dim(int nf, int K) {
  return (nf * K + nf * (nf - 1) / 2 + 7) & ~7;
}

// orders the wave's own LDS traffic: what its lanes wrote before is what
// they read after (a wave's LDS operations complete in order)
__device__ __forceinline__ void pnn_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// round to nearest even; a NaN stays a NaN
__device__ __forceinline__ pnn_bf pnn_f2bf(float f) {
  const unsigned v = __builtin_bit_cast(unsigned, f);
  if ((v & 0x7fffffffu) > 0x7f800000u) return (pnn_bf)((v >> 16) | 0x40u);
  return (pnn_bf)((v + 0x7fffu + ((v >> 16) & 1u)) >> 16);
}

// first pair index of row i
__device__ __forceinline__ int pnn_row_start(int i, int nf) {
  return i * (2 * nf - i - 1) / 2;
}

// the row i of pair p: the largest i with pnn_row_start(i) <= p, p < P
__device__ __forceinline__ int pnn_row_of(int p, int nf) {
  const int m = 2 * nf - 1;
  int i = (int)(((float)m - sqrtf((float)(m * m - 8 * p))) * 0.5f);
  i = i < 0 ? 0 : (i > nf - 2 ? nf - 2 : i);
  while (i < nf - 2 && pnn_row_start(i + 1, nf) <= p) ++i;
  while (pnn_row_start(i, nf) > p) --i;
  return i;
}

// The lane's operand words of one field tile: field f = 16 t + lane % 16, the
// k run of the instruction that K takes, zeros outside the row.
template <int K>
struct PnnFrag {
  static constexpr int KS = K <= 32 ? 1 : K / 32;  // MFMAs a tile pair
  uint4 v[KS];  // K <= 16: the low 8 bytes only
};

template <int K>
__device__ __forceinline__ PnnFrag<K> pnn_load_frag(
    const pnn_bf* __restrict__ xr, int f, int nf, int lq) {
  PnnFrag<K> r;
#pragma unroll
  for (int s = 0; s < PnnFrag<K>::KS; ++s) r.v[s] = make_uint4(0u, 0u, 0u, 0u);
  if (f < nf) {
    if constexpr (K <= 16) {
      if (4 * lq < K) {
        const uint2 w = *(const uint2*)(xr + f * K + 4 * lq);
        r.v[0].x = w.x, r.v[0].y = w.y;
      }
    } else {
#pragma unroll
      for (int s = 0; s < PnnFrag<K>::KS; ++s)
        r.v[s] = *(const uint4*)(xr + f * K + 32 * s + 8 * lq);
    }
  }
  return r;
}

template <int K>
__device__ __forceinline__ pnn_f32x4 pnn_gram_tile(const PnnFrag<K>& a,
                                                   const PnnFrag<K>& b) {
  pnn_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if constexpr (K <= 16) {
    acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
        __builtin_bit_cast(pnn_bf16x4, make_uint2(a.v[0].x, a.v[0].y)),
        __builtin_bit_cast(pnn_bf16x4, make_uint2(b.v[0].x, b.v[0].y)), acc, 0,
        0, 0);
  } else {
#pragma unroll
    for (int s = 0; s < PnnFrag<K>::KS; ++s)
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(pnn_bf16x8, a.v[s]),
          __builtin_bit_cast(pnn_bf16x8, b.v[s]), acc, 0, 0, 0);
  }
  return acc;
}

template <int K, int NT>
__global__ __launch_bounds__(256) void pnn_forward_kernel(
    const pnn_bf* __restrict__ x0, pnn_bf* __restrict__ z, int nf, int Dz,
    int B) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int d = nf * K, P = nf * (nf - 1) / 2;
  pnn_bf* row = (pnn_bf*)pnn_lds + wave * Dz;
  for (int e = blockIdx.x * kPnnWaves + wave; e < B;
       e += gridDim.x * kPnnWaves) {
    const pnn_bf* xr = x0 + (size_t)e * d;
    PnnFrag<K> fr[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
      fr[t] = pnn_load_frag<K>(xr, 16 * t + lrow, nf, lq);
    pnn_wsync();  // the last example's row has been read
    for (int w = lane; w < d / 4; w += 64)
      ((uint2*)row)[w] = ((const uint2*)xr)[w];
    if (d + P + lane < Dz) row[d + P + lane] = 0;  // at most 7 pad columns
#pragma unroll
    for (int ti = 0; ti < NT; ++ti)
#pragma unroll
      for (int tj = ti; tj < NT; ++tj) {
        const pnn_f32x4 acc = pnn_gram_tile<K>(fr[ti], fr[tj]);
        const int j = 16 * tj + lrow;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int i = 16 * ti + 4 * lq + c;
          if (i < j && j < nf)
            row[d + pnn_row_start(i, nf) + j - i - 1] = pnn_f2bf(acc[c]);
        }
      }
    pnn_wsync();
    uint4* zr = (uint4*)(z + (size_t)e * Dz);
    for (int w = lane; w < Dz / 8; w += 64) zr[w] = ((const uint4*)row)[w];
  }
}

// dynamic LDS of the backward per block: at most 45 KB (nf = 64, K = 16)
static inline size_t pnn_bwd_lds(int nf, int K) {
  const int rows = ((nf + 15) & ~15) + (K < 16 ? 16 : K);
  return (size_t)kPnnWaves * rows * (32 * ((nf + 31) / 32) + 8) *
         sizeof(pnn_bf);
}

template <int K>
__global__ __launch_bounds__(256) void pnn_backward_kernel(
    const pnn_bf* __restrict__ z, const float* __restrict__ dz,
    float* __restrict__ dDeep, int nf, int Dz, int B) {
  constexpr int KP = K < 16 ? 16 : K, KT = KP / 16;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  const int d = nf * K, P = nf * (nf - 1) / 2;
  const int NT = (nf + 15) >> 4, JS = (nf + 31) >> 5, SG = 32 * JS + 8;
  const int rows = 16 * NT + KP;
  pnn_bf* gs = (pnn_bf*)pnn_lds + wave * rows * SG;  // [16 NT][SG]
  pnn_bf* et = gs + 16 * NT * SG;                    // [KP][SG]
  for (int w = lane; w < rows * SG / 8; w += 64)
    ((uint4*)gs)[w] = make_uint4(0u, 0u, 0u, 0u);
  for (int e = blockIdx.x * kPnnWaves + wave; e < B;
       e += gridDim.x * kPnnWaves) {
    const pnn_bf* zr = z + (size_t)e * Dz;
    const float* dr = dz + (size_t)e * Dz;
    pnn_wsync();  // the zeros are in place, the last example's reads are done
    for (int w = lane; w < d / 4; w += 64) {  // E^T: 4 k of one field a word
      const uint2 v = ((const uint2*)zr)[w];
      const int j = 4 * w / K, k = 4 * w - j * K;
      pnn_bf* o = et + k * SG + j;
      o[0] = (pnn_bf)v.x, o[SG] = (pnn_bf)(v.x >> 16);
      o[2 * SG] = (pnn_bf)v.y, o[3 * SG] = (pnn_bf)(v.y >> 16);
    }
    for (int p = 4 * lane; p < P; p += 256) {  // Gs from 4 pair gradients
      const float4 v = *(const float4*)(dr + d + p);
      const float g[4] = {v.x, v.y, v.z, v.w};
      int i = pnn_row_of(p, nf), j = i + 1 + p - pnn_row_start(i, nf);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (p + c < P) {
          const pnn_bf b = pnn_f2bf(g[c]);
          gs[i * SG + j] = b, gs[j * SG + i] = b;
          if (++j == nf) ++i, j = i + 1;
        }
      }
    }
    pnn_wsync();
    float* out = dDeep + (size_t)e * d;
    for (int ti = 0; ti < NT; ++ti) {
      const int i = 16 * ti + lrow;
      // B operand: Gs[j = 32 s + 8 lq .. +8][i], read along row i (symmetric)
      const pnn_bf* gp = gs + i * SG + 8 * lq;
      const uint4 b0 = *(const uint4*)gp;
      uint4 b1 = make_uint4(0u, 0u, 0u, 0u);
      if (JS > 1) b1 = *(const uint4*)(gp + 32);
#pragma unroll
      for (int tk = 0; tk < KT; ++tk) {
        // A operand: E^T[k = 16 tk + lrow][j = 32 s + 8 lq .. +8]
        const pnn_bf* ep = et + (16 * tk + lrow) * SG + 8 * lq;
        pnn_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            __builtin_bit_cast(pnn_bf16x8, *(const uint4*)ep),
            __builtin_bit_cast(pnn_bf16x8, b0), acc, 0, 0, 0);
        if (JS > 1)
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(pnn_bf16x8, *(const uint4*)(ep + 32)),
              __builtin_bit_cast(pnn_bf16x8, b1), acc, 0, 0, 0);
        // the lane holds dDeep[i][k .. k + 3]
        const int k = 16 * tk + 4 * lq;
        if (i < nf && k < K) {
          float4 r = *(const float4*)(dr + i * K + k);
          r.x += acc[0], r.y += acc[1], r.z += acc[2], r.w += acc[3];
          *(float4*)(out + i * K + k) = r;
        }
      }
    }
  }
}

static inline unsigned pnn_grid(int B) {
  const int t = (B + kPnnWaves - 1) / kPnnWaves;
  return (unsigned)(t < kPnnMaxBlocks ? t : kPnnMaxBlocks);
}

#define PNN_FWD_CASE(KV, NTV)                                              \
  case (KV) * 8 + (NTV):                                                   \
    hipLaunchKernelGGL((pnn_forward_kernel<KV, NTV>), dim3(pnn_grid(B)),   \
                       dim3(kPnnWaves * LCTR_WAVE), lds, stream,           \
                       (const pnn_bf*)x0, (pnn_bf*)z, nf, Dz, B);          \
    break;

// z: bf16 [B, pnn_out_dim(nf, K)], every element written
void pnn_forward_launch(const void* x0, void* z, int nf, int K, int B,
                        hipStream_t stream) {
  if (B <= 0) return;
  const int Dz = pnn_out_dim(nf, K);
  const size_t lds = (size_t)kPnnWaves * Dz * sizeof(pnn_bf);
  switch (K * 8 + (nf + 15) / 16) {  // nf K <= 1024 leaves these 15
    PNN_FWD_CASE(4, 1) PNN_FWD_CASE(4, 2) PNN_FWD_CASE(4, 3) PNN_FWD_CASE(4, 4)
    PNN_FWD_CASE(8, 1) PNN_FWD_CASE(8, 2) PNN_FWD_CASE(8, 3) PNN_FWD_CASE(8, 4)
    PNN_FWD_CASE(16, 1) PNN_FWD_CASE(16, 2) PNN_FWD_CASE(16, 3)
    PNN_FWD_CASE(16, 4) PNN_FWD_CASE(32, 1) PNN_FWD_CASE(32, 2)
    PNN_FWD_CASE(64, 1)
    default:
      fprintf(stderr, "lightctr_amd: unsupported pnn nf %d, K %d\n", nf, K);
      abort();
  }
}

// z: the forward's output (its first nf K columns are read); dz: fp32
// [B, Dz]; dDeep: fp32 [B, nf K], every element written
void pnn_backward_launch(const void* z, const float* dz, float* dDeep, int nf,
                         int K, int B, hipStream_t stream) {
  if (B <= 0) return;
  const int Dz = pnn_out_dim(nf, K);
  const size_t lds = pnn_bwd_lds(nf, K);
  DISPATCH_K(K, hipLaunchKernelGGL((pnn_backward_kernel<KC>),
                                   dim3(pnn_grid(B)),
                                   dim3(kPnnWaves * LCTR_WAVE), lds, stream,
                                   (const pnn_bf*)z, dz, dDeep, nf, Dz, B));
}

}  // namespace lightctr
