// Attentional FM (Xiao et al., IJCAI 2017) for MI355X/gfx950: attention over
// the pairwise products of the field vectors of the concat row x0 (bf16
// [B, nf*K]) that the MLP reads, viewed as e[b, i, :], i < nf. A = the
// attention width, Wa [K, A], ba [A], qa [A], ua [K]:
//
//   p_ij   = e_i * e_j                 i < j, P = nf (nf - 1) / 2 pairs
//   z_ij   = Wa^T p_ij + ba
//   s_ij   = qa . relu(z_ij)
//   a      = softmax over the P pairs of s
//   afm[b] = ua . sum_ij a_ij p_ij
//
// Work split. A wave owns whole examples and never synchronises with the
// other waves of its block until the parameter gradients are written; a block
// of 4 waves takes tiles of 16 consecutive examples. The example's row sits in
// the wave's LDS as fp32, K padded with zeros to KP = 16 KS, rows 4 floats
// apart from a multiple of 16 so that the 16 rows a tile reads hit 64 distinct
// banks. Wa (both operand orientations), ba, qa and ua live in registers for
// the whole launch.
//
// A tile is one i and up to 16 consecutive j > i: lane l holds pair
// j = j0 + l % 16 and the k-slice 4 (l / 16) .. +4 of each of the KS k-steps.
// The lane forms its slice of p from two LDS reads, keeps it in fp32 and
// rounds one copy to bf16: that copy is the B operand of
// v_mfma_f32_16x16x16_bf16 (4 k-values a lane), the A operand being Wa^T, so
// the C fragment gives the lane 4 attention units a row fragment of its own
// pair. + ba, ReLU, * qa, a sum in the lane and two cross-lane steps over the
// four lane groups leave s of the pair in every lane that holds a slice of its
// product: no transpose, no LDS round trip. Tail lanes are masked (s = -inf,
// product 0). nf = 39 takes 66 tiles for 741 pairs, 70 % of the lanes live.
//
// The softmax streams: each lane keeps a running max, a running sum and the
// f partial of its pair column and k-slice; the 16 columns are merged once an
// example (4 xor steps and a rescale), which also gives lse = max + log(sum).
//
// Backward, one launch: z, s and a = exp(s - lse) are recomputed per tile.
// t = ua . p (two cross-lane steps), ds = dpred a (t - afm),
// dz^T = ds qa [z > 0] comes out in the C layout, which is the B layout of
// dP^T = Wa dz^T (Wa as the A operand), whose C layout is again the lane's own
// product slice; the lane adds dpred a ua and feeds de_i (registers over the
// tiles of a row, reduced over the 16 columns once a row) and de_j (every
// (j, k) of a tile belongs to one lane: a plain LDS read-add-write in a fixed
// order). dDeep += dx0 is written along the row once an example. dWa^T =
// sum dz^T P reduces over the pairs, so both operands go transposed through a
// 16-row LDS tile of the wave. Its accumulators and the lane partials of dba,
// dqa and dua persist over all examples of the wave, are added in wave order
// through LDS once a block, written to part[blocks, K A + 2 A + K] and added
// in block order by afm_sum_parts_kernel. No float atomics: every output is
// bit-identical from run to run.
//
// Rounding points (everything else is fp32): x0 and Wa as given (bf16); the
// pair product once, as an MFMA operand only (f, t, dua and the de terms read
// the fp32 product); dz as an operand. The ReLU mask reads the fp32 z.
#include "common.h"

// No packed fp32 instructions in this file (as cin_kernels.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                     \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

namespace lightctr {

typedef __attribute__((ext_vector_type(4))) short afm_bf16x4;
typedef __attribute__((ext_vector_type(4))) float afm_f32x4;
typedef unsigned short afm_bf;  // a bf16 as its bits

static constexpr int kAfmTile = 16;        // examples per block tile
static constexpr int kAfmWaves = 4;
static constexpr int kAfmFwdBlocks = 1024;
static constexpr int kAfmBwdBlocks = 512;  // one partial a block

extern __shared__ __align__(16) unsigned char afm_lds[];

int afm_tile_rows() { return kAfmTile; }

static inline int afm_kp(int K) { return (K + 15) & ~15; }
static inline long afm_fwd_wave(int nf, int K) {
  return 4L * nf * (afm_kp(K) + 4);
}
static inline long afm_bwd_wave(int nf, int K, int A) {
  return 2 * afm_fwd_wave(nf, K) + 32L * (A + 4 + afm_kp(K) + 4);
}
static inline long afm_part_floats(int K, int A) {
  return (long)K * A + 2 * A + K;
}

// dynamic LDS per block of the backward, the larger of the two kernels
long afm_lds_bytes(int nf, int K, int A) {
  const long w = kAfmWaves * afm_bwd_wave(nf, K, A);
  const long r = 4 * afm_part_floats(K, A);
  return w > r ? w : r;
}

int afm_backward_chunks(int B) {
  const int t = (B + kAfmTile - 1) / kAfmTile;
  return t < kAfmBwdBlocks ? t : kAfmBwdBlocks;
}

// orders the wave's own LDS traffic: what its lanes wrote before is what
// they read after (a wave's LDS operations complete in order)
__device__ __forceinline__ void afm_wsync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ void afm_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ float afm_bf2f(afm_bf v) {
  return __builtin_bit_cast(float, (unsigned)v << 16);
}

// round to nearest even; a NaN stays a NaN
__device__ __forceinline__ afm_bf afm_f2bf(float f) {
  const unsigned v = __builtin_bit_cast(unsigned, f);
  if ((v & 0x7fffffffu) > 0x7f800000u) return (afm_bf)((v >> 16) | 0x40u);
  return (afm_bf)((v + 0x7fffu + ((v >> 16) & 1u)) >> 16);
}

__device__ __forceinline__ afm_bf16x4 afm_pack(const float (&v)[4]) {
  return afm_bf16x4{(short)afm_f2bf(v[0]), (short)afm_f2bf(v[1]),
                    (short)afm_f2bf(v[2]), (short)afm_f2bf(v[3])};
}

// sum over the four lane groups (the lanes of one pair column)
__device__ __forceinline__ float afm_sum_groups(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// sum over the 16 pair columns of a lane group
__device__ __forceinline__ float afm_sum_cols(float v) {
#pragma unroll
  for (int s = 1; s < 16; s <<= 1) v += __shfl_xor(v, s);
  return v;
}

// Wa^T as the A operand of the score product: lane (lrow, lq) holds
// Wa[k = 16 ks + 4 lq + i][a = 16 af + lrow]; W[k sk + a sa] (either mirror)
template <int KS, int AF>
__device__ __forceinline__ void afm_load_wat(afm_bf16x4 (&wat)[AF][KS],
                                             const afm_bf* __restrict__ W,
                                             int sk, int sa, int K, int lrow,
                                             int lq) {
#pragma unroll
  for (int af = 0; af < AF; ++af)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      short v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k = 16 * ks + 4 * lq + i;
        v[i] = k < K ? (short)W[(size_t)k * sk + (size_t)(16 * af + lrow) * sa]
                     : (short)0;
      }
      wat[af][ks] = afm_bf16x4{v[0], v[1], v[2], v[3]};
    }
}

// the lane's 4 values of a vector of 16 N entries: v[n][i] = src[16 n + 4 lq
// + i], zeros past len
template <int N>
__device__ __forceinline__ void afm_load_vec(float (&v)[N][4],
                                             const float* __restrict__ src,
                                             int len, int lq) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * n + 4 * lq + i;
      v[n][i] = c < len ? src[c] : 0.f;
    }
}

// the example's row as fp32 into xs [nf][KP + 4], k >= K as zeros
template <int KS>
__device__ __forceinline__ void afm_load_row(float* xs,
                                             const afm_bf* __restrict__ src,
                                             int nf, int K, int lane) {
  constexpr int KP = 16 * KS, XS = KP + 4;
  for (int idx = lane; idx < nf * KP; idx += 64) {
    const int i = idx / KP, k = idx - i * KP;
    xs[i * XS + k] = k < K ? afm_bf2f(src[i * K + k]) : 0.f;
  }
}

template <int KS>
__device__ __forceinline__ void afm_read_slice(float (&v)[KS][4],
                                               const float* row, int lq) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const float4 r = *(const float4*)(row + 16 * ks + 4 * lq);
    v[ks][0] = r.x, v[ks][1] = r.y, v[ks][2] = r.z, v[ks][3] = r.w;
  }
}

// the lane's slice of p = e_i * e_j (zeros in a masked lane), its bf16 copy,
// h = z + ba of the lane's 4 AF attention units and s of the pair. The
// backward recomputes through this function, so its s is the forward's.
template <int KS, int AF>
__device__ __forceinline__ float afm_score(
    const afm_bf16x4 (&wat)[AF][KS], const float (&ba)[AF][4],
    const float (&qa)[AF][4], const float (&ei)[KS][4],
    const float (&ej)[KS][4], bool live, float (&p)[KS][4],
    afm_bf16x4 (&pb)[KS], float (&h)[AF][4]) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
    for (int i = 0; i < 4; ++i) p[ks][i] = live ? ei[ks][i] * ej[ks][i] : 0.f;
    pb[ks] = afm_pack(p[ks]);
  }
  float s = 0.f;
#pragma unroll
  for (int af = 0; af < AF; ++af) {
    afm_f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      z = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wat[af][ks], pb[ks], z, 0,
                                                    0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      h[af][i] = z[i] + ba[af][i];
      s = fmaf(qa[af][i], fmaxf(h[af][i], 0.f), s);
    }
  }
  return afm_sum_groups(s);
}

template <int KS, int AF>
__global__ __launch_bounds__(256) void afm_forward_kernel(
    const afm_bf* __restrict__ x0, const afm_bf* __restrict__ Wbf,
    const float* __restrict__ bav, const float* __restrict__ qav,
    const float* __restrict__ uav, float* __restrict__ afm,
    float* __restrict__ lse, int nf, int K, int B, int save) {
  constexpr int XS = 16 * KS + 4, A = 16 * AF;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  float* xs = (float*)afm_lds + wave * nf * XS;
  afm_bf16x4 wat[AF][KS];
  float ba[AF][4], qa[AF][4], ua[KS][4];
  afm_load_wat<KS, AF>(wat, Wbf, A, 1, K, lrow, lq);
  afm_load_vec<AF>(ba, bav, A, lq);
  afm_load_vec<AF>(qa, qav, A, lq);
  afm_load_vec<KS>(ua, uav, K, lq);
  const int ntiles = (B + kAfmTile - 1) / kAfmTile;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int eend = tile * kAfmTile + kAfmTile < B ? tile * kAfmTile + kAfmTile
                                                    : B;
    for (int e = tile * kAfmTile + wave; e < eend; e += kAfmWaves) {
      afm_wsync();  // the last example's reads are done
      afm_load_row<KS>(xs, x0 + (size_t)e * nf * K, nf, K, lane);
      afm_wsync();
      float m = -__builtin_inff(), l = 0.f, f[KS][4];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int i = 0; i < 4; ++i) f[ks][i] = 0.f;
      for (int i = 0; i + 1 < nf; ++i) {
        float ei[KS][4];
        afm_read_slice<KS>(ei, xs + i * XS, lq);
        for (int j0 = i + 1; j0 < nf; j0 += 16) {
          const bool live = j0 + lrow < nf;
          float ej[KS][4], p[KS][4], h[AF][4];
          afm_bf16x4 pb[KS];
          afm_read_slice<KS>(ej, xs + (live ? j0 + lrow : i) * XS, lq);
          float s = afm_score<KS, AF>(wat, ba, qa, ei, ej, live, p, pb, h);
          s = live ? s : -__builtin_inff();
          const float mn = fmaxf(m, s);
          const float sc = m == mn ? 1.f : __expf(m - mn);
          const float w = live ? __expf(s - mn) : 0.f;
          l = fmaf(l, sc, w);
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int c = 0; c < 4; ++c)
              f[ks][c] = fmaf(f[ks][c], sc, w * p[ks][c]);
          m = mn;
        }
      }
      // the 16 pair columns into one: column 0 is never empty
      float M = m;
#pragma unroll
      for (int s = 1; s < 16; s <<= 1) M = fmaxf(M, __shfl_xor(M, s));
      const float sc = m == -__builtin_inff() ? 0.f : __expf(m - M);
      l = afm_sum_cols(l * sc);
      float t = 0.f;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int c = 0; c < 4; ++c) t = fmaf(ua[ks][c], f[ks][c] * sc, t);
      t = afm_sum_groups(afm_sum_cols(t));
      if (lane == 0) {
        afm[e] = t / l;
        if (save) lse[e] = M + __logf(l);
      }
    }
  }
}

template <int KS, int AF>
__global__ __launch_bounds__(256) void afm_backward_kernel(
    const afm_bf* __restrict__ x0, const float* __restrict__ lse,
    const float* __restrict__ afm, const afm_bf* __restrict__ Wbf,
    const afm_bf* __restrict__ Wtbf, const float* __restrict__ bav,
    const float* __restrict__ qav, const float* __restrict__ uav,
    const float* __restrict__ dpred, float* __restrict__ dDeep,
    float* __restrict__ part, int nf, int K, int B) {
  constexpr int KP = 16 * KS, XS = KP + 4, A = 16 * AF;
  constexpr int SA = A + 4, SK = KP + 4;  // strides of the transposing tiles
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lrow = lane & 15, lq = lane >> 4;
  float* xs = (float*)(afm_lds + (size_t)wave * (8 * nf * XS + 32 * (SA + SK)));
  float* de = xs + nf * XS;               // [nf][XS] dx0 of the example
  afm_bf* tz = (afm_bf*)(de + nf * XS);   // [16 pairs][SA] dz
  afm_bf* tp = tz + 16 * SA;              // [16 pairs][SK] p
  afm_bf16x4 wat[AF][KS], wa[KS][AF];
  float ba[AF][4], qa[AF][4], ua[KS][4];
  afm_load_wat<KS, AF>(wat, Wtbf, 1, K, K, lrow, lq);
  // Wa as the A operand of dP^T = Wa dz^T: Wa[k = 16 ks + lrow][a = 16 af +
  // 4 lq + i], the rows past K as zeros
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int af = 0; af < AF; ++af) {
      const int k = 16 * ks + lrow;
      short v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
        v[i] = k < K ? (short)Wbf[(size_t)k * A + 16 * af + 4 * lq + i]
                     : (short)0;
      wa[ks][af] = afm_bf16x4{v[0], v[1], v[2], v[3]};
    }
  afm_load_vec<AF>(ba, bav, A, lq);
  afm_load_vec<AF>(qa, qav, A, lq);
  afm_load_vec<KS>(ua, uav, K, lq);
  afm_f32x4 dW[AF][KS];  // dWa^T[a = 16 af + 4 lq + i][k = 16 ks + lrow]
  float dba[AF][4], dqa[AF][4], dua[KS][4];
#pragma unroll
  for (int af = 0; af < AF; ++af) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) dW[af][ks] = afm_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) dba[af][i] = dqa[af][i] = 0.f;
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int i = 0; i < 4; ++i) dua[ks][i] = 0.f;
  const int ntiles = (B + kAfmTile - 1) / kAfmTile;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int eend = tile * kAfmTile + kAfmTile < B ? tile * kAfmTile + kAfmTile
                                                    : B;
    for (int e = tile * kAfmTile + wave; e < eend; e += kAfmWaves) {
      afm_wsync();  // the last example's reads are done
      afm_load_row<KS>(xs, x0 + (size_t)e * nf * K, nf, K, lane);
      for (int idx = lane; idx < nf * XS; idx += 64) de[idx] = 0.f;
      afm_wsync();
      const float lse_e = lse[e], afm_e = afm[e], dp_e = dpred[e];
      for (int i = 0; i + 1 < nf; ++i) {
        float ei[KS][4], dei[KS][4];
        afm_read_slice<KS>(ei, xs + i * XS, lq);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int c = 0; c < 4; ++c) dei[ks][c] = 0.f;
        for (int j0 = i + 1; j0 < nf; j0 += 16) {
          const bool live = j0 + lrow < nf;
          const int j = live ? j0 + lrow : i;
          float ej[KS][4], p[KS][4], h[AF][4];
          afm_bf16x4 pb[KS], dzb[AF];
          afm_read_slice<KS>(ej, xs + j * XS, lq);
          const float s = afm_score<KS, AF>(wat, ba, qa, ei, ej, live, p, pb,
                                            h);
          const float a = live ? __expf(s - lse_e) : 0.f;
          float t = 0.f;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
#pragma unroll
            for (int c = 0; c < 4; ++c) t = fmaf(ua[ks][c], p[ks][c], t);
          t = afm_sum_groups(t);
          const float g = dp_e * a, ds = g * (t - afm_e);
#pragma unroll
          for (int af = 0; af < AF; ++af) {
            float dz[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              dz[c] = h[af][c] > 0.f ? ds * qa[af][c] : 0.f;
              dba[af][c] += dz[c];
              dqa[af][c] = fmaf(ds, fmaxf(h[af][c], 0.f), dqa[af][c]);
            }
            dzb[af] = afm_pack(dz);
          }
          // dP^T = Wa dz^T + dpred a ua, then de_i (registers) and de_j (LDS)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            afm_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int af = 0; af < AF; ++af)
              acc = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
                  wa[ks][af], dzb[af], acc, 0, 0, 0);
            float dpv[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              dua[ks][c] = fmaf(g, p[ks][c], dua[ks][c]);
              dpv[c] = fmaf(g, ua[ks][c], acc[c]);
              dei[ks][c] = fmaf(dpv[c], live ? ej[ks][c] : 0.f, dei[ks][c]);
            }
            if (live) {  // (j, this k-slice) is this lane's alone in the tile
              float4* d = (float4*)(de + j * XS + 16 * ks + 4 * lq);
              float4 r = *d;
              r.x = fmaf(dpv[0], ei[ks][0], r.x);
              r.y = fmaf(dpv[1], ei[ks][1], r.y);
              r.z = fmaf(dpv[2], ei[ks][2], r.z);
              r.w = fmaf(dpv[3], ei[ks][3], r.w);
              *d = r;
            }
          }
          // dWa^T += dz^T P: both operands transposed through the wave's tile
          afm_wsync();  // the last tile's reads are done
#pragma unroll
          for (int af = 0; af < AF; ++af)
            *(afm_bf16x4*)(tz + lrow * SA + 16 * af + 4 * lq) = dzb[af];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            *(afm_bf16x4*)(tp + lrow * SK + 16 * ks + 4 * lq) = pb[ks];
          afm_wsync();
          afm_bf16x4 bp[KS];
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            bp[ks] = afm_bf16x4{(short)tp[(4 * lq + 0) * SK + 16 * ks + lrow],
                                (short)tp[(4 * lq + 1) * SK + 16 * ks + lrow],
                                (short)tp[(4 * lq + 2) * SK + 16 * ks + lrow],
                                (short)tp[(4 * lq + 3) * SK + 16 * ks + lrow]};
#pragma unroll
          for (int af = 0; af < AF; ++af) {
            const afm_bf16x4 az = {
                (short)tz[(4 * lq + 0) * SA + 16 * af + lrow],
                (short)tz[(4 * lq + 1) * SA + 16 * af + lrow],
                (short)tz[(4 * lq + 2) * SA + 16 * af + lrow],
                (short)tz[(4 * lq + 3) * SA + 16 * af + lrow]};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks)
              dW[af][ks] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(
                  az, bp[ks], dW[af][ks], 0, 0, 0);
          }
        }
        // de_i of the row: the 16 columns summed, added after the de_j that
        // earlier rows left in it
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
#pragma unroll
          for (int c = 0; c < 4; ++c) dei[ks][c] = afm_sum_cols(dei[ks][c]);
        afm_wsync();
        if (lrow == 0) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) {
            float4* d = (float4*)(de + i * XS + 16 * ks + 4 * lq);
            float4 r = *d;
            r.x += dei[ks][0], r.y += dei[ks][1];
            r.z += dei[ks][2], r.w += dei[ks][3];
            *d = r;
          }
        }
        afm_wsync();
      }
      float* out = dDeep + (size_t)e * nf * K;
      for (int idx = lane; idx < nf * K; idx += 64) {
        const int i = idx / K;
        out[idx] += de[i * XS + idx - i * K];
      }
    }
  }
  // the wave's partials: lanes of a column group summed, then the four waves
  // in wave order through LDS, then one row of part a block
#pragma unroll
  for (int af = 0; af < AF; ++af)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      dba[af][c] = afm_sum_cols(dba[af][c]);
      dqa[af][c] = afm_sum_cols(dqa[af][c]);
    }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int c = 0; c < 4; ++c) dua[ks][c] = afm_sum_cols(dua[ks][c]);
  float* red = (float*)afm_lds;
  const int n = K * A + 2 * A + K;
  for (int w = 0; w < kAfmWaves; ++w) {
    afm_sync();  // w = 0: every wave is done with its own buffers
    if (wave != w) continue;
#pragma unroll
    for (int af = 0; af < AF; ++af)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int a = 16 * af + 4 * lq + c;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const int k = 16 * ks + lrow;
          if (k < K)
            red[k * A + a] = (w ? red[k * A + a] : 0.f) + dW[af][ks][c];
        }
        if (lrow == 0) {
          red[K * A + a] = (w ? red[K * A + a] : 0.f) + dba[af][c];
          red[K * A + A + a] = (w ? red[K * A + A + a] : 0.f) + dqa[af][c];
        }
      }
    if (lrow == 0) {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int k = 16 * ks + 4 * lq + c, o = K * A + 2 * A + k;
          if (k < K) red[o] = (w ? red[o] : 0.f) + dua[ks][c];
        }
    }
  }
  afm_sync();
  for (int idx = threadIdx.x; idx < n; idx += blockDim.x)
    part[(size_t)blockIdx.x * n + idx] = red[idx];
}

// out[j] = sum_k part[k n + j], k = 0 .. nparts - 1 in that order
__global__ __launch_bounds__(256) void afm_sum_parts_kernel(
    const float* __restrict__ part, float* __restrict__ out, int n,
    int nparts) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(size_t)k * n + j];
  out[j] = s;
}

#define AFM_CASE(KSV, AFV, ...)                                       \
  case (KSV) * 8 + (AFV): {                                           \
    constexpr int KSC = KSV, AFC = AFV;                               \
    __VA_ARGS__;                                                      \
    break;                                                            \
  }
#define AFM_ROW(KSV, ...)                                             \
  AFM_CASE(KSV, 1, __VA_ARGS__)                                       \
  AFM_CASE(KSV, 2, __VA_ARGS__)                                       \
  AFM_CASE(KSV, 3, __VA_ARGS__)                                       \
  AFM_CASE(KSV, 4, __VA_ARGS__)
#define DISPATCH_AFM(K, A, ...)                                       \
  switch ((((K) + 15) / 16) * 8 + (A) / 16) {                         \
    AFM_ROW(1, __VA_ARGS__)                                           \
    AFM_ROW(2, __VA_ARGS__)                                           \
    AFM_ROW(3, __VA_ARGS__)                                           \
    AFM_ROW(4, __VA_ARGS__)                                           \
    default:                                                          \
      fprintf(stderr, "lightctr_amd: unsupported afm K %d, A %d\n",   \
              K, A);                                                  \
      abort();                                                        \
  }

// requests above 64 KB of dynamic LDS have to be announced per kernel
#define AFM_ANNOUNCE_LDS(KERNEL, BYTES)                               \
  if ((BYTES) > 64 * 1024)                                            \
  LCTR_CHECK_HIP(hipFuncSetAttribute(                                 \
      (const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, \
      (int)(BYTES)))

// lse [B] is written when save is set and may be null otherwise
void afm_forward_launch(const void* x0, const void* Wbf, const float* ba,
                        const float* qa, const float* ua, float* afm,
                        float* lse, bool save, int nf, int K, int A, int B,
                        hipStream_t stream) {
  if (B <= 0) return;
  const int t = (B + kAfmTile - 1) / kAfmTile;
  const unsigned grid = (unsigned)(t < kAfmFwdBlocks ? t : kAfmFwdBlocks);
  const size_t lds = (size_t)(kAfmWaves * afm_fwd_wave(nf, K));
  DISPATCH_AFM(
      K, A, AFM_ANNOUNCE_LDS((afm_forward_kernel<KSC, AFC>), lds);
      hipLaunchKernelGGL((afm_forward_kernel<KSC, AFC>), dim3(grid),
                         dim3(kAfmWaves * LCTR_WAVE), lds, stream,
                         (const afm_bf*)x0, (const afm_bf*)Wbf, ba, qa, ua,
                         afm, lse, nf, K, B, (int)save));
}

// part: afm_backward_chunks(B) * (K A + 2 A + K) floats; out: K A + 2 A + K
// floats, [dWa [K, A] | dba | dqa | dua], written for every B, as zeros for an
// empty batch
void afm_backward_launch(const void* x0, const float* lse, const float* afm,
                         const void* Wbf, const void* Wtbf, const float* ba,
                         const float* qa, const float* ua, const float* dpred,
                         float* dDeep, float* part, float* out, int nf, int K,
                         int A, int B, hipStream_t stream) {
  const int nparts = B > 0 ? afm_backward_chunks(B) : 0;
  const int n = (int)afm_part_floats(K, A);
  if (nparts > 0) {
    const size_t lds = (size_t)afm_lds_bytes(nf, K, A);
    DISPATCH_AFM(
        K, A, AFM_ANNOUNCE_LDS((afm_backward_kernel<KSC, AFC>), lds);
        hipLaunchKernelGGL((afm_backward_kernel<KSC, AFC>), dim3(nparts),
                           dim3(kAfmWaves * LCTR_WAVE), lds, stream,
                           (const afm_bf*)x0, lse, afm, (const afm_bf*)Wbf,
                           (const afm_bf*)Wtbf, ba, qa, ua, dpred, dDeep,
                           part, nf, K, B));
  }
  hipLaunchKernelGGL(afm_sum_parts_kernel, dim3((unsigned)((n + 255) / 256)),
                     dim3(256), 0, stream, part, out, n, nparts);
}

}  // namespace lightctr

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
