// Batched nearest-neighbour search for MI355X/gfx950 (predict/knn.py):
// exact (flat) and product-quantised (ADC) top-k.
//
// Result contract: row q of (ids, dist) holds the k smallest pairs in
// ascending lexicographic (dist, id) order, float comparison by `<` (so -0
// and +0 tie), ties to the lower id; slots past the number of rows are
// id -1, dist +inf. Smaller is better in both metrics: squared L2, or
// 0 - <q, x>.
//
// One selection serves every kernel. A (dist, id) pair is packed into one
// 64-bit key whose unsigned order is the contract's order (float bits made
// monotone in the high word, id in the low word), so the top-k of a set of
// rows is the k smallest keys and is unique. A block keeps its sorted best
// k keys and a candidate buffer in LDS. Rows are visited in batches; a row
// whose key is below the block's current k-th key is appended to the buffer
// (an LDS counter hands out the slots; the slot order is arbitrary, but the
// buffer is only ever sorted, and keys are unique, so it cannot reach the
// result). When the next batch might not fit, the buffer is merged into the
// list by a bitonic sort of list + buffer and the threshold tightens. Rows
// are fed by a source policy: ADC (codes + the query's LUT in LDS), flat
// (X streamed or gathered through a candidate list, the query in LDS) and
// the per-slice partial lists of the merge pass.
//
// Work split: block = (query, slice of the row axis). knn_slice_rows is
// the slicing rule; with more than one slice every block stores its k keys
// to partial[nq, n_slices, k] and knn_merge_kernel (one block per query)
// selects over them with the same code. No float atomics, no atomics on
// global memory: two runs are bit-equal.
#include "common.h"

#include <cstdint>

namespace lightctr {

#define KNN_BLOCK 256
#define KNN_MAX_K 256
#define KNN_SORT 2048        // LDS key slots: list [0, k) + buffer
#define KNN_MIN_SLICE 1024   // rows; a multiple of every source's batch
#define KNN_ROUND 1024
#define KNN_TARGET_BLOCKS 1024
#define KNN_MAX_SUB 64
#define KNN_MAX_DIM 1024

typedef unsigned long long knn_key_t;
#define KNN_PAD (~0ull)  // above every real key; decodes to (-1, +inf)

__device__ __forceinline__ knn_key_t knn_make_key(float d, int id) {
  d = (d == 0.f) ? 0.f : d;  // -0 ties with +0
  unsigned u = __float_as_uint(d);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((knn_key_t)u << 32) | (unsigned)id;
}

__device__ __forceinline__ float knn_key_dist(knn_key_t key) {
  unsigned u = (unsigned)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  return __uint_as_float(u);
}

// ascending bitonic sort of a[0, P) in LDS, P a power of two <= KNN_SORT
__device__ void knn_bitonic_sort(knn_key_t* a, int P) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (P >> 1); t += KNN_BLOCK) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;
        const knn_key_t x = a[lo], y = a[hi];
        if ((x > y) == up) {
          a[lo] = y;
          a[hi] = x;
        }
      }
    }
  }
  __syncthreads();
}

// Merges the buffer [k, k + cnt) into the list [0, k). Block-uniform call;
// every thread has read cnt and no push is in flight. With DEDUP, equal
// keys (the same row listed twice) keep one copy.
template <bool DEDUP>
__device__ void knn_compact(knn_key_t* s_keys, int* s_cnt, int k, int cnt) {
  const int n = min(k + cnt, KNN_SORT);
  int P = 2;
  while (P < n) P <<= 1;
  for (int i = n + threadIdx.x; i < P; i += KNN_BLOCK) s_keys[i] = KNN_PAD;
  if (threadIdx.x == 0) *s_cnt = 0;
  knn_bitonic_sort(s_keys, P);
  if (DEDUP) {
    // equal keys are adjacent now: blank all but the first, sort again
    bool dup[KNN_SORT / KNN_BLOCK];
    bool any = false;
#pragma unroll
    for (int j = 0; j < KNN_SORT / KNN_BLOCK; ++j) {
      const int i = threadIdx.x + j * KNN_BLOCK;
      dup[j] = i > 0 && i < P && s_keys[i] != KNN_PAD &&
               s_keys[i] == s_keys[i - 1];
      any |= dup[j];
    }
    if (__syncthreads_or(any)) {
#pragma unroll
      for (int j = 0; j < KNN_SORT / KNN_BLOCK; ++j)
        if (dup[j]) s_keys[threadIdx.x + j * KNN_BLOCK] = KNN_PAD;
      knn_bitonic_sort(s_keys, P);
    }
  }
}

// Leaves the k smallest keys of items [begin, end) sorted in s_keys[0, k).
// Src::LPI lanes cooperate on one item and Src::R items are in flight per
// lane group; src.key returns KNN_PAD for an item to skip.
template <class Src, bool DEDUP>
__device__ void knn_select(const Src& src, long begin, long end, int k,
                           knn_key_t* s_keys, int* s_cnt) {
  constexpr int GROUPS = KNN_BLOCK / Src::LPI;
  constexpr int BATCH = GROUPS * Src::R;
  static_assert(BATCH <= KNN_SORT - KNN_MAX_K, "a batch must fit the buffer");
  static_assert(KNN_MIN_SLICE % BATCH == 0, "slices hold whole batches");
  const int g = threadIdx.x / Src::LPI;
  const bool leader = threadIdx.x % Src::LPI == 0;
  const int room = KNN_SORT - k;
  for (int i = threadIdx.x; i < k; i += KNN_BLOCK) s_keys[i] = KNN_PAD;
  if (threadIdx.x == 0) *s_cnt = 0;
  knn_key_t thr = KNN_PAD;
  for (long base = begin; base < end; base += BATCH) {
    __syncthreads();  // the previous batch's pushes (and the setup) landed
    const int cnt = *s_cnt;
    __syncthreads();  // everyone holds cnt before anyone pushes again
    if (cnt + BATCH > room) {
      knn_compact<DEDUP>(s_keys, s_cnt, k, cnt);
      thr = s_keys[k - 1];
    }
    knn_key_t key[Src::R];
#pragma unroll
    for (int r = 0; r < Src::R; ++r)
      key[r] = src.key(base + (long)r * GROUPS + g, end);
#pragma unroll
    for (int r = 0; r < Src::R; ++r) {
      if (leader && key[r] < thr) {
        const int slot = atomicAdd(s_cnt, 1);
        if (slot < room) s_keys[k + slot] = key[r];
      }
    }
  }
  __syncthreads();
  const int cnt = *s_cnt;
  __syncthreads();
  knn_compact<DEDUP>(s_keys, s_cnt, k, cnt);
}

// the block's result: keys to its partial slot, or decoded to the outputs
__device__ void knn_write(const knn_key_t* s_keys, int k, knn_key_t* partial,
                          int* ids, float* dist) {
  for (int i = threadIdx.x; i < k; i += KNN_BLOCK) {
    const knn_key_t key = s_keys[i];
    if (partial) {
      partial[i] = key;
    } else if (key == KNN_PAD) {
      ids[i] = -1;
      dist[i] = __uint_as_float(0x7f800000u);
    } else {
      ids[i] = (int)(unsigned)(key & 0xffffffffu);
      dist[i] = knn_key_dist(key);
    }
  }
}

// ---- sources ----

// ADC: dist = lut[0][code[0]] + lut[1][code[1]] + ... added in fp32 in
// ascending sub-vector order from 0.0f. VEC = bytes per code load.
template <int VEC>
struct KnnAdcSrc {
  static constexpr int LPI = 1;
  static constexpr int R = 4;
  const unsigned char* codes;
  long stride;
  int n_sub, ncb;
  const float* lut;  // LDS, [n_sub, ncb]

  __device__ __forceinline__ knn_key_t key(long item, long end) const {
    if (item >= end) return KNN_PAD;
    const unsigned char* row = codes + item * stride;
    float acc = 0.f;
    if constexpr (VEC == 1) {
      for (int s = 0; s < n_sub; ++s) acc += lut[s * ncb + row[s]];
    } else {
      for (int s0 = 0; s0 < n_sub; s0 += VEC) {
        unsigned w[VEC / 4];
        if constexpr (VEC == 16) {
          const uint4 v = *reinterpret_cast<const uint4*>(row + s0);
          w[0] = v.x;
          w[1] = v.y;
          w[2] = v.z;
          w[3] = v.w;
        } else if constexpr (VEC == 8) {
          const uint2 v = *reinterpret_cast<const uint2*>(row + s0);
          w[0] = v.x;
          w[1] = v.y;
        } else {
          w[0] = *reinterpret_cast<const unsigned*>(row + s0);
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const unsigned c = (w[j / 4] >> (8 * (j % 4))) & 0xffu;
          acc += lut[(s0 + j) * ncb + c];
        }
      }
    }
    return knn_make_key(acc, (int)item);
  }
};

// Flat: 16 lanes per row, each strides the row (16 bytes at a time when
// VEC4), then a fixed shuffle tree. cand (optional) lists the rows to
// visit; entries outside [0, N) are skipped.
template <bool VEC4, bool IP>
struct KnnFlatSrc {
  static constexpr int LPI = 16;
  static constexpr int R = 16;
  const float* X;
  long stride, N;
  int dim;
  const float* q;   // LDS, [dim]
  const int* cand;  // this query's list, or null

  __device__ __forceinline__ knn_key_t key(long item, long end) const {
    const int lig = threadIdx.x % LPI;
    long row = -1;
    if (item < end) {
      row = cand ? (long)cand[item] : item;
      if (row < 0 || row >= N) row = -1;
    }
    float acc = 0.f;
    if (row >= 0) {
      const float* x = X + row * stride;
      if (VEC4) {
        for (int j = lig * 4; j < dim; j += LPI * 4) {
          const float4 v = *reinterpret_cast<const float4*>(x + j);
          const float4 u = *reinterpret_cast<const float4*>(q + j);
          if (IP) {
            acc += u.x * v.x;
            acc += u.y * v.y;
            acc += u.z * v.z;
            acc += u.w * v.w;
          } else {
            acc += (u.x - v.x) * (u.x - v.x);
            acc += (u.y - v.y) * (u.y - v.y);
            acc += (u.z - v.z) * (u.z - v.z);
            acc += (u.w - v.w) * (u.w - v.w);
          }
        }
      } else {
        for (int j = lig; j < dim; j += LPI) {
          const float d = IP ? 0.f : q[j] - x[j];
          acc += IP ? q[j] * x[j] : d * d;
        }
      }
    }
#pragma unroll
    for (int s = 1; s < LPI; s <<= 1) acc += __shfl_xor(acc, s);
    if (row < 0) return KNN_PAD;
    return knn_make_key(IP ? 0.f - acc : acc, (int)row);
  }
};

// the partial lists of one query, [n_slices * k] keys
struct KnnPartialSrc {
  static constexpr int LPI = 1;
  static constexpr int R = 4;
  const knn_key_t* keys;
  __device__ __forceinline__ knn_key_t key(long item, long end) const {
    return item < end ? keys[item] : KNN_PAD;
  }
};

// ---- kernels ----

// lut[q, s, c] = sum_j (Q[q, s*d+j] - C[s, c, j])^2, or 0 - <.,.>
__global__ __launch_bounds__(KNN_BLOCK) void pq_lut_kernel(
    const float* __restrict__ Q, const float* __restrict__ C,
    float* __restrict__ lut, long total, int n_sub, int ncb, int d_sub,
    int ip) {
  const long i = (long)blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % ncb);
  const int s = (int)((i / ncb) % n_sub);
  const long q = i / ((long)ncb * n_sub);
  const float* qv = Q + (q * n_sub + s) * d_sub;
  const float* cv = C + ((long)s * ncb + c) * d_sub;
  float acc = 0.f;
  for (int j = 0; j < d_sub; ++j) {
    const float d = qv[j] - cv[j];
    acc += ip ? qv[j] * cv[j] : d * d;
  }
  lut[i] = ip ? 0.f - acc : acc;
}

template <int VEC>
__global__ __launch_bounds__(KNN_BLOCK) void pq_adc_topk_kernel(
    const float* __restrict__ lut, const unsigned char* __restrict__ codes,
    long stride, long N, int n_sub, int ncb, int k, long slice_rows,
    int n_slices, knn_key_t* __restrict__ partial, int* __restrict__ ids,
    float* __restrict__ dist) {
  extern __shared__ float s_lut[];
  __shared__ knn_key_t s_keys[KNN_SORT];
  __shared__ int s_cnt;
  const long q = blockIdx.x / n_slices;
  const int sl = blockIdx.x % n_slices;
  const int ln = n_sub * ncb;
  for (int i = threadIdx.x; i < ln; i += KNN_BLOCK)
    s_lut[i] = lut[q * ln + i];
  const long begin = (long)sl * slice_rows;
  const long end = min(N, begin + slice_rows);
  const KnnAdcSrc<VEC> src{codes, stride, n_sub, ncb, s_lut};
  knn_select<KnnAdcSrc<VEC>, false>(src, begin, end, k, s_keys, &s_cnt);
  knn_write(s_keys, k,
            n_slices > 1 ? partial + (q * n_slices + sl) * k : nullptr,
            ids + q * k, dist + q * k);
}

// items are rows of X, or positions of cand[q, 0..R) when CAND
template <bool VEC4, bool IP, bool CAND>
__global__ __launch_bounds__(KNN_BLOCK) void flat_topk_kernel(
    const float* __restrict__ X, long stride, long N, int dim,
    const float* __restrict__ Q, const int* __restrict__ cand, long n_items,
    int k, long slice_rows, int n_slices, knn_key_t* __restrict__ partial,
    int* __restrict__ ids, float* __restrict__ dist) {
  __shared__ __attribute__((aligned(16))) float s_q[KNN_MAX_DIM];
  __shared__ knn_key_t s_keys[KNN_SORT];
  __shared__ int s_cnt;
  const long q = blockIdx.x / n_slices;
  const int sl = blockIdx.x % n_slices;
  for (int i = threadIdx.x; i < dim; i += KNN_BLOCK) s_q[i] = Q[q * dim + i];
  const long begin = (long)sl * slice_rows;
  const long end = min(n_items, begin + slice_rows);
  const KnnFlatSrc<VEC4, IP> src{X,   stride, N,
                                 dim, s_q,    CAND ? cand + q * n_items
                                                   : nullptr};
  knn_select<KnnFlatSrc<VEC4, IP>, CAND>(src, begin, end, k, s_keys, &s_cnt);
  knn_write(s_keys, k,
            n_slices > 1 ? partial + (q * n_slices + sl) * k : nullptr,
            ids + q * k, dist + q * k);
}

// one block per query over its n_slices sorted partial lists
template <bool DEDUP>
__global__ __launch_bounds__(KNN_BLOCK) void knn_merge_kernel(
    const knn_key_t* __restrict__ partial, int n_slices, int k,
    int* __restrict__ ids, float* __restrict__ dist) {
  __shared__ knn_key_t s_keys[KNN_SORT];
  __shared__ int s_cnt;
  const long q = blockIdx.x;
  const long n = (long)n_slices * k;
  const KnnPartialSrc src{partial + q * n};
  knn_select<KnnPartialSrc, DEDUP>(src, 0, n, k, s_keys, &s_cnt);
  knn_write(s_keys, k, nullptr, ids + q * k, dist + q * k);
}

// ---- host side ----

int knn_max_k() { return KNN_MAX_K; }
int knn_max_sub() { return KNN_MAX_SUB; }
int knn_max_dim() { return KNN_MAX_DIM; }

// Rows per slice for n rows and nq queries: enough slices that nq *
// n_slices reaches KNN_TARGET_BLOCKS blocks, never below KNN_MIN_SLICE
// rows, rounded up to KNN_ROUND. n_slices = ceil(n / rows).
long knn_slice_rows(long n, long nq) {
  if (nq < 1) nq = 1;
  if (n < 1) n = 1;
  const long want = (KNN_TARGET_BLOCKS + nq - 1) / nq;
  long rows = (n + want - 1) / want;
  rows = (rows + KNN_ROUND - 1) / KNN_ROUND * KNN_ROUND;
  return rows < KNN_MIN_SLICE ? KNN_MIN_SLICE : rows;
}

// LDS per block of pq_adc_topk: the LUT (dynamic) + keys and counter
long pq_adc_lds_bytes(int n_sub, int ncb) {
  return (long)n_sub * ncb * (long)sizeof(float) +
         (long)KNN_SORT * (long)sizeof(knn_key_t) + 16;
}

void pq_lut_launch(const float* Q, const float* C, float* lut, long nq,
                   int n_sub, int ncb, int d_sub, int ip,
                   hipStream_t stream) {
  const long total = nq * n_sub * ncb;
  if (total <= 0) return;
  const long blocks = (total + KNN_BLOCK - 1) / KNN_BLOCK;
  hipLaunchKernelGGL(pq_lut_kernel, dim3((unsigned)blocks), dim3(KNN_BLOCK),
                     0, stream, Q, C, lut, total, n_sub, ncb, d_sub, ip);
}

static bool knn_aligned(const void* p, long stride_bytes, int a) {
  return ((uintptr_t)p) % a == 0 && stride_bytes % a == 0;
}

void knn_merge_launch(const void* partial, long nq, int n_slices, int k,
                      int dedup, int* ids, float* dist, hipStream_t stream) {
  if (nq <= 0) return;
  if (dedup)
    hipLaunchKernelGGL(knn_merge_kernel<true>, dim3((unsigned)nq),
                       dim3(KNN_BLOCK), 0, stream, (const knn_key_t*)partial,
                       n_slices, k, ids, dist);
  else
    hipLaunchKernelGGL(knn_merge_kernel<false>, dim3((unsigned)nq),
                       dim3(KNN_BLOCK), 0, stream, (const knn_key_t*)partial,
                       n_slices, k, ids, dist);
}

// codes[N, n_sub] uint8 with `stride` bytes between rows. partial (when
// n_slices > 1) is [nq, n_slices, k] 8-byte keys. The widest code load
// that n_sub, the base and the stride allow is chosen for the whole range.
void pq_adc_topk_launch(const float* lut, const unsigned char* codes,
                        long stride, long N, long nq, int n_sub, int ncb,
                        int k, long slice_rows, int n_slices, void* partial,
                        int* ids, float* dist, hipStream_t stream) {
  if (nq <= 0) return;
  const dim3 grid((unsigned)(nq * n_slices)), block(KNN_BLOCK);
  const size_t lds = (size_t)n_sub * ncb * sizeof(float);
#define KNN_ADC(V)                                                          \
  hipLaunchKernelGGL(pq_adc_topk_kernel<V>, grid, block, lds, stream, lut,  \
                     codes, stride, N, n_sub, ncb, k, slice_rows, n_slices, \
                     (knn_key_t*)partial, ids, dist)
  if (n_sub % 16 == 0 && knn_aligned(codes, stride, 16)) {
    KNN_ADC(16);
  } else if (n_sub % 8 == 0 && knn_aligned(codes, stride, 8)) {
    KNN_ADC(8);
  } else if (n_sub % 4 == 0 && knn_aligned(codes, stride, 4)) {
    KNN_ADC(4);
  } else {
    KNN_ADC(1);
  }
#undef KNN_ADC
}

// X[N, dim] fp32 with `stride` floats between rows; cand (optional) is
// [nq, n_items] int32, otherwise n_items == N.
void flat_topk_launch(const float* X, long stride, long N, int dim,
                      const float* Q, long nq, const int* cand, long n_items,
                      int ip, int k, long slice_rows, int n_slices,
                      void* partial, int* ids, float* dist,
                      hipStream_t stream) {
  if (nq <= 0) return;
  const dim3 grid((unsigned)(nq * n_slices)), block(KNN_BLOCK);
  const bool vec = dim % 4 == 0 && knn_aligned(X, stride * 4, 16);
#define KNN_FLAT(V, I, C)                                                  \
  hipLaunchKernelGGL((flat_topk_kernel<V, I, C>), grid, block, 0, stream,  \
                     X, stride, N, dim, Q, cand, n_items, k, slice_rows,   \
                     n_slices, (knn_key_t*)partial, ids, dist)
#define KNN_FLAT_C(V, I)   \
  if (cand) {              \
    KNN_FLAT(V, I, true);  \
  } else {                 \
    KNN_FLAT(V, I, false); \
  }
  if (vec && ip) {
    KNN_FLAT_C(true, true)
  } else if (vec) {
    KNN_FLAT_C(true, false)
  } else if (ip) {
    KNN_FLAT_C(false, true)
  } else {
    KNN_FLAT_C(false, false)
  }
#undef KNN_FLAT_C
#undef KNN_FLAT
}

// ---- random-projection forest: candidate lists (predict/rp_forest.py) ----
//
// One wavefront walks the whole forest for one query with a best-first
// queue of (bound, code) entries; a code is an inner node i >= 0 or
// -1 - l for leaf l. Queue order: larger bound first (float `<`, so -0 and
// +0 tie), ties to the lower signed code. An entry is one 64-bit key, high
// word -bound through knn_make_key's float mapping, low word code ^ 2^31,
// so the unsigned key order is the queue order and the first entry is the
// smallest key. The queue is an unordered array of FOREST_QUEUE keys per
// wave in LDS: pop is a wave-wide min over the live prefix (the last entry
// fills the hole), a push into a full queue is a wave-wide max and replace.
// The query sits in registers, lane-strided; a plane row is read coalesced
// and reduced with a fixed shuffle tree, the bias is added last. Every
// queue decision is taken from values every lane holds alike; there are no
// atomics, and no block barrier (waves of a block share nothing).
//
// Guards for a malformed forest: every code read from memory is
// range-checked before it is queued, leaf bounds before they are used, the
// pop loop runs at most n_inner + n_leaves + T times and every store is
// inside the row of `width` slots.

#define FOREST_WAVES (KNN_BLOCK / LCTR_WAVE)
#define FOREST_QUEUE 1024
#define FOREST_MAX_SEARCH 65536
#define FOREST_QREGS (KNN_MAX_DIM / LCTR_WAVE)

__device__ __forceinline__ knn_key_t forest_key(float bound, int code) {
  return knn_make_key(-bound, (int)((unsigned)code ^ 0x80000000u));
}

// orders one lane's LDS writes before the other lanes' reads (same wave)
__device__ __forceinline__ void forest_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// wave-wide min or max of 64-bit keys; every lane gets the same key
template <bool MAX>
__device__ __forceinline__ knn_key_t forest_wave_extreme(knn_key_t v) {
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, s);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), s);
    const knn_key_t o = ((knn_key_t)hi << 32) | lo;
    v = MAX ? (o > v ? o : v) : (o < v ? o : v);
  }
  return v;
}

__device__ __forceinline__ int forest_uniform(int v) {
  return __builtin_amdgcn_readfirstlane(v);
}

// the lowest lane whose flag is set (one is)
__device__ __forceinline__ int forest_first_lane(bool flag) {
  return __ffsll((unsigned long long)__ballot(flag)) - 1;
}

__device__ __forceinline__ void forest_push(knn_key_t* qu, int& n,
                                            knn_key_t key, int lane) {
  if (n < FOREST_QUEUE) {
    if (lane == 0) qu[n] = key;
    ++n;
  } else {
    // full: whichever of the FOREST_QUEUE + 1 entries is last goes
    knn_key_t worst = 0;
    int slot = lane;
    for (int j = lane; j < FOREST_QUEUE; j += LCTR_WAVE) {
      const knn_key_t e = qu[j];
      if (e >= worst) {
        worst = e;
        slot = j;
      }
    }
    const knn_key_t w = forest_wave_extreme<true>(worst);
    const int owner = forest_first_lane(worst == w);
    if (key < w && lane == owner) qu[slot] = key;
  }
  forest_wave_sync();
}

// removes and returns the first entry of a queue of n >= 1 entries
__device__ __forceinline__ knn_key_t forest_pop(knn_key_t* qu, int& n,
                                                int lane) {
  knn_key_t best = KNN_PAD;
  int slot = 0;
  for (int j = lane; j < n; j += LCTR_WAVE) {
    const knn_key_t e = qu[j];
    if (e <= best) {
      best = e;
      slot = j;
    }
  }
  const knn_key_t b = forest_wave_extreme<false>(best);
  const int owner = forest_first_lane(best == b && lane < n);
  const int hole = __shfl(slot, owner);
  const knn_key_t last = qu[n - 1];
  forest_wave_sync();  // everyone has read the queue
  --n;
  if (lane == 0 && hole < n) qu[hole] = last;
  forest_wave_sync();
  return b;
}

__device__ __forceinline__ bool forest_code_ok(int c, int n_inner,
                                               int n_leaves) {
  return c >= 0 ? c < n_inner : -1 - c < n_leaves;
}

__global__ __launch_bounds__(KNN_BLOCK) void forest_candidates_kernel(
    const float* __restrict__ planes, const float* __restrict__ bias,
    const int* __restrict__ child, const int* __restrict__ roots,
    const int* __restrict__ leaf_off, const int* __restrict__ leaf_items,
    const float* __restrict__ Q, int* __restrict__ cand, long nq, int dim,
    int n_inner, int n_leaves, int T, long total, int search_k, long width) {
  __shared__ knn_key_t s_queue[FOREST_WAVES][FOREST_QUEUE];
  const int lane = threadIdx.x % LCTR_WAVE;
  const int wave = forest_uniform(threadIdx.x / LCTR_WAVE);
  const long q = (long)blockIdx.x * FOREST_WAVES + wave;
  if (q >= nq) return;
  knn_key_t* qu = s_queue[wave];
  int* row = cand + q * width;

  float qr[FOREST_QREGS];
#pragma unroll
  for (int r = 0; r < FOREST_QREGS; ++r) {
    const int j = lane + r * LCTR_WAVE;
    qr[r] = j < dim ? Q[q * dim + j] : 0.f;
  }

  int n = 0;
  const float inf = __uint_as_float(0x7f800000u);
  for (int t = 0; t < T; ++t) {
    const int c = roots[t];
    if (forest_code_ok(c, n_inner, n_leaves))
      forest_push(qu, n, forest_key(inf, c), lane);
  }

  long written = 0;
  long budget = (long)n_inner + n_leaves + T;
  while (n > 0 && written < search_k && budget-- > 0) {
    const knn_key_t key = forest_pop(qu, n, lane);
    const unsigned klo = (unsigned)forest_uniform((int)(unsigned)key);
    const unsigned khi = (unsigned)forest_uniform((int)(unsigned)(key >> 32));
    const float bound = -knn_key_dist((knn_key_t)khi << 32);
    const int code = (int)(klo ^ 0x80000000u);
    if (code < 0) {
      const int l = -1 - code;
      const long beg = leaf_off[l], end = leaf_off[l + 1];
      if (beg < 0 || end < beg || end > total) continue;
      for (long j = lane; j < end - beg; j += LCTR_WAVE)
        if (written + j < width) row[written + j] = leaf_items[beg + j];
      written += end - beg;
    } else {
      const float* p = planes + (long)code * dim;
      const int c0 = child[2 * (long)code], c1 = child[2 * (long)code + 1];
      const float bi = bias[code];
      float acc = 0.f;
#pragma unroll
      for (int r = 0; r < FOREST_QREGS; ++r) {
        if (r * LCTR_WAVE >= dim) break;
        const int j = lane + r * LCTR_WAVE;
        if (j < dim) acc += p[j] * qr[r];
      }
      float m = wave_reduce_sum(acc) + bi;
      m = __uint_as_float((unsigned)forest_uniform((int)__float_as_uint(m)));
      const float am = fabsf(m);
      const int near = m > 0.f ? c0 : c1, far = m > 0.f ? c1 : c0;
      if (forest_code_ok(near, n_inner, n_leaves))
        forest_push(qu, n, forest_key(fminf(bound, am), near), lane);
      if (forest_code_ok(far, n_inner, n_leaves))
        forest_push(qu, n, forest_key(fminf(bound, -am), far), lane);
    }
  }
  for (long j = written + lane; j < width; j += LCTR_WAVE) row[j] = -1;
}

int forest_queue() { return FOREST_QUEUE; }
int forest_max_search() { return FOREST_MAX_SEARCH; }

// cand is [nq, width] int32; the forest arrays are those of
// predict/rp_forest.py (child is [n_inner, 2])
void forest_candidates_launch(const float* planes, const float* bias,
                              const int* child, const int* roots,
                              const int* leaf_off, const int* leaf_items,
                              const float* Q, int* cand, long nq, int dim,
                              int n_inner, int n_leaves, int T, long total,
                              int search_k, long width, hipStream_t stream) {
  if (nq <= 0) return;
  const long blocks = (nq + FOREST_WAVES - 1) / FOREST_WAVES;
  hipLaunchKernelGGL(forest_candidates_kernel, dim3((unsigned)blocks),
                     dim3(KNN_BLOCK), 0, stream, planes, bias, child, roots,
                     leaf_off, leaf_items, Q, cand, nq, dim, n_inner,
                     n_leaves, T, total, search_k, width);
}

}  // namespace lightctr
