// Parameter-server dense-table kernels for MI355X/gfx950.
//
// The PS keeps the dense (MLP) weights of all workers as one flat fp32 slab
// per shard (reference tensorShardTable, distribut/paramserver.h:40-47, 'T'
// pull/push branches :146-165, :220-240). A dense push is a streaming
// read-modify-write over the whole slab, so unlike ps_apply_kernel (one wave
// per key, indexed) these are plain memory-bound streaming kernels:
//
//   ps_dense_check  non-finite scan of the wire payload -> device flag
//   ps_dense_apply  wire decode + updater + slab/accumulator/shadow stores in
//                   one pass, gated on the flag (a flagged push is dropped
//                   and counted on device; the host never syncs)
//   ps_dense_pack   slab -> fp32/fp16 pull payload, + shadow[wi] = slab
//
// wire: 0 = fp32, 1 = fp16, 2 = uint8 codes (table[code] * scale[0]).
// updater: 0=sgd, 1=adagrad, 2=dcasgd, 3=dcasgda — the elementwise math of
// ps_apply_kernel.
//
// 256-thread blocks, grid capped at 2048 blocks, grid-stride loops; four
// elements per lane per trip (16 B on the fp32 streams, 8 B fp16, 4 B
// codes) when every base pointer is aligned for it, otherwise (e.g. a slab
// view starting at element 1) the one-element-per-lane body runs over the
// whole range. The launchers decide from the pointer values. The <4-element
// remainder is a scalar tail.
#include <hip/hip_fp16.h>

#include <cstdint>

#include "common.h"

namespace lightctr {

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 2048;
constexpr int kMaxLevels = 256;

// flags[0]: current push is corrupt; flags[1]: dropped-push counter.

__device__ __forceinline__ bool nonfinite_f32(float v) {
  return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u;
}
__device__ __forceinline__ bool nonfinite_f16bits(unsigned int h) {
  return (h & 0x7c00u) == 0x7c00u;
}

// Block-wide "any lane bad" -> one atomic per block.
__device__ __forceinline__ void block_flag(bool bad, int* flags) {
  __shared__ int blk_bad;
  if (threadIdx.x == 0) blk_bad = 0;
  __syncthreads();
  if (__any(bad) && (threadIdx.x & (LCTR_WAVE - 1)) == 0) blk_bad = 1;
  __syncthreads();
  if (threadIdx.x == 0 && blk_bad) atomicOr(&flags[0], 1);
}

template <int WIRE>
struct Wire;
template <>
struct Wire<0> { using T = float; };
template <>
struct Wire<1> { using T = __half; };
template <>
struct Wire<2> { using T = unsigned char; };

template <int WIRE>
__device__ __forceinline__ float decode1(const typename Wire<WIRE>::T* p,
                                         long i, const float* tab,
                                         float scale) {
  if constexpr (WIRE == 0) {
    return p[i];
  } else if constexpr (WIRE == 1) {
    return __half2float(p[i]);
  } else {
    return tab[p[i]] * scale;
  }
}

// four consecutive wire values starting at element 4*v (aligned bases only)
template <int WIRE>
__device__ __forceinline__ float4 decode4(const typename Wire<WIRE>::T* p,
                                          long v, const float* tab,
                                          float scale) {
  if constexpr (WIRE == 0) {
    return reinterpret_cast<const float4*>(p)[v];
  } else if constexpr (WIRE == 1) {
    const uint2 raw = reinterpret_cast<const uint2*>(p)[v];
    const __half2 lo = *reinterpret_cast<const __half2*>(&raw.x);
    const __half2 hi = *reinterpret_cast<const __half2*>(&raw.y);
    const float2 a = __half22float2(lo), b = __half22float2(hi);
    return make_float4(a.x, a.y, b.x, b.y);
  } else {
    const unsigned int raw = reinterpret_cast<const unsigned int*>(p)[v];
    return make_float4(tab[raw & 0xffu] * scale,
                       tab[(raw >> 8) & 0xffu] * scale,
                       tab[(raw >> 16) & 0xffu] * scale,
                       tab[raw >> 24] * scale);
  }
}

// One element of the updater family (PSShard._apply math). w: weight,
// a: accumulator (UPD 1, 3), s: this worker's shadow (UPD 2, 3).
template <int UPD>
__device__ __forceinline__ void update1(float& w, float& a, float& s, float g,
                                        float lr, float lam, float eps) {
  if constexpr (UPD == 0) {
    w -= lr * g;
  } else if constexpr (UPD == 1) {
    a += g * g;
    w -= lr * g * __frsqrt_rn(a + eps);
  } else {
    float l = lam;
    if constexpr (UPD == 3) {
      a = 0.95f * a + 0.05f * g * g;
      l = lam * __frsqrt_rn(a + eps);
    }
    w = w - lr * (g + l * g * g * (w - s));
    s = w;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// check
// ---------------------------------------------------------------------------
template <int WIRE>
__global__ void __launch_bounds__(kBlock)
ps_dense_check_kernel(const typename Wire<WIRE>::T* __restrict__ payload,
                      long n, int vec, int* __restrict__ flags) {
  static_assert(WIRE == 0 || WIRE == 1, "codes are checked via the table");
  const long tid = (long)blockIdx.x * kBlock + threadIdx.x;
  const long stride = (long)gridDim.x * kBlock;
  bool bad = false;
  const long nvec = vec ? n / 4 : 0;
  for (long v = tid; v < nvec; v += stride) {
    if constexpr (WIRE == 0) {
      const float4 x = reinterpret_cast<const float4*>(payload)[v];
      bad |= nonfinite_f32(x.x) | nonfinite_f32(x.y) | nonfinite_f32(x.z) |
             nonfinite_f32(x.w);
    } else {
      const uint2 x = reinterpret_cast<const uint2*>(payload)[v];
      bad |= nonfinite_f16bits(x.x) | nonfinite_f16bits(x.x >> 16) |
             nonfinite_f16bits(x.y) | nonfinite_f16bits(x.y >> 16);
    }
  }
  for (long i = nvec * 4 + tid; i < n; i += stride) {
    if constexpr (WIRE == 0) {
      bad |= nonfinite_f32(payload[i]);
    } else {
      bad |= nonfinite_f16bits(
          reinterpret_cast<const unsigned short*>(payload)[i]);
    }
  }
  block_flag(bad, flags);
}

// int8 wire: every decoded value is one of the (<= 256) products
// table[j] * scale, so checking those products (the exact expression the
// apply kernel decodes with, overflow of a finite scale times a finite
// entry included) and the scale covers any code sequence. One block. A
// push is flagged if ANY table entry decodes non-finite, used or not.
__global__ void __launch_bounds__(kBlock)
ps_dense_check_codes_kernel(const float* __restrict__ scale,
                            const float* __restrict__ table, int levels,
                            int* __restrict__ flags) {
  const float s = scale[0];
  bool bad = nonfinite_f32(s);
  for (int i = threadIdx.x; i < levels; i += kBlock)
    bad |= nonfinite_f32(table[i] * s);
  block_flag(bad, flags);
}

// ---------------------------------------------------------------------------
// apply
// ---------------------------------------------------------------------------
template <int WIRE, int UPD>
__global__ void __launch_bounds__(kBlock)
ps_dense_apply_kernel(const typename Wire<WIRE>::T* __restrict__ payload,
                      const float* __restrict__ scale_p,
                      const float* __restrict__ table, int levels,
                      float* __restrict__ slab, float* __restrict__ acc,
                      float* __restrict__ shadow, long n, int vec, float lr,
                      float lam, float eps, int* __restrict__ flags) {
  // Dropped push: every block sees the same flag and leaves state untouched.
  if (flags[0] != 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) flags[1] += 1;
    return;
  }
  __shared__ float tab[kMaxLevels];
  float scale = 1.f;
  if constexpr (WIRE == 2) {
    for (int i = threadIdx.x; i < kMaxLevels; i += kBlock)
      tab[i] = i < levels ? table[i] : 0.f;
    __syncthreads();
    scale = scale_p[0];
  }
  constexpr bool HAS_ACC = (UPD == 1 || UPD == 3);
  constexpr bool HAS_SH = (UPD == 2 || UPD == 3);
  const long tid = (long)blockIdx.x * kBlock + threadIdx.x;
  const long stride = (long)gridDim.x * kBlock;
  const long nvec = vec ? n / 4 : 0;
  for (long v = tid; v < nvec; v += stride) {
    const float4 g = decode4<WIRE>(payload, v, tab, scale);
    float4 w = reinterpret_cast<float4*>(slab)[v];
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), s = a;
    if constexpr (HAS_ACC) a = reinterpret_cast<float4*>(acc)[v];
    if constexpr (HAS_SH) s = reinterpret_cast<float4*>(shadow)[v];
    update1<UPD>(w.x, a.x, s.x, g.x, lr, lam, eps);
    update1<UPD>(w.y, a.y, s.y, g.y, lr, lam, eps);
    update1<UPD>(w.z, a.z, s.z, g.z, lr, lam, eps);
    update1<UPD>(w.w, a.w, s.w, g.w, lr, lam, eps);
    reinterpret_cast<float4*>(slab)[v] = w;
    if constexpr (HAS_ACC) reinterpret_cast<float4*>(acc)[v] = a;
    if constexpr (HAS_SH) reinterpret_cast<float4*>(shadow)[v] = s;
  }
  for (long i = nvec * 4 + tid; i < n; i += stride) {
    const float g = decode1<WIRE>(payload, i, tab, scale);
    float w = slab[i], a = 0.f, s = 0.f;
    if constexpr (HAS_ACC) a = acc[i];
    if constexpr (HAS_SH) s = shadow[i];
    update1<UPD>(w, a, s, g, lr, lam, eps);
    slab[i] = w;
    if constexpr (HAS_ACC) acc[i] = a;
    if constexpr (HAS_SH) shadow[i] = s;
  }
}

// ---------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------
template <bool FP16>
__global__ void __launch_bounds__(kBlock)
ps_dense_pack_kernel(const float* __restrict__ slab, void* __restrict__ out,
                     float* __restrict__ shadow, long n, int vec) {
  const long tid = (long)blockIdx.x * kBlock + threadIdx.x;
  const long stride = (long)gridDim.x * kBlock;
  const long nvec = vec ? n / 4 : 0;
  for (long v = tid; v < nvec; v += stride) {
    const float4 w = reinterpret_cast<const float4*>(slab)[v];
    if constexpr (FP16) {
      const __half2 lo = __floats2half2_rn(w.x, w.y);
      const __half2 hi = __floats2half2_rn(w.z, w.w);
      uint2 raw;
      raw.x = *reinterpret_cast<const unsigned int*>(&lo);
      raw.y = *reinterpret_cast<const unsigned int*>(&hi);
      reinterpret_cast<uint2*>(out)[v] = raw;
    } else {
      reinterpret_cast<float4*>(out)[v] = w;
    }
    if (shadow) reinterpret_cast<float4*>(shadow)[v] = w;
  }
  for (long i = nvec * 4 + tid; i < n; i += stride) {
    const float w = slab[i];
    if constexpr (FP16) {
      reinterpret_cast<__half*>(out)[i] = __float2half_rn(w);
    } else {
      reinterpret_cast<float*>(out)[i] = w;
    }
    if (shadow) shadow[i] = w;
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
namespace {

inline bool aligned_to(const void* p, uintptr_t a) {
  return p == nullptr || (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0;
}

inline uintptr_t wire_vec_bytes(int wire) {
  return wire == 0 ? 16 : (wire == 1 ? 8 : 4);
}

// lanes needed: one per 4-element vector (the <4-element tail runs on the
// first lanes of block 0, which always exist), or one per element
inline dim3 dense_grid(long n, bool vec) {
  const long lanes = vec ? n / 4 : n;
  long blocks = (lanes + kBlock - 1) / kBlock;
  if (blocks < 1) blocks = 1;
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  return dim3((unsigned)blocks);
}

}  // namespace

void ps_dense_check_launch(const void* payload, int wire, const float* scale,
                           const float* table, int levels, long n,
                           int* flags, hipStream_t stream) {
  LCTR_CHECK_HIP(hipMemsetAsync(flags, 0, sizeof(int), stream));
  if (wire == 2) {
    hipLaunchKernelGGL(ps_dense_check_codes_kernel, dim3(1), dim3(kBlock), 0,
                       stream, scale, table, levels, flags);
    return;
  }
  const bool vec = aligned_to(payload, wire_vec_bytes(wire));
  const dim3 grid = dense_grid(n, vec);
  if (wire == 0) {
    hipLaunchKernelGGL(ps_dense_check_kernel<0>, grid, dim3(kBlock), 0,
                       stream, (const float*)payload, n, (int)vec, flags);
  } else {
    hipLaunchKernelGGL(ps_dense_check_kernel<1>, grid, dim3(kBlock), 0,
                       stream, (const __half*)payload, n, (int)vec, flags);
  }
}

#define LCTR_DENSE_APPLY(WIRE, UPD)                                          \
  hipLaunchKernelGGL((ps_dense_apply_kernel<WIRE, UPD>), grid, dim3(kBlock), \
                     0, stream, (const Wire<WIRE>::T*)payload, scale, table, \
                     levels, slab, acc, shadow, n, (int)vec, lr, lam, eps,   \
                     flags)
#define LCTR_DENSE_APPLY_UPD(WIRE)                                  \
  switch (updater) {                                                \
    case 0: LCTR_DENSE_APPLY(WIRE, 0); break;                       \
    case 1: LCTR_DENSE_APPLY(WIRE, 1); break;                       \
    case 2: LCTR_DENSE_APPLY(WIRE, 2); break;                       \
    default: LCTR_DENSE_APPLY(WIRE, 3); break;                      \
  }

void ps_dense_apply_launch(const void* payload, int wire, const float* scale,
                           const float* table, int levels, float* slab,
                           float* acc, float* shadow, long n, int updater,
                           float lr, float lam, float eps, int* flags,
                           hipStream_t stream) {
  if (n <= 0) return;
  const bool vec = aligned_to(payload, wire_vec_bytes(wire)) &&
                   aligned_to(slab, 16) && aligned_to(acc, 16) &&
                   aligned_to(shadow, 16);
  const dim3 grid = dense_grid(n, vec);
  if (wire == 0) {
    LCTR_DENSE_APPLY_UPD(0)
  } else if (wire == 1) {
    LCTR_DENSE_APPLY_UPD(1)
  } else {
    LCTR_DENSE_APPLY_UPD(2)
  }
}
#undef LCTR_DENSE_APPLY_UPD
#undef LCTR_DENSE_APPLY

void ps_dense_pack_launch(const float* slab, void* out, int fp16,
                          float* shadow, long n, hipStream_t stream) {
  if (n <= 0) return;
  const bool vec = aligned_to(slab, 16) && aligned_to(out, fp16 ? 8 : 16) &&
                   aligned_to(shadow, 16);
  const dim3 grid = dense_grid(n, vec);
  if (fp16) {
    hipLaunchKernelGGL(ps_dense_pack_kernel<true>, grid, dim3(kBlock), 0,
                       stream, slab, out, shadow, n, (int)vec);
  } else {
    hipLaunchKernelGGL(ps_dense_pack_kernel<false>, grid, dim3(kBlock), 0,
                       stream, slab, out, shadow, n, (int)vec);
  }
}

}  // namespace lightctr
