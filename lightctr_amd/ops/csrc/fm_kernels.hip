// Fused FM (factorization machine) kernels for MI355X / gfx950.
//
// Capability parity with the reference FM trainer
// (/root/reference/LightCTR/train/train_fm_algo.cpp:63-127: forward via the
// O(nk) sumVX trick, backward gradV = d*(sumVX - v*x)*x, Adagrad apply;
// FTRL per reference util/gradientUpdater.h:235-278) — redesigned for CDNA4:
//   * one 64-lane wavefront per CSR row; lane = (feature_group, factor k)
//     so a wave gathers G=64/K embedding rows in parallel, K floats each
//   * cross-lane combine via __shfl_xor (no LDS round trip needed at K<=64)
//   * backward scatters into dense per-feature gradient slabs with fp32
//     atomics + a touched-bitmap; a compaction kernel turns the bitmap into
//     a unique-fid list; the optimizer (Adagrad / FTRL) is a separate fused
//     kernel over that list only (sparse apply, zero host round trips).
//
// All buffers live in HBM3E; the whole step is 5 kernel launches and is
// hipGraph-capturable (no device->host syncs).
#include <algorithm>
#include <cstdio>
#include "common.h"

namespace lightctr {

// Optimizer update bodies, on register values: every FM kernel that applies
// an update (sparse apply over a fid list, the walk's fused flush, the
// segment reduce) loads the state, calls one of these and stores it back,
// so the arithmetic exists once.
//
// FTRL-proximal (per-coordinate), semantics of the reference FTRL updater
// (gradientUpdater.h:235-278): z,n state per parameter.
__device__ __forceinline__ void ftrl_step(float& w, float& z, float& n,
                                          float g, float alpha, float beta,
                                          float l1, float l2) {
  const float g2 = g * g;
  const float nold = n;
  const float sigma = (sqrtf(nold + g2) - sqrtf(nold)) / alpha;
  const float znew = z + g - sigma * w;
  const float nnew = nold + g2;
  z = znew;
  n = nnew;
  if (fabsf(znew) <= l1) {
    w = 0.f;
  } else {
    w = -(znew - copysignf(l1, znew)) / ((beta + sqrtf(nnew)) / alpha + l2);
  }
}

// Adagrad with L2 folded into the gradient.
__device__ __forceinline__ void adagrad_step(float& w, float& n, float g_in,
                                             float lr, float eps, float l2) {
  const float g = g_in + l2 * w;
  const float a = n + g * g;
  n = a;
  w -= lr * g * __frsqrt_rn(a + eps);
}

__device__ __forceinline__ void ftrl_update(float* __restrict__ w,
                                            float* __restrict__ z,
                                            float* __restrict__ n, float g,
                                            float alpha, float beta, float l1,
                                            float l2) {
  float wv = *w, zv = *z, nv = *n;
  ftrl_step(wv, zv, nv, g, alpha, beta, l1, l2);
  *z = zv;
  *n = nv;
  *w = wv;
}

__device__ __forceinline__ void adagrad_update(float* __restrict__ w,
                                               float* __restrict__ n, float g,
                                               float lr, float eps,
                                               float l2) {
  float wv = *w, nv = *n;
  adagrad_step(wv, nv, g, lr, eps, l2);
  *n = nv;
  *w = wv;
}

// Optimizer state + knobs for the kernels that fuse the update into the
// gradient reduction. opt_mode: 1 = Adagrad, 2 = FTRL, 3 = FTRL on W +
// Adagrad on V (the default FM pairing, models/fm.py ftrl_v="adagrad").
struct FmOptArgs {
  float* W;
  float* nW;
  float* zW;
  float* nV;
  float* zV;
  float p0, p1, p2, p3;  // adagrad: lr, eps, l2 | ftrl: alpha, beta, l1, l2
  float q0, q1, q2;      // opt_mode 3, V side: v_lr, v_eps, v_l2
};

// one latent factor / one linear weight under opt_mode (z unused by Adagrad)
__device__ __forceinline__ void fm_opt_step_v(int opt_mode, float& v,
                                              float& n, float& z, float g,
                                              const FmOptArgs& oa) {
  if (opt_mode == 1) {
    adagrad_step(v, n, g, oa.p0, oa.p1, oa.p2);
  } else if (opt_mode == 3) {
    adagrad_step(v, n, g, oa.q0, oa.q1, oa.q2);
  } else {
    ftrl_step(v, z, n, g, oa.p0, oa.p1, oa.p2, oa.p3);
  }
}

__device__ __forceinline__ void fm_opt_step_w(int opt_mode, float& w,
                                              float& n, float& z, float g,
                                              const FmOptArgs& oa) {
  if (opt_mode == 1) {
    adagrad_step(w, n, g, oa.p0, oa.p1, oa.p2);
  } else {
    ftrl_step(w, z, n, g, oa.p0, oa.p1, oa.p2, oa.p3);
  }
}

// Stable logloss + upstream gradient of one row: the one place this maths
// lives (logloss_grad_kernel and the training forward both call it).
//   loss  = max(z,0) - z*y + log(1+exp(-|z|))
//   dpred = (sigmoid(z) - y) * scale
__device__ __forceinline__ void logloss_grad_row(float z, float y, float scale,
                                                 float& loss, float& dpred) {
  loss = fmaxf(z, 0.f) - z * y + __logf(1.f + __expf(-fabsf(z)));
  dpred = (sigmoidf_clamped(z) - y) * scale;
}

// ---------------------------------------------------------------------------
// Forward: pred[row] = sum_j w[fid]*x + 0.5*(||sumVX||^2 - sum_j ||v*x||^2)
// Also writes sumVX[row*K+k] (needed by backward).
// ---------------------------------------------------------------------------
// Row body shared by the inference and the training forward. REC adds the
// per-entry record rec[j] = {row, bits of vals[j]} (written by the k == 0
// lane of the feature group that has just loaded vals[j]): the segment
// backward sorts these records by fid and recomputes each entry's gradient
// from them, so no per-entry gradient buffer is ever written. The records
// are pure batch data: fm_records_kernel writes the same ones without the
// model and the CSR-fed sort of sort_kernels.hip makes them in registers in
// its first pass, which lets the sort run beside a forward that has REC off.
// Returns the row's pred (valid in every lane).
template <int K, bool REC>
__device__ __forceinline__ float fm_forward_row(
    const int* __restrict__ row_ptr, const int* __restrict__ fids,
    const float* __restrict__ vals, const float* __restrict__ W,
    const float* __restrict__ V, float* __restrict__ sumVX,
    int2* __restrict__ rec, int row, int lane) {
  constexpr int G = LCTR_WAVE / K;  // features processed in parallel
  const int g = lane / K;
  const int k = lane % K;
  const int beg = row_ptr[row], end = row_ptr[row + 1];

  float sVX = 0.f;    // partial sum_j V[fid,k]*x over this lane's features
  float sV2X2 = 0.f;  // partial sum_j (V[fid,k]*x)^2
  float lin = 0.f;    // partial sum_j W[fid]*x (k==0 lanes only)
  // 4-deep pipelined gathers (same latency argument as the emit kernel)
  int j = beg + g;
  for (; j + 3 * G < end; j += 4 * G) {
    int f[4];
    float x[4], v[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      f[u] = fids[j + u * G];
      x[u] = vals[j + u * G];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = V[(size_t)f[u] * K + k];
      w[u] = (k == 0) ? W[f[u]] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (REC && k == 0)
        rec[j + u * G] = make_int2(row, __float_as_int(x[u]));
      const float vx = v[u] * x[u];
      sVX += vx;
      sV2X2 += vx * vx;
      lin = fmaf(w[u], x[u], lin);
    }
  }
  for (; j < end; j += G) {
    const int fid = fids[j];
    const float x = vals[j];
    if (REC && k == 0) rec[j] = make_int2(row, __float_as_int(x));
    const float vx = V[(size_t)fid * K + k] * x;
    sVX += vx;
    sV2X2 += vx * vx;
    if (k == 0) lin = fmaf(W[fid], x, lin);
  }
  // combine feature groups: lanes {k, K+k, 2K+k, ...} sum -> every lane
  // holds the row's total sumVX for its k (replicated G times).
  sVX = group_reduce_sum<K>(sVX);
  const float t = sVX * sVX;  // replicated G times per k
  const float tot_t = wave_reduce_sum(t) * (1.f / G);
  const float tot_v2 = wave_reduce_sum(sV2X2);
  const float tot_lin = wave_reduce_sum(lin);
  if (lane < K) sumVX[(size_t)row * K + lane] = sVX;
  return tot_lin + 0.5f * (tot_t - tot_v2);
}

template <int K>
__global__ void fm_forward_kernel(const int* __restrict__ row_ptr,
                                  const int* __restrict__ fids,
                                  const float* __restrict__ vals,
                                  const float* __restrict__ W,
                                  const float* __restrict__ V,
                                  float* __restrict__ pred,
                                  float* __restrict__ sumVX, int B) {
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int row = blockIdx.x * (blockDim.x / LCTR_WAVE) + (threadIdx.x >> 6);
  if (row >= B) return;
  const float p = fm_forward_row<K, false>(row_ptr, fids, vals, W, V, sumVX,
                                           nullptr, row, lane);
  if (lane == 0) pred[row] = p;
}

// Training forward: the row body above plus, in lane 0, the loss and the
// upstream gradient of the row (what logloss_grad_kernel computes from a
// stored pred), and, with REC, the per-entry records for the segment backward.
template <int K, bool REC>
__global__ void fm_forward_train_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fids,
    const float* __restrict__ vals, const float* __restrict__ W,
    const float* __restrict__ V, const float* __restrict__ label, float scale,
    float* __restrict__ loss, float* __restrict__ dpred,
    float* __restrict__ sumVX, int2* __restrict__ rec, int B,
    int* __restrict__ reset) {
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int row = blockIdx.x * (blockDim.x / LCTR_WAVE) + (threadIdx.x >> 6);
  // the spill counter of the segment backward that follows in the stream
  if (reset != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *reset = 0;
  if (row >= B) return;
  const float p = fm_forward_row<K, REC>(row_ptr, fids, vals, W, V, sumVX,
                                         rec, row, lane);
  if (lane == 0) {
    float l, d;
    logloss_grad_row(p, label[row], scale, l, d);
    loss[row] = l;
    dpred[row] = d;
  }
}

// The records alone: rec[j] = {row of j, bits of vals[j]}, one wave per row,
// lanes striding over the row (empty rows write nothing). Feeds the sorts that
// do not make the records themselves, and is the reference for the ones that
// do.
__global__ void fm_records_kernel(const int* __restrict__ row_ptr,
                                  const float* __restrict__ vals,
                                  int2* __restrict__ rec, int B) {
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int row = blockIdx.x * (blockDim.x / LCTR_WAVE) + (threadIdx.x >> 6);
  if (row >= B) return;
  const int end = row_ptr[row + 1];
  for (int j = row_ptr[row] + lane; j < end; j += LCTR_WAVE)
    rec[j] = make_int2(row, __float_as_int(vals[j]));
}

// ---------------------------------------------------------------------------
// Loss: numerically stable logloss + dpred = (sigmoid(pred) - y) * scale.
// Writes per-row loss (host reduces with a library sum) and the upstream
// gradient used by the backward kernel. Also emits correct-count bits for
// accuracy if acc != nullptr.
// ---------------------------------------------------------------------------
__global__ void logloss_grad_kernel(const float* __restrict__ pred,
                                    const float* __restrict__ label,
                                    float* __restrict__ loss,
                                    float* __restrict__ dpred, float scale,
                                    int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  float l, d;
  logloss_grad_row(pred[i], label[i], scale, l, d);
  loss[i] = l;
  dpred[i] = d;
}

// ---------------------------------------------------------------------------
// Backward: scatter-accumulate per-feature grads with fp32 atomics.
//   gradW[fid]    += d * x
//   gradV[fid,k]  += d * (sumVX[k]*x - V[fid,k]*x^2)
// Marks fid in a 64-bit touched bitmap for the sparse optimizer pass.
// ---------------------------------------------------------------------------
template <int K>
__global__ void fm_backward_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fids,
    const float* __restrict__ vals, const float* __restrict__ V,
    const float* __restrict__ sumVX, const float* __restrict__ dpred,
    float* __restrict__ gradW, float* __restrict__ gradV,
    unsigned long long* __restrict__ touched, int B) {
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int row = blockIdx.x * (blockDim.x / LCTR_WAVE) + (threadIdx.x >> 6);
  if (row >= B) return;
  const int g = lane / K;
  const int k = lane % K;
  const float d = dpred[row];
  const float sv = sumVX[(size_t)row * K + k];
  const int beg = row_ptr[row], end = row_ptr[row + 1];
  for (int j = beg + g; j < end; j += G) {
    const int fid = fids[j];
    const float x = vals[j];
    const float v = V[(size_t)fid * K + k];
    atomicAdd(&gradV[(size_t)fid * K + k], d * (sv - v * x) * x);
    if (k == 0) {
      atomicAdd(&gradW[fid], d * x);
      atomicOr(&touched[fid >> 6], 1ull << (fid & 63));
    }
  }
}

// ---------------------------------------------------------------------------
// Sorted backward, phase 1 (emit): write per-entry gradient contributions
// coalesced, no atomics:
//   gw[j]   = d * x_j
//   gv[j,k] = d * (sumVX[k] - V[fid_j,k]*x_j) * x_j
// The batch's fids are then radix-sorted (rocPRIM bit-range sort,
// sort_kernels.hip) and phase 2 (fm_sorted_apply_kernel) segment-reduces
// them into the dense grad slabs
// with at most a handful of atomics per unique feature — this removes the
// hot-feature atomic serialization that dominates the naive scatter backward
// (measured 2.76 ms/step vs ~0.1 ms total for everything else; see
// profiles/r01_fm_atomic_backward.txt).
// ---------------------------------------------------------------------------
// `pos` (optional): per-entry write slot. When given, entry j's gradient
// lands at gv[pos[j]] / gw[pos[j]] — i.e. directly in SORTED order (pos =
// inverse of the sort permutation). That moves the randomness of the
// sorted pipeline from the apply kernel's dependent 64 B GATHERS (latency
// bound, measured 285 us/step) onto this kernel's independent STORES
// (fire-and-forget through L2), and lets the apply read gv sequentially.
template <int K>
__global__ void fm_backward_emit_kernel(
    const int* __restrict__ row_ptr, const int* __restrict__ fids,
    const float* __restrict__ vals, const float* __restrict__ V,
    const float* __restrict__ sumVX, const float* __restrict__ dpred,
    float* __restrict__ gw, float* __restrict__ gv, int B,
    const int* __restrict__ pos) {
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int row = blockIdx.x * (blockDim.x / LCTR_WAVE) + (threadIdx.x >> 6);
  if (row >= B) return;
  const int g = lane / K;
  const int k = lane % K;
  const float d = dpred[row];
  const float sv = sumVX[(size_t)row * K + k];
  const int beg = row_ptr[row], end = row_ptr[row + 1];
  // 4-deep manual pipeline: the V row gathers are the latency bound
  // (119 us vs a ~42 us traffic floor); issuing 4 independent gathers
  // per lane before consuming them quadruples the bytes in flight
  int j = beg + g;
  for (; j + 3 * G < end; j += 4 * G) {
    int f[4], sl[4];
    float x[4], v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int jj = j + u * G;
      f[u] = fids[jj];
      x[u] = vals[jj];
      sl[u] = pos ? pos[jj] : jj;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = V[(size_t)f[u] * K + k];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      gv[(size_t)sl[u] * K + k] = d * (sv - v[u] * x[u]) * x[u];
      if (k == 0) gw[sl[u]] = d * x[u];
    }
  }
  for (; j < end; j += G) {
    const int fid = fids[j];
    const float x = vals[j];
    const int slot = pos ? pos[j] : j;
    gv[(size_t)slot * K + k] = d * (sv - V[(size_t)fid * K + k] * x) * x;
    if (k == 0) gw[slot] = d * x;
  }
}

// inv[perm[i]] = i : build the emit kernel's write-slot array from the
// sort permutation (sequential reads of perm, scattered int32 stores).
__global__ void inv_perm_kernel(const int* __restrict__ perm,
                                int* __restrict__ inv, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) inv[perm[i]] = i;
}

// Sorted backward, phase 2: segment-reduce sorted per-entry grads into the
// dense slabs. Each 64-lane wave owns a contiguous chunk of sorted entries;
// K-lane subgroups walk their stride, accumulating runs of equal fid in
// registers and flushing with one atomicAdd per run. Segment heads also set
// the touched bitmap (one atomicOr per unique fid).
// opt_mode: 0 = slab-only (accumulate into gradW/gradV + touched bitmap);
//           1 = fused Adagrad, 2 = fused FTRL. In fused modes, any feature
//           whose sorted segment lies ENTIRELY within one subgroup's range
//           (checked via the global neighbors sorted_fids[first-1] /
//           sorted_fids[last+1]) holds its TOTAL batch gradient at flush
//           time, so the optimizer update is applied in place with no
//           atomics and the slab/bitmap/compaction/apply pass only handles
//           the ~2 boundary-spanning features per subgroup.
// WPE: min waves/SIMD handed to the allocator (HIP __launch_bounds__
// 2nd arg). The K=16 walk allocates 86 VGPR — one register over the
// 6-wave boundary (512/6 = 85.3); WPE=6 caps it at 85 for +20%
// occupancy on this latency-bound kernel (LCTR_FM_APPLY_WPE=6 A/B).
template <int K, bool PP = true, int WPE = 1>
__global__ __launch_bounds__(256, WPE) void fm_sorted_apply_kernel(
    const int* __restrict__ sorted_fids, const int* __restrict__ perm,
    const float* __restrict__ gw, const float* __restrict__ gv,
    float* __restrict__ gradW, float* __restrict__ gradV,
    unsigned long long* __restrict__ touched, int nnz, int chunk,
    int opt_mode, float* __restrict__ V, FmOptArgs oa) {
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int wave = blockIdx.x * (blockDim.x / LCTR_WAVE) + (threadIdx.x >> 6);
  const int g = lane / K;
  const int k = lane % K;
  const int base = wave * chunk;
  if (base >= nnz) return;
  const int end = min(base + chunk, nnz);
  // each K-lane subgroup owns a CONTIGUOUS sub-chunk (runs stay contiguous
  // -> one flush per run) and walks it 4 entries at a time with the gathers
  // issued up-front (4 independent 64B loads in flight per subgroup: the
  // random gv gather is latency-bound, unrolling feeds the memory system)
  const int sub = (chunk + G - 1) / G;
  const int sb = min(base + g * sub, end);
  const int se = min(sb + sub, end);

  int cur_fid = -1;
  bool head_ok = false;  // this subgroup saw the segment's global start
  float acc = 0.f, accw = 0.f;

  auto flush = [&](int tail_e) {
    if (cur_fid < 0) return;
    // tail_e = index of the first entry AFTER the run
    const bool tail_ok =
        (tail_e >= nnz) || (sorted_fids[tail_e] != cur_fid);
    if (opt_mode != 0 && head_ok && tail_ok) {
      // exclusive owner of this feature's total gradient: fused update
      const size_t off = (size_t)cur_fid * K + k;
      float v = V[off], n = oa.nV[off];
      float z = opt_mode == 2 ? oa.zV[off] : 0.f;
      fm_opt_step_v(opt_mode, v, n, z, acc, oa);
      if (opt_mode == 2) oa.zV[off] = z;
      oa.nV[off] = n;
      V[off] = v;
      if (k == 0) {
        float w = oa.W[cur_fid], nw = oa.nW[cur_fid];
        float zw = opt_mode != 1 ? oa.zW[cur_fid] : 0.f;
        fm_opt_step_w(opt_mode, w, nw, zw, accw, oa);
        if (opt_mode != 1) oa.zW[cur_fid] = zw;
        oa.nW[cur_fid] = nw;
        oa.W[cur_fid] = w;
      }
    } else if (head_ok && tail_ok) {
      // exclusive owner of the whole segment: the slabs are zero for every
      // untouched fid (the optimizer pass zeroes what it consumes), so a
      // plain coalesced store replaces 17 atomics. Measured: the flush
      // atomics, not the gv reads, bound this kernel (tools/bench_apply.py).
      gradV[(size_t)cur_fid * K + k] = acc;
      if (k == 0) {
        gradW[cur_fid] = accw;
        atomicOr(&touched[cur_fid >> 6], 1ull << (cur_fid & 63));
      }
    } else {
      atomicAdd(&gradV[(size_t)cur_fid * K + k], acc);
      if (k == 0) {
        atomicAdd(&gradW[cur_fid], accw);
        atomicOr(&touched[cur_fid >> 6], 1ull << (cur_fid & 63));
      }
    }
  };

  // 2-deep batch pipeline — MEASURED NEGATIVE within-probe (210 vs
  // 220 us at chunk 384): despite the PMC profile (VALUBusy 9.6%,
  // MemUnitStalled 0.6% — latency idling), prefetching the next 8-entry
  // batch costs more in register pressure / issue placement than the
  // extra lines in flight buy at ~6.5 waves/SIMD. Kept selectable
  // (chunk=-4) as the documented experiment; the single-buffer walk
  // stays default. Named ping-pong buffers (NOT runtime-indexed arrays
  // — those allocate in scratch, guide common-mistake 20).
  float vA[8], vwA[8], vB[8], vwB[8];
  int fA[8], fB[8];
#define FM_WALK_LOAD(e0, VV, VW, FF)                                       \
  do {                                                                     \
    const int nv_ = min(8, se - (e0));                                     \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) {                        \
      if (u < nv_) {                                                       \
        FF[u] = sorted_fids[(e0) + u];                                     \
        const long p_ = perm ? (long)perm[(e0) + u] : (long)((e0) + u);    \
        VV[u] = gv[(size_t)p_ * K + k];                                    \
        VW[u] = (k == 0) ? gw[p_] : 0.f;                                   \
      }                                                                    \
    }                                                                      \
  } while (0)
#define FM_WALK_PROC(e0, VV, VW, FF)                                       \
  do {                                                                     \
    const int nv_ = min(8, se - (e0));                                     \
    _Pragma("unroll") for (int u = 0; u < 8; ++u) {                        \
      if (u >= nv_) break;                                                 \
      if (FF[u] != cur_fid) {                                              \
        flush((e0) + u);                                                   \
        cur_fid = FF[u];                                                   \
        acc = 0.f;                                                         \
        accw = 0.f;                                                        \
        head_ok = ((e0) + u == 0 || sorted_fids[(e0) + u - 1] != FF[u]);   \
      }                                                                    \
      acc += VV[u];                                                        \
      accw += VW[u];                                                       \
    }                                                                      \
  } while (0)
  if (PP) {
    if (sb < se) FM_WALK_LOAD(sb, vA, vwA, fA);
    for (int e = sb; e < se; e += 16) {
      if (e + 8 < se) FM_WALK_LOAD(e + 8, vB, vwB, fB);
      FM_WALK_PROC(e, vA, vwA, fA);
      if (e + 8 >= se) break;
      if (e + 16 < se) FM_WALK_LOAD(e + 16, vA, vwA, fA);
      FM_WALK_PROC(e + 8, vB, vwB, fB);
    }
  } else {  // round-1 single-buffer walk (within-probe A/B baseline)
    for (int e = sb; e < se; e += 8) {
      FM_WALK_LOAD(e, vA, vwA, fA);
      FM_WALK_PROC(e, vA, vwA, fA);
    }
  }
#undef FM_WALK_LOAD
#undef FM_WALK_PROC
  flush(se);
}

// ---------------------------------------------------------------------------
// Sorted backward, phase 2, segmented-scan variant (K <= 16): one LANE per
// sorted entry, the entry's whole [K] gradient row + gw held in registers.
// A wave covers 64 consecutive sorted entries; run sums are produced by a
// 6-step intra-wave SEGMENTED inclusive scan (shfl_up with head-flag
// propagation) instead of the walk kernel's serial per-subgroup loop —
// the measured bound of the walk was exactly that serial run-detection
// chain + flush divergence (tools/bench_apply.py), not the gv gathers.
// Segment tails write their run's total: a plain 64 B row store when the
// segment's head is in-wave (exclusive owner — slabs are zeroed by the
// optimizer pass), atomicAdd only for the <=2 wave-spanning segments.
// ---------------------------------------------------------------------------
template <int K>
__global__ void fm_segscan_apply_kernel(
    const int* __restrict__ sorted_fids, const int* __restrict__ perm,
    const float* __restrict__ gw, const float* __restrict__ gv,
    float* __restrict__ gradW, float* __restrict__ gradV,
    unsigned long long* __restrict__ touched, int nnz) {
  static_assert(K <= 16, "register-vector variant holds the row per lane");
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long base = (long)wave * LCTR_WAVE;
  if (base >= nnz) return;
  const long e = base + lane;
  const bool valid = e < nnz;

  const int fid = valid ? sorted_fids[e] : -1;
  // original head flag: first entry of a run (lane 0 checks its global
  // predecessor — one extra cached read per wave)
  bool head0 = false;
  if (valid) head0 = (e == 0) || (sorted_fids[e - 1] != fid);

  float v[K + 1];  // [0..K) = gv row, [K] = gw
  if (valid) {
    const long p = perm ? (long)perm[e] : e;
    const float4* src = (const float4*)&gv[(size_t)p * K];
#pragma unroll
    for (int q = 0; q < K / 4; ++q) {
      const float4 t = src[q];
      v[q * 4 + 0] = t.x;
      v[q * 4 + 1] = t.y;
      v[q * 4 + 2] = t.z;
      v[q * 4 + 3] = t.w;
    }
    v[K] = gw[p];
  } else {
#pragma unroll
    for (int i = 0; i <= K; ++i) v[i] = 0.f;
  }

  // segmented inclusive scan: f = "a head lies within my covered window";
  // add the incoming prefix only while my window is still head-free.
  unsigned f = head0 ? 1u : 0u;
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) {
    const unsigned tf = __shfl_up(f, s);
    const bool take = (lane >= s) && (f == 0u);
    float tv[K + 1];
#pragma unroll
    for (int i = 0; i <= K; ++i) tv[i] = __shfl_up(v[i], s);
    if (take) {
#pragma unroll
      for (int i = 0; i <= K; ++i) v[i] += tv[i];
    }
    if (lane >= s) f |= tf;
  }

  // tail = last entry of a run: the next entry starts a new run (its
  // original head flag), or the stream ends here.
  const bool nh = __shfl_down((int)head0, 1);
  bool tail = false;
  if (valid) {
    if (e + 1 >= nnz) {
      tail = true;
    } else if (lane == LCTR_WAVE - 1) {
      tail = sorted_fids[e + 1] != fid;
    } else {
      tail = nh;
    }
  }

  if (tail) {
    if (f) {
      // head in-wave -> this lane holds the run's TOTAL and owns it
      float4* dst = (float4*)&gradV[(size_t)fid * K];
#pragma unroll
      for (int q = 0; q < K / 4; ++q) {
        float4 t;
        t.x = v[q * 4 + 0];
        t.y = v[q * 4 + 1];
        t.z = v[q * 4 + 2];
        t.w = v[q * 4 + 3];
        dst[q] = t;
      }
      gradW[fid] = v[K];
    } else {
#pragma unroll
      for (int i = 0; i < K; ++i)
        atomicAdd(&gradV[(size_t)fid * K + i], v[i]);
      atomicAdd(&gradW[fid], v[K]);
    }
    atomicOr(&touched[fid >> 6], 1ull << (fid & 63));
  } else if (valid && lane == LCTR_WAVE - 1) {
    // run continues into the next wave: flush this wave's partial sum
#pragma unroll
    for (int i = 0; i < K; ++i)
      atomicAdd(&gradV[(size_t)fid * K + i], v[i]);
    atomicAdd(&gradW[fid], v[K]);
    atomicOr(&touched[fid >> 6], 1ull << (fid & 63));
  }
}

// ---------------------------------------------------------------------------
// Sorted backward, phase 2, QUAD-PER-ENTRY segmented scan (round 2,
// docs/STATUS.md lever 3): K/4 lanes per entry, each holding one float4
// quad of the gv row (+ gw on the first lane) — 5 live registers instead
// of the 17 that made the lane-per-entry segscan lose to the walk. The
// wave covers 64/(K/4) consecutive sorted entries; run totals come from
// a log2-step segmented inclusive scan over entry slots (shfl_up at
// entry stride), tails flush with one dwordx4 store per lane (plain for
// in-wave-head runs — slabs zeroed by the optimizer pass — atomics only
// for wave-spanning runs).
// ---------------------------------------------------------------------------
template <int K>
__global__ void fm_segscan4_apply_kernel(
    const int* __restrict__ sorted_fids, const int* __restrict__ perm,
    const float* __restrict__ gw, const float* __restrict__ gv,
    float* __restrict__ gradW, float* __restrict__ gradV,
    unsigned long long* __restrict__ touched, int nnz) {
  static_assert(K % 4 == 0 && K >= 4 && K <= 64, "quad layout needs K%4==0");
  constexpr int L = K / 4;            // lanes per entry
  constexpr int EPW = LCTR_WAVE / L;  // entries per wave
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const long base = (long)wave * EPW;
  if (base >= nnz) return;
  const int ei = lane / L;
  const int q = lane % L;
  const long e = base + ei;
  const bool valid = e < nnz;

  const int fid = valid ? sorted_fids[e] : -1;
  const bool head0 = valid && ((e == 0) || (sorted_fids[e - 1] != fid));

  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float w = 0.f;
  if (valid) {
    const long p = perm ? (long)perm[e] : e;
    v = ((const float4*)&gv[(size_t)p * K])[q];
    if (q == 0) w = gw[p];
  }

  unsigned f = head0 ? 1u : 0u;
#pragma unroll
  for (int s = L; s < LCTR_WAVE; s <<= 1) {
    const unsigned tf = __shfl_up(f, s);
    float4 tv;
    tv.x = __shfl_up(v.x, s);
    tv.y = __shfl_up(v.y, s);
    tv.z = __shfl_up(v.z, s);
    tv.w = __shfl_up(v.w, s);
    const float tw = __shfl_up(w, s);
    if ((lane >= s) && (f == 0u)) {
      v.x += tv.x;
      v.y += tv.y;
      v.z += tv.z;
      v.w += tv.w;
      w += tw;
    }
    if (lane >= s) f |= tf;
  }

  const bool tail = valid && ((e + 1 >= nnz) || (sorted_fids[e + 1] != fid));
  if (tail && f) {
    // run's head is in-wave -> this entry's lanes hold the TOTAL and own
    // the feature exclusively: plain coalesced row store
    ((float4*)&gradV[(size_t)fid * K])[q] = v;
    if (q == 0) {
      gradW[fid] = w;
      atomicOr(&touched[fid >> 6], 1ull << (fid & 63));
    }
  } else if (tail || (valid && ei == EPW - 1)) {
    // spanning run (tail without in-wave head, or wave's last entry with
    // the run continuing): atomic partial flush
    atomicAdd(&gradV[(size_t)fid * K + q * 4 + 0], v.x);
    atomicAdd(&gradV[(size_t)fid * K + q * 4 + 1], v.y);
    atomicAdd(&gradV[(size_t)fid * K + q * 4 + 2], v.z);
    atomicAdd(&gradV[(size_t)fid * K + q * 4 + 3], v.w);
    if (q == 0) {
      atomicAdd(&gradW[fid], w);
      atomicOr(&touched[fid >> 6], 1ull << (fid & 63));
    }
  }
}

// ---------------------------------------------------------------------------
// Segment backward (backward_mode="segment"): per-piece reduce with the
// optimizer fused in. The sorted stream is cut beforehand (sort_kernels.hip,
// segment_worklist_launch) into pieces: a piece starts at every run head and
// at every multiple of CAP, so it lies inside one run and is at most CAP
// long. One K-lane subgroup sums one piece; the loop has no neighbour
// comparison, and the loads of a batch are independent.
//   * WHOLE piece (starts at its run's head, ends at its tail): the subgroup
//     holds the feature's total batch gradient and applies the optimizer in
//     place — no slab, no bitmap, no atomics.
//   * PARTIAL piece (its run crosses a CAP boundary): atomicAdd into the
//     gradW/gradV slabs; the piece holding the run's head appends the fid to
//     the spill list (one counter atomic per wave), which the sparse apply
//     kernels below consume, re-zeroing the slab entries they read.
// At most ceil(nnz/CAP)-1 runs cross a boundary, which bounds the list.
// The grid is fixed; waves stride over the device-side piece count. Per
// piece the dependent loads are piece_start -> (fid, handle) -> (entry data,
// V, nV, neighbours): the first two levels are fetched one and two
// iterations ahead, so an iteration waits for one round trip, not three.
//
// Where an entry's gradient comes from is a policy (Src), so the piece loop,
// the whole/partial logic, the spill append and the optimizer calls exist
// once. A policy has
//   Handle             what is read sequentially at sorted position e, one
//                      batch ahead (handle(e)); Handle{} stands for no entry
//   Data load<K>(h,k)  the entry's random gather(s), issued per batch
//   add(h,t,v,acc,accw) the entry's contribution, v = the piece's V[fid,k]
//                      from before the update; Handle{} with Data{} adds 0
// ---------------------------------------------------------------------------
// Gathered: the gradients were emitted per entry (fm_backward_emit_kernel)
// in CSR order; handle = perm[e], the entry's slot in gv / gw.
struct FmSrcGathered {
  const int* __restrict__ perm;
  const float* __restrict__ gw;
  const float* __restrict__ gv;
  using Handle = int;
  struct Data {
    float gv, gw;
  };
  __device__ __forceinline__ Handle handle(int e) const {
    return perm ? perm[e] : e;
  }
  template <int K>
  __device__ __forceinline__ Data load(Handle h, int k) const {
    return {gv[(size_t)h * K + k], (k == 0) ? gw[h] : 0.f};
  }
  __device__ __forceinline__ void add(Handle, Data t, float, float& acc,
                                      float& accw) const {
    acc += t.gv;
    accw += t.gw;
  }
};

// Recompute: the sort carried the forward's records {row, bits of x} as its
// payload, so position e holds the entry's row and value directly (no perm,
// no per-entry gradient buffer). The gathers go to sumVX (B*K floats, a few
// MB) and dpred; the contribution is formed with the expressions of
// fm_backward_emit_kernel, per entry (not factorised over the piece), from
// the V row the piece loads for the optimizer anyway.
struct FmSrcRecompute {
  const int2* __restrict__ rec;
  const float* __restrict__ sumVX;
  const float* __restrict__ dpred;
  int B;
  using Handle = int2;
  struct Data {
    float sv, d;
  };
  __device__ __forceinline__ Handle handle(int e) const { return rec[e]; }
  template <int K>
  __device__ __forceinline__ Data load(Handle h, int k) const {
    // rows come from the forward kernel; the clamp only keeps a foreign
    // record buffer from reading outside sumVX / dpred
    const int row = min(max(h.x, 0), B - 1);
    return {sumVX[(size_t)row * K + k], dpred[row]};
  }
  __device__ __forceinline__ void add(Handle h, Data t, float v, float& acc,
                                      float& accw) const {
    const float x = __int_as_float(h.y);
    acc += t.d * (t.sv - v * x) * x;
    accw += t.d * x;
  }
};

// D: entries per batch of the inner loop (independent gathers in flight per
// lane). More lookahead costs registers, i.e. resident waves.
template <int K, class Src, int D>
__global__ __launch_bounds__(256) void fm_segment_apply_kernel(
    const int* __restrict__ sorted_fids, Src src,
    const int* __restrict__ piece_start, const int* __restrict__ n_pieces,
    float* __restrict__ gradW, float* __restrict__ gradV,
    int* __restrict__ spill, int* __restrict__ spill_count, int spill_cap,
    int nnz, int opt_mode, float* __restrict__ V, FmOptArgs oa) {
  using Handle = typename Src::Handle;
  using Data = typename Src::Data;
  constexpr int G = LCTR_WAVE / K;
  const int lane = threadIdx.x & (LCTR_WAVE - 1);
  const int g = lane / K;
  const int k = lane % K;
  const long P = min(*n_pieces, nnz);
  const long stride = (long)gridDim.x * (blockDim.x / LCTR_WAVE) * G;
  long base =
      ((long)blockIdx.x * (blockDim.x / LCTR_WAVE) + (threadIdx.x >> 6)) * G;

  // [s, e) of this subgroup's piece in the wave's group at `b`; a subgroup
  // past the last piece gets the empty piece s = e = nnz
  auto load_piece = [&](long b, int& s, int& e) {
    const long p = b + g;
    s = nnz;
    e = nnz;
    if (p < P) {
      s = min(max(piece_start[p], 0), nnz);
      if (p + 1 < P) e = min(max(piece_start[p + 1], s), nnz);
    }
  };
  auto load_head = [&](int s, int& fid, Handle& h) {
    fid = -1;
    h = Handle{};
    if (s < nnz) {
      fid = sorted_fids[s];
      h = src.handle(s);
    }
  };

  int s0, e0, s1, e1, fid0;
  Handle h0;
  load_piece(base, s0, e0);
  load_piece(base + stride, s1, e1);
  load_head(s0, fid0, h0);

  // wave-uniform loop: every lane stays in it until the wave's last group,
  // so the ballot below sees the whole wave
  for (; base < P; base += stride) {
    int s2, e2, fid1;
    Handle h1;
    load_piece(base + 2 * stride, s2, e2);
    load_head(s1, fid1, h1);

    bool spill_me = false;
    if (s0 < nnz) {
      const int fid = fid0;
      const size_t off = (size_t)fid * K + k;
      // everything the piece needs besides its own entries depends on fid
      // alone: issue it with the first entry's data
      const Data t0 = src.template load<K>(h0, k);
      const bool head = (s0 == 0) || (sorted_fids[s0 - 1] != fid);
      const bool tail = (e0 >= nnz) || (sorted_fids[e0] != fid);
      float v = V[off], n = oa.nV[off];
      float z = (opt_mode == 2) ? oa.zV[off] : 0.f;
      float w = 0.f, nw = 0.f, zw = 0.f;
      if (k == 0) {
        w = oa.W[fid];
        nw = oa.nW[fid];
        if (opt_mode != 1) zw = oa.zW[fid];
      }
      // rest of the piece, D independent gathers per batch; the batch's
      // handles are fetched one batch ahead, so a batch costs one round
      // trip, not handle -> data
      Handle hn[D];
#pragma unroll
      for (int u = 0; u < D; ++u) {
        const int ee = s0 + 1 + u;
        hn[u] = (ee < e0) ? src.handle(ee) : Handle{};
      }
      float acc = 0.f, accw = 0.f;
      for (int e = s0 + 1; e < e0; e += D) {
        Handle hc[D];
        Data t[D];
#pragma unroll
        for (int u = 0; u < D; ++u) {
          hc[u] = hn[u];
          t[u] = Data{};
          if (e + u < e0) t[u] = src.template load<K>(hc[u], k);
        }
#pragma unroll
        for (int u = 0; u < D; ++u) {
          const int ee = e + D + u;
          hn[u] = (ee < e0) ? src.handle(ee) : Handle{};
        }
#pragma unroll
        for (int u = 0; u < D; ++u) src.add(hc[u], t[u], v, acc, accw);
      }
      // the head entry last: its add is the first use of v, so the first
      // batch's gathers are issued without waiting for the V row
      src.add(h0, t0, v, acc, accw);
      if (head && tail) {
        fm_opt_step_v(opt_mode, v, n, z, acc, oa);
        if (opt_mode == 2) oa.zV[off] = z;
        oa.nV[off] = n;
        V[off] = v;
        if (k == 0) {
          fm_opt_step_w(opt_mode, w, nw, zw, accw, oa);
          if (opt_mode != 1) oa.zW[fid] = zw;
          oa.nW[fid] = nw;
          oa.W[fid] = w;
        }
      } else {
        atomicAdd(&gradV[off], acc);
        if (k == 0) atomicAdd(&gradW[fid], accw);
        spill_me = head && (k == 0);
      }
    }
    // wave-aggregated append of the runs that spilled to the slabs
    const unsigned long long m = __ballot(spill_me);
    if (m) {
      int slot = 0;
      if (lane == 0) slot = atomicAdd(spill_count, __popcll(m));
      slot = __shfl(slot, 0) + __popcll(m & ((1ull << lane) - 1ull));
      if (spill_me && slot < spill_cap) spill[slot] = fid0;  // clamp
    }

    s0 = s1;
    e0 = e1;
    fid0 = fid1;
    h0 = h1;
    s1 = s2;
    e1 = e2;
  }
}

// ---------------------------------------------------------------------------
// Tile-local segment reduce (backward_mode="segment"): the reduce above
// without its global work list. A block owns TILE consecutive sorted entries.
// TILE is a multiple of CAP and pieces start at run heads and multiples of
// CAP, so a tile holds whole pieces only and the block finds them itself:
//   1. stage the tile's fids (plus the two neighbour fids, for the run
//      head / tail tests) and records into LDS with coalesced loads;
//   2. flag the unit starts and compact them with a block scan. A unit is a
//      piece cut once more at the multiples of SPLIT of the sorted position
//      (CUT = min(CAP, SPLIT)), so it is at most SPLIT long; a list entry
//      also says whether its unit starts a piece;
//   3. every K-lane subgroup takes NF units per turn and issues all their
//      row loads (V, and for a one-unit piece nV/W/nW/zW, plus the first
//      entry's sumVX/dpred) together: the fids and records come from LDS, so
//      the only dependent global level left is the gathers themselves.
//      A one-unit piece is finished on the spot as in the kernel above
//      (whole: optimizer in place; partial: slabs + spill list), with the
//      same per-entry expressions in the same order. A unit of a longer
//      piece leaves its partial (acc[k], accw) in its own LDS slot, so the
//      units of a long piece are spread over the block's subgroups;
//   4. after a block barrier one subgroup per multi-unit piece adds the
//      piece's partials in ascending position order (no float atomics in
//      LDS: a whole piece's sum does not depend on scheduling) and finishes
//      the piece the same way.
// No parameter store of a fid precedes a read of its old V: one-unit whole
// pieces own their fid alone, multi-unit pieces store only after the
// barrier, partial pieces never store (the spill apply, launched next, does).
// Slots: a unit of a multi-unit piece either starts on a multiple of CUT
// (slot 2c for cell c) or is its piece's first unit and reaches the end of
// its cell (slot 2c + 1, at most one per cell): 2 * TILE / SPLIT slots.
// ---------------------------------------------------------------------------
constexpr int kFmTilePieceBit = 1 << 30;  // list entry: unit starts a piece

template <int K, int TILE, int SPLIT, int NF>
__global__ __launch_bounds__(256) void fm_segment_tile_kernel(
    const int* __restrict__ sorted_fids, const int2* __restrict__ rec,
    const float* __restrict__ sumVX, const float* __restrict__ dpred, int B,
    int cap, float* __restrict__ gradW, float* __restrict__ gradV,
    int* __restrict__ spill, int* __restrict__ spill_count, int spill_cap,
    int nnz, int opt_mode, float* __restrict__ V, FmOptArgs oa) {
  constexpr int NT = 256;
  constexpr int NW = NT / LCTR_WAVE;
  constexpr int ITEMS = TILE / NT;
  constexpr int NSG = NT / K;  // subgroups per block
  constexpr int D = 4;         // gathers in flight per lane inside a unit
  constexpr int NSLOT = 2 * TILE / SPLIT;
  static_assert(TILE % NT == 0 && TILE % SPLIT == 0, "tile shape");

  __shared__ int s_fid[TILE + 2];  // [0] = fid before the tile, [n+1] after
  __shared__ int2 s_rec[TILE];
  __shared__ int s_unit[TILE + 1];
  __shared__ int s_multi[TILE / SPLIT];
  __shared__ float s_part[NSLOT * (K + 1)];
  __shared__ int s_wave_tot[NW];
  __shared__ int s_nmulti;

  const int tid = threadIdx.x;
  const int lane = tid & (LCTR_WAVE - 1);
  const int wv = tid >> 6;
  const int sg = tid / K;
  const int k = tid % K;
  const long t0 = (long)blockIdx.x * TILE;
  const int n = (int)min((long)TILE, (long)nnz - t0);
  if (n <= 0) return;
  const int cut = min(cap, SPLIT);

  // -- 1. stage ------------------------------------------------------------
#pragma unroll
  for (int u = 0; u < ITEMS; ++u) {
    const int i = u * NT + tid;
    if (i < n) {
      s_fid[i + 1] = sorted_fids[t0 + i];
      s_rec[i] = rec[t0 + i];
    }
  }
  if (tid == 0) {
    s_fid[0] = (t0 > 0) ? sorted_fids[t0 - 1] : 0;
    s_fid[n + 1] = (t0 + n < nnz) ? sorted_fids[t0 + n] : 0;
    s_nmulti = 0;
  }
  __syncthreads();
  // run head at local i / run tail before local i (neighbours guarded)
  auto is_head = [&](int i) {
    return (t0 + i == 0) || (s_fid[i] != s_fid[i + 1]);
  };
  auto is_tail_before = [&](int i, int fid) {
    return (t0 + i >= nnz) || (s_fid[i + 1] != fid);
  };

  // -- 2. local unit list --------------------------------------------------
  int mine[ITEMS];
  int cnt = 0;
#pragma unroll
  for (int u = 0; u < ITEMS; ++u) {
    const int i = tid * ITEMS + u;
    mine[u] = -1;
    if (i < n) {
      const long gi = t0 + i;
      const bool head = is_head(i);
      if (head || (gi & (cut - 1)) == 0) {
        const bool pstart = head || (gi & (cap - 1)) == 0;
        mine[u] = i | (pstart ? kFmTilePieceBit : 0);
        ++cnt;
      }
    }
  }
  int scan = cnt;
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) {
    const int t = __shfl_up(scan, s);
    if (lane >= s) scan += t;
  }
  if (lane == LCTR_WAVE - 1) s_wave_tot[wv] = scan;
  __syncthreads();
  int pos = scan - cnt, nu = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    const int t = s_wave_tot[w];
    if (w < wv) pos += t;
    nu += t;
  }
#pragma unroll
  for (int u = 0; u < ITEMS; ++u)
    if (mine[u] >= 0) s_unit[pos++] = mine[u];
  if (tid == 0) s_unit[nu] = n | kFmTilePieceBit;  // end of the last unit
  __syncthreads();

  // what a finished piece does with its sum: `whole` applies the optimizer
  // to the rows loaded before the sum, otherwise the sum goes to the slabs
  // and the run's head piece reports the fid
  auto append_spill = [&](bool spill_me, int fid) {
    const unsigned long long m = __ballot(spill_me);
    if (m) {
      int slot = 0;
      if (lane == 0) slot = atomicAdd(spill_count, __popcll(m));
      slot = __shfl(slot, 0) + __popcll(m & ((1ull << lane) - 1ull));
      if (spill_me && slot < spill_cap) spill[slot] = fid;  // clamp
    }
  };
  auto gather = [&](int i, float& sv, float& d) {
    // rows come from the forward kernel; the clamp only keeps a foreign
    // record buffer from reading outside sumVX / dpred
    const int row = min(max(s_rec[i].x, 0), B - 1);
    sv = sumVX[(size_t)row * K + k];
    d = dpred[row];
  };
  auto add = [&](int i, float sv, float d, float v, float& acc,
                 float& accw) {
    const float x = __int_as_float(s_rec[i].y);
    acc += d * (sv - v * x) * x;
    accw += d * x;
  };

  // -- 3. units ------------------------------------------------------------
  for (int j0 = 0; j0 < nu; j0 += NSG * NF) {
    int us[NF], ue[NF], fid[NF];
    bool single[NF], first[NF], whole[NF], headp[NF];
    float v[NF], nv[NF], z[NF], w[NF], nw[NF], zw[NF], sv0[NF], d0[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const int j = j0 + f * NSG + sg;
      us[f] = ue[f] = 0;
      fid[f] = 0;
      single[f] = first[f] = whole[f] = headp[f] = false;
      v[f] = nv[f] = z[f] = w[f] = nw[f] = zw[f] = sv0[f] = d0[f] = 0.f;
      if (j < nu) {
        const int a = s_unit[j], b = s_unit[j + 1];
        us[f] = a & (kFmTilePieceBit - 1);
        ue[f] = b & (kFmTilePieceBit - 1);
        first[f] = (a & kFmTilePieceBit) != 0;
        single[f] = first[f] && (b & kFmTilePieceBit) != 0;
        fid[f] = s_fid[us[f] + 1];
        const size_t off = (size_t)fid[f] * K + k;
        v[f] = V[off];
        gather(us[f], sv0[f], d0[f]);
        if (single[f]) {
          headp[f] = is_head(us[f]);
          whole[f] = headp[f] && is_tail_before(ue[f], fid[f]);
        }
        if (whole[f]) {
          nv[f] = oa.nV[off];
          if (opt_mode == 2) z[f] = oa.zV[off];
          if (k == 0) {
            w[f] = oa.W[fid[f]];
            nw[f] = oa.nW[fid[f]];
            if (opt_mode != 1) zw[f] = oa.zW[fid[f]];
          }
        }
      }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      bool spill_me = false;
      if (ue[f] > us[f]) {
        float acc = 0.f, accw = 0.f;
        for (int e = us[f] + 1; e < ue[f]; e += D) {
          float sv[D], d[D];
#pragma unroll
          for (int u = 0; u < D; ++u) {
            sv[u] = d[u] = 0.f;
            if (e + u < ue[f]) gather(e + u, sv[u], d[u]);
          }
#pragma unroll
          for (int u = 0; u < D; ++u)
            if (e + u < ue[f]) add(e + u, sv[u], d[u], v[f], acc, accw);
        }
        // the head entry last, as in fm_segment_apply_kernel
        add(us[f], sv0[f], d0[f], v[f], acc, accw);
        const size_t off = (size_t)fid[f] * K + k;
        if (whole[f]) {
          fm_opt_step_v(opt_mode, v[f], nv[f], z[f], acc, oa);
          if (opt_mode == 2) oa.zV[off] = z[f];
          oa.nV[off] = nv[f];
          V[off] = v[f];
          if (k == 0) {
            fm_opt_step_w(opt_mode, w[f], nw[f], zw[f], accw, oa);
            if (opt_mode != 1) oa.zW[fid[f]] = zw[f];
            oa.nW[fid[f]] = nw[f];
            oa.W[fid[f]] = w[f];
          }
        } else if (single[f]) {
          atomicAdd(&gradV[off], acc);
          if (k == 0) atomicAdd(&gradW[fid[f]], accw);
          spill_me = headp[f] && (k == 0);
        } else {
          const int c = us[f] / SPLIT;
          const int slot = 2 * c + ((us[f] & (SPLIT - 1)) ? 1 : 0);
          s_part[slot * (K + 1) + k] = acc;
          if (k == 0) {
            s_part[slot * (K + 1) + K] = accw;
            if (first[f]) s_multi[atomicAdd(&s_nmulti, 1)] = j0 + f * NSG + sg;
          }
        }
      }
      append_spill(spill_me, fid[f]);
    }
  }
  __syncthreads();

  // -- 4. multi-unit pieces ------------------------------------------------
  const int nm = s_nmulti;
  for (int m0 = 0; m0 < nm; m0 += NSG) {
    bool spill_me = false;
    int fidm = 0;
    if (m0 + sg < nm) {
      int j = s_multi[m0 + sg];
      const int ps = s_unit[j] & (kFmTilePieceBit - 1);
      fidm = s_fid[ps + 1];
      const size_t off = (size_t)fidm * K + k;
      // the piece's end: the next list entry that starts a piece
      int j1 = j + 1;
      while (!(s_unit[j1] & kFmTilePieceBit)) ++j1;
      const int pe = s_unit[j1] & (kFmTilePieceBit - 1);
      const bool whole = is_head(ps) && is_tail_before(pe, fidm);
      float v = 0.f, nv = 0.f, z = 0.f, w = 0.f, nw = 0.f, zw = 0.f;
      if (whole) {
        v = V[off];
        nv = oa.nV[off];
        if (opt_mode == 2) z = oa.zV[off];
        if (k == 0) {
          w = oa.W[fidm];
          nw = oa.nW[fidm];
          if (opt_mode != 1) zw = oa.zW[fidm];
        }
      }
      float acc = 0.f, accw = 0.f;
      for (; j < j1; ++j) {
        const int s = s_unit[j] & (kFmTilePieceBit - 1);
        const int slot = 2 * (s / SPLIT) + ((s & (SPLIT - 1)) ? 1 : 0);
        acc += s_part[slot * (K + 1) + k];
        accw += s_part[slot * (K + 1) + K];
      }
      if (whole) {
        fm_opt_step_v(opt_mode, v, nv, z, acc, oa);
        if (opt_mode == 2) oa.zV[off] = z;
        oa.nV[off] = nv;
        V[off] = v;
        if (k == 0) {
          fm_opt_step_w(opt_mode, w, nw, zw, accw, oa);
          if (opt_mode != 1) oa.zW[fidm] = zw;
          oa.nW[fidm] = nw;
          oa.W[fidm] = w;
        }
      } else {
        atomicAdd(&gradV[off], acc);
        if (k == 0) atomicAdd(&gradW[fidm], accw);
        spill_me = is_head(ps) && (k == 0);
      }
    }
    append_spill(spill_me, fidm);
  }
}

// ---------------------------------------------------------------------------
// Bitmap -> unique-fid list compaction. One thread per 64-feature word;
// clears the word as it goes so the bitmap is reusable next step.
// ---------------------------------------------------------------------------
__global__ void bitmap_compact_kernel(unsigned long long* __restrict__ bitmap,
                                      int nwords, int* __restrict__ out_fids,
                                      int* __restrict__ out_count, int cap) {
  // BLOCK-aggregated append (1024 threads = 16 waves): waves prefix-scan
  // locally, wave totals are scanned in LDS, and only thread 0 touches
  // the global counter — one atomic per 65536 features instead of per
  // wave (the single-counter atomics serialized the old kernel: 57 us
  // for a 2 MB pass).
  __shared__ int wave_tot[16];
  __shared__ int block_base;
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  unsigned long long m = (w < nwords) ? bitmap[w] : 0ull;
  if (m) bitmap[w] = 0ull;
  const int n = __popcll(m);
  int scan = n;
#pragma unroll
  for (int s = 1; s < LCTR_WAVE; s <<= 1) {
    const int t = __shfl_up(scan, s);
    if (lane >= s) scan += t;
  }
  if (lane == LCTR_WAVE - 1) wave_tot[wv] = scan;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = wave_tot[i];
      wave_tot[i] = run;
      run += t;
    }
    block_base = run > 0 ? atomicAdd(out_count, run) : 0;
  }
  __syncthreads();
  int off = block_base + wave_tot[wv] + scan - n;
  while (m) {
    const int b = __ffsll((long long)m) - 1;
    m &= m - 1;
    if (off < cap) out_fids[off] = w * 64 + b;  // clamp: never overrun uniq
    ++off;
  }
}

// ---------------------------------------------------------------------------
// Sparse fused optimizers over the unique-fid list. Thread (i,k) owns
// V[fid_i, k]; lane k==0 additionally owns W[fid_i]. Reads the accumulated
// gradient, applies the update + state, and zeroes the gradient slot so the
// slabs stay clean for the next step. Launched over `capacity` (max possible
// uniques) and guarded by *count so no host sync is needed.
// ---------------------------------------------------------------------------
template <int K>
__global__ void fm_adagrad_apply_kernel(
    const int* __restrict__ uniq, const int* __restrict__ count,
    float* __restrict__ W, float* __restrict__ V, float* __restrict__ nW,
    float* __restrict__ nV, float* __restrict__ gradW,
    float* __restrict__ gradV, float lr, float eps, float l2, int capacity) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i = idx / K;
  const int k = (int)(idx % K);
  if (i >= capacity || i >= *count) return;
  const int fid = uniq[i];
  const size_t off = (size_t)fid * K + k;
  adagrad_update(&V[off], &nV[off], gradV[off], lr, eps, l2);
  gradV[off] = 0.f;
  if (k == 0) {
    adagrad_update(&W[fid], &nW[fid], gradW[fid], lr, eps, l2);
    gradW[fid] = 0.f;
  }
}

// v_adagrad: the classic CTR split — FTRL-proximal on the sparse linear
// weights W, Adagrad on the latent factors V (FTRL's L1 shrinkage starves
// the interaction terms; measured 0.66 vs 0.79 held-out AUC uniform-FTRL
// vs mixed on the synthetic Criteo stream).
template <int K>
__global__ void fm_ftrl_apply_kernel(
    const int* __restrict__ uniq, const int* __restrict__ count,
    float* __restrict__ W, float* __restrict__ V, float* __restrict__ zW,
    float* __restrict__ nW, float* __restrict__ zV, float* __restrict__ nV,
    float* __restrict__ gradW, float* __restrict__ gradV, float alpha,
    float beta, float l1, float l2, int capacity, int v_adagrad, float v_lr,
    float v_eps, float v_l2) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i = idx / K;
  const int k = (int)(idx % K);
  if (i >= capacity || i >= *count) return;
  const int fid = uniq[i];
  const size_t off = (size_t)fid * K + k;
  if (v_adagrad) {
    adagrad_update(&V[off], &nV[off], gradV[off], v_lr, v_eps, v_l2);
  } else {
    ftrl_update(&V[off], &zV[off], &nV[off], gradV[off], alpha, beta, l1,
                l2);
  }
  gradV[off] = 0.f;
  if (k == 0) {
    ftrl_update(&W[fid], &zW[fid], &nW[fid], gradW[fid], alpha, beta, l1, l2);
    gradW[fid] = 0.f;
  }
}

// ---------------------------------------------------------------------------
// Host-side launchers (thin; stream comes from the caller / PyTorch).
// ---------------------------------------------------------------------------
static inline int waves_per_block() { return 4; }  // 256 threads

void fm_forward_launch(const int* row_ptr, const int* fids, const float* vals,
                       const float* W, const float* V, float* pred,
                       float* sumVX, int B, int K, hipStream_t stream) {
  if (B <= 0) return;
  const int wpb = waves_per_block();
  dim3 block(wpb * LCTR_WAVE);
  dim3 grid((B + wpb - 1) / wpb);
  DISPATCH_K(K, hipLaunchKernelGGL((fm_forward_kernel<KC>), grid, block, 0,
                                   stream, row_ptr, fids, vals, W, V, pred,
                                   sumVX, B));
}

void fm_forward_train_launch(const int* row_ptr, const int* fids,
                             const float* vals, const float* W, const float* V,
                             const float* label, float scale, float* loss,
                             float* dpred, float* sumVX, int* rec, int B,
                             int K, int* reset, hipStream_t stream) {
  if (B <= 0) return;
  const int wpb = waves_per_block();
  dim3 block(wpb * LCTR_WAVE);
  dim3 grid((B + wpb - 1) / wpb);
  // rec == nullptr: the records are made elsewhere, the row body writes none
  if (rec != nullptr) {
    DISPATCH_K(K, hipLaunchKernelGGL((fm_forward_train_kernel<KC, true>), grid,
                                     block, 0, stream, row_ptr, fids, vals, W,
                                     V, label, scale, loss, dpred, sumVX,
                                     (int2*)rec, B, reset));
  } else {
    DISPATCH_K(K, hipLaunchKernelGGL((fm_forward_train_kernel<KC, false>),
                                     grid, block, 0, stream, row_ptr, fids,
                                     vals, W, V, label, scale, loss, dpred,
                                     sumVX, (int2*)nullptr, B, reset));
  }
}

void fm_records_launch(const int* row_ptr, const float* vals, int* rec, int B,
                       hipStream_t stream) {
  if (B <= 0) return;
  const int wpb = waves_per_block();
  dim3 block(wpb * LCTR_WAVE);
  dim3 grid((B + wpb - 1) / wpb);
  hipLaunchKernelGGL(fm_records_kernel, grid, block, 0, stream, row_ptr, vals,
                     (int2*)rec, B);
}

void logloss_grad_launch(const float* pred, const float* label, float* loss,
                         float* dpred, float scale, int B,
                         hipStream_t stream) {
  if (B <= 0) return;
  dim3 block(256);
  dim3 grid((B + 255) / 256);
  hipLaunchKernelGGL(logloss_grad_kernel, grid, block, 0, stream, pred, label,
                     loss, dpred, scale, B);
}

void fm_backward_launch(const int* row_ptr, const int* fids, const float* vals,
                        const float* V, const float* sumVX, const float* dpred,
                        float* gradW, float* gradV, unsigned long long* touched,
                        int B, int K, hipStream_t stream) {
  if (B <= 0) return;
  const int wpb = waves_per_block();
  dim3 block(wpb * LCTR_WAVE);
  dim3 grid((B + wpb - 1) / wpb);
  DISPATCH_K(K, hipLaunchKernelGGL((fm_backward_kernel<KC>), grid, block, 0,
                                   stream, row_ptr, fids, vals, V, sumVX,
                                   dpred, gradW, gradV, touched, B));
}

void fm_backward_emit_launch(const int* row_ptr, const int* fids,
                             const float* vals, const float* V,
                             const float* sumVX, const float* dpred, float* gw,
                             float* gv, int B, int K, const int* pos,
                             hipStream_t stream) {
  if (B <= 0) return;
  const int wpb = waves_per_block();
  dim3 block(wpb * LCTR_WAVE);
  dim3 grid((B + wpb - 1) / wpb);
  DISPATCH_K(K, hipLaunchKernelGGL((fm_backward_emit_kernel<KC>), grid, block,
                                   0, stream, row_ptr, fids, vals, V, sumVX,
                                   dpred, gw, gv, B, pos));
}

void inv_perm_launch(const int* perm, int* inv, int n, hipStream_t stream) {
  if (n <= 0) return;
  dim3 block(256);
  dim3 grid((n + 255) / 256);
  hipLaunchKernelGGL(inv_perm_kernel, grid, block, 0, stream, perm, inv, n);
}

void fm_sorted_apply_launch(const int* sorted_fids, const int* perm,
                            const float* gw, const float* gv, float* gradW,
                            float* gradV, unsigned long long* touched, int nnz,
                            int K, int opt_mode, float* V, float* W,
                            float* nW, float* zW, float* nV, float* zV,
                            float p0, float p1, float p2, float p3,
                            float q0, float q1, float q2,
                            int chunk, hipStream_t stream) {
  if (nnz <= 0) return;
  // chunk 0 = auto (walk kernel, chunk 384 — measured best), -1 = the
  // lane-per-entry segmented-scan kernel (correct, measured 275 vs 218
  // us: the 6-step 17-register shfl_up chain costs more than the serial
  // walk saves; kept selectable + parity-tested as a documented negative
  // result), -2 = the round-2 quad-per-entry segscan (K/4 lanes per
  // entry, 5 live registers).
  if (chunk == -2 && (K % 4 == 0) && K <= 64 && opt_mode == 0) {
    const int wpb = waves_per_block();
    const int epw = LCTR_WAVE / (K / 4);
    const int nwaves = (nnz + epw - 1) / epw;
    dim3 block(wpb * LCTR_WAVE);
    dim3 grid((nwaves + wpb - 1) / wpb);
    DISPATCH_K(K, hipLaunchKernelGGL((fm_segscan4_apply_kernel<KC>), grid,
                                     block, 0, stream, sorted_fids, perm,
                                     gw, gv, gradW, gradV, touched, nnz));
    return;
  }
  const bool can_scan =
      (K == 4 || K == 8 || K == 16) && opt_mode == 0;
  if (chunk == -1 && can_scan) {
    const int wpb = waves_per_block();
    const int nwaves = (nnz + LCTR_WAVE - 1) / LCTR_WAVE;
    dim3 block(wpb * LCTR_WAVE);
    dim3 grid((nwaves + wpb - 1) / wpb);
    switch (K) {
      case 4:
        hipLaunchKernelGGL((fm_segscan_apply_kernel<4>), grid, block, 0,
                           stream, sorted_fids, perm, gw, gv, gradW, gradV,
                           touched, nnz);
        return;
      case 8:
        hipLaunchKernelGGL((fm_segscan_apply_kernel<8>), grid, block, 0,
                           stream, sorted_fids, perm, gw, gv, gradW, gradV,
                           touched, nnz);
        return;
      default:
        hipLaunchKernelGGL((fm_segscan_apply_kernel<16>), grid, block, 0,
                           stream, sorted_fids, perm, gw, gv, gradW, gradV,
                           touched, nnz);
        return;
    }
  }
  // chunk == -4 selects the 2-deep pipelined walk (measured negative;
  // kept for A/B); default = single-buffer walk
  const bool pp = chunk == -4;
  if (chunk == -3 || chunk == -4) chunk = 0;
  if (chunk <= 0) chunk = 384;  // measured optimum, tools/bench_apply.py
  const int wpb = waves_per_block();
  const int nwaves = (nnz + chunk - 1) / chunk;
  dim3 block(wpb * LCTR_WAVE);
  dim3 grid((nwaves + wpb - 1) / wpb);
  FmOptArgs oa{W, nW, zW, nV, zV, p0, p1, p2, p3, q0, q1, q2};
  if (pp) {
    DISPATCH_K(K, hipLaunchKernelGGL((fm_sorted_apply_kernel<KC, true>),
                                     grid, block, 0, stream, sorted_fids,
                                     perm, gw, gv, gradW, gradV, touched,
                                     nnz, chunk, opt_mode, V, oa));
  } else {
    // default for the flagship K=16: the 6-wave cap trims 86 -> 80
    // VGPR (no spill) and measured 213.4 vs 222.5 us (+4.3%, 8/8
    // alternating passes, profiles/r2_13_fm_wpe.txt). '0' reverts.
    const char* ew = getenv("LCTR_FM_APPLY_WPE");
    if (K == 16 && !(ew && ew[0] == '0')) {
      hipLaunchKernelGGL((fm_sorted_apply_kernel<16, false, 6>), grid,
                         block, 0, stream, sorted_fids, perm, gw, gv,
                         gradW, gradV, touched, nnz, chunk, opt_mode, V,
                         oa);
      return;
    }
    DISPATCH_K(K, hipLaunchKernelGGL((fm_sorted_apply_kernel<KC, false>),
                                     grid, block, 0, stream, sorted_fids,
                                     perm, gw, gv, gradW, gradV, touched,
                                     nnz, chunk, opt_mode, V, oa));
  }
}

// resident 256-thread blocks of the segment kernel per CU (register bound)
template <int K, class Src, int D>
static int fm_segment_blocks_per_cu() {
  static const int nb = [] {
    int n = 0;
    LCTR_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &n, fm_segment_apply_kernel<K, Src, D>,
        waves_per_block() * LCTR_WAVE, 0));
    return std::max(n, 1);
  }();
  return nb;
}

// What both entry sources share besides the policy object
struct FmSegmentArgs {
  const int* sorted_fids;
  const int* piece_start;
  const int* n_pieces;
  float* gradW;
  float* gradV;
  int* spill;
  int* spill_count;
  int spill_cap, nnz, opt_mode;
  float* V;
  FmOptArgs oa;
  int num_cus;
};

template <int K, class Src, int D>
static void fm_segment_launch_one(const FmSegmentArgs& a, const Src& src,
                                  hipStream_t stream) {
  // fixed grid: exactly the blocks the device holds at once (a block more
  // per CU would run as a second round), never more than one subgroup per
  // possible piece
  const int wpb = waves_per_block();
  constexpr int G = LCTR_WAVE / K;
  const int per_cu = fm_segment_blocks_per_cu<K, Src, D>();
  const long need = ((long)a.nnz + (long)wpb * G - 1) / ((long)wpb * G);
  const int blocks = (int)std::max(
      1L, std::min(need, (long)per_cu * std::max(a.num_cus, 1)));
  hipLaunchKernelGGL((fm_segment_apply_kernel<K, Src, D>), dim3(blocks),
                     dim3(wpb * LCTR_WAVE), 0, stream, a.sorted_fids, src,
                     a.piece_start, a.n_pieces, a.gradW, a.gradV, a.spill,
                     a.spill_count, a.spill_cap, a.nnz, a.opt_mode, a.V,
                     a.oa);
}

void fm_segment_apply_launch(const int* sorted_fids, const int* perm,
                             const int* piece_start, const int* n_pieces,
                             const float* gw, const float* gv, float* gradW,
                             float* gradV, int* spill, int* spill_count,
                             int spill_cap, int nnz, int K, int opt_mode,
                             float* V, float* W, float* nW, float* zW,
                             float* nV, float* zV, float p0, float p1,
                             float p2, float p3, float q0, float q1, float q2,
                             int num_cus, hipStream_t stream) {
  if (nnz <= 0) return;
  const FmSegmentArgs a{sorted_fids, piece_start, n_pieces, gradW, gradV,
                        spill, spill_count, spill_cap, nnz, opt_mode, V,
                        FmOptArgs{W, nW, zW, nV, zV, p0, p1, p2, p3, q0, q1,
                                  q2},
                        num_cus};
  const FmSrcGathered src{perm, gw, gv};
  DISPATCH_K(K, (fm_segment_launch_one<KC, FmSrcGathered, 8>(a, src, stream)));
}

// Batch depth of the recompute reduce. Measured at the flagship shape: 4
// (65 VGPR, 7 waves/SIMD) beats 8 (85 VGPR, 5 waves/SIMD) by 3.7 % of the
// step; 8 wins only above CAP 512 (profiles/r4_01_fm_recompute.txt).
constexpr int kFmRecomputeDepth = 4;

void fm_segment_recompute_launch(
    const int* sorted_fids, const int* rec, const float* sumVX,
    const float* dpred, int B, const int* piece_start, const int* n_pieces,
    float* gradW, float* gradV, int* spill, int* spill_count, int spill_cap,
    int nnz, int K, int opt_mode, float* V, float* W, float* nW, float* zW,
    float* nV, float* zV, float p0, float p1, float p2, float p3, float q0,
    float q1, float q2, int num_cus, hipStream_t stream) {
  if (nnz <= 0 || B <= 0) return;
  const FmSegmentArgs a{sorted_fids, piece_start, n_pieces, gradW, gradV,
                        spill, spill_count, spill_cap, nnz, opt_mode, V,
                        FmOptArgs{W, nW, zW, nV, zV, p0, p1, p2, p3, q0, q1,
                                  q2},
                        num_cus};
  const FmSrcRecompute src{(const int2*)rec, sumVX, dpred, B};
  DISPATCH_K(K, (fm_segment_launch_one<KC, FmSrcRecompute, kFmRecomputeDepth>(
                    a, src, stream)));
}

// Shape of the tile reduce: entries per block, longest unit, units a
// subgroup keeps in flight. Swept over {256, 512, 1024} x {16, 32, 64} x
// {1, 2, 4} at the flagship shape (profiles/r5_01_fm_tile.txt): the smallest
// tile wins (more blocks for the dispatcher to balance, 8 blocks per CU),
// SPLIT 16 and 32 tie, and a second unit in flight buys nothing at TILE 256
// (four in flight lose 5 %): occupancy beats lookahead here too.
constexpr int kFmTile = 256;
constexpr int kFmTileSplit = 32;
constexpr int kFmTileFlight = 1;

struct FmTileArgs {
  const int* sorted_fids;
  const int* rec;
  const float* sumVX;
  const float* dpred;
  int B, cap;
  float* gradW;
  float* gradV;
  int* spill;
  int* spill_count;
  int spill_cap, nnz, opt_mode;
  float* V;
  FmOptArgs oa;
};

template <int K, int TILE, int SPLIT, int NF>
static void fm_segment_tile_launch_one(const FmTileArgs& a,
                                       hipStream_t stream) {
  // one block per tile: the count is known here, the dispatcher balances
  const int blocks = (int)(((long)a.nnz + TILE - 1) / TILE);
  hipLaunchKernelGGL((fm_segment_tile_kernel<K, TILE, SPLIT, NF>),
                     dim3(blocks), dim3(256), 0, stream, a.sorted_fids,
                     (const int2*)a.rec, a.sumVX, a.dpred, a.B, a.cap, a.gradW,
                     a.gradV, a.spill, a.spill_count, a.spill_cap, a.nnz,
                     a.opt_mode, a.V, a.oa);
}

int fm_segment_tile() { return kFmTile; }
int fm_segment_split() { return kFmTileSplit; }

void fm_segment_tile_launch(const int* sorted_fids, const int* rec,
                            const float* sumVX, const float* dpred, int B,
                            int cap, float* gradW, float* gradV, int* spill,
                            int* spill_count, int spill_cap, int nnz, int K,
                            int opt_mode, float* V, float* W, float* nW,
                            float* zW, float* nV, float* zV, float p0,
                            float p1, float p2, float p3, float q0, float q1,
                            float q2, hipStream_t stream) {
  if (nnz <= 0 || B <= 0) return;
  const FmTileArgs a{sorted_fids, rec, sumVX, dpred, B, cap, gradW, gradV,
                     spill, spill_count, spill_cap, nnz, opt_mode, V,
                     FmOptArgs{W, nW, zW, nV, zV, p0, p1, p2, p3, q0, q1,
                               q2}};
  DISPATCH_K(K, (fm_segment_tile_launch_one<KC, kFmTile, kFmTileSplit,
                                            kFmTileFlight>(a, stream)));
}

void bitmap_compact_launch(unsigned long long* bitmap, int nwords,
                           int* out_fids, int* out_count, int cap,
                           hipStream_t stream) {
  dim3 block(1024);
  dim3 grid((nwords + 1023) / 1024);
  hipLaunchKernelGGL(bitmap_compact_kernel, grid, block, 0, stream, bitmap,
                     nwords, out_fids, out_count, cap);
}

void fm_adagrad_apply_launch(const int* uniq, const int* count, float* W,
                             float* V, float* nW, float* nV, float* gradW,
                             float* gradV, float lr, float eps, float l2,
                             int capacity, int K, hipStream_t stream) {
  const long long total = (long long)capacity * K;
  dim3 block(256);
  dim3 grid((unsigned)((total + 255) / 256));
  DISPATCH_K(K, hipLaunchKernelGGL((fm_adagrad_apply_kernel<KC>), grid, block,
                                   0, stream, uniq, count, W, V, nW, nV, gradW,
                                   gradV, lr, eps, l2, capacity));
}

void fm_ftrl_apply_launch(const int* uniq, const int* count, float* W,
                          float* V, float* zW, float* nW, float* zV, float* nV,
                          float* gradW, float* gradV, float alpha, float beta,
                          float l1, float l2, int capacity, int K,
                          int v_adagrad, float v_lr, float v_eps, float v_l2,
                          hipStream_t stream) {
  const long long total = (long long)capacity * K;
  dim3 block(256);
  dim3 grid((unsigned)((total + 255) / 256));
  DISPATCH_K(K, hipLaunchKernelGGL((fm_ftrl_apply_kernel<KC>), grid, block, 0,
                                   stream, uniq, count, W, V, zW, nW, zV, nV,
                                   gradW, gradV, alpha, beta, l1, l2,
                                   capacity, v_adagrad, v_lr, v_eps, v_l2));
}

}  // namespace lightctr
