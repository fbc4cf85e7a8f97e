// GBM (gradient-boosted trees) kernels for MI355X/gfx950.
//
// The reference does per-feature parallel split search over sorted columns
// on a thread pool (/root/reference/LightCTR/train/train_gbm_algo.cpp:
// 124-135, 215-328). The GPU-native redesign is histogram-based split
// finding (bucketized features, per-node (grad, hess) histograms, then a
// bin scan — the standard GPU GBDT formulation): the histogram build is
// the hot op and lives here; the gain scan is cheap tensor algebra.
//
// LDS-staged version: each workgroup owns one (node, feature-block) pair's
// private LDS histogram, accumulates its row range with LDS atomics, then
// flushes to the global histogram with global atomics once.
#include "common.h"

namespace lightctr {

// bins[N, D] uint8, grad/hess[N], node_of_row[N] int32 (-1 = not in tree
// level), out hist[n_nodes, D, 256, 2] fp32.
// Grid: (feature_blocks, n_nodes); each block grid-strides rows.
#define GBM_FB 4  // features per block (4 * 256 bins * 2 floats = 8 KB LDS)

__global__ void gbm_hist_kernel(const unsigned char* __restrict__ bins,
                                const float* __restrict__ grad,
                                const float* __restrict__ hess,
                                const int* __restrict__ node_of_row,
                                float* __restrict__ hist, int N, int D,
                                int n_nodes) {
  __shared__ float lh[GBM_FB * 256 * 2];
  const int node = blockIdx.y;
  const int f0 = blockIdx.x * GBM_FB;
  const int nf = min(GBM_FB, D - f0);
  for (int i = threadIdx.x; i < GBM_FB * 256 * 2; i += blockDim.x)
    lh[i] = 0.f;
  __syncthreads();
  for (int r = blockIdx.z * blockDim.x + threadIdx.x; r < N;
       r += gridDim.z * blockDim.x) {
    if (node_of_row[r] != node) continue;
    const float g = grad[r];
    const float h = hess[r];
    for (int f = 0; f < nf; ++f) {
      const int b = bins[(size_t)r * D + f0 + f];
      atomicAdd(&lh[(f * 256 + b) * 2 + 0], g);
      atomicAdd(&lh[(f * 256 + b) * 2 + 1], h);
    }
  }
  __syncthreads();
  float* out = &hist[(((size_t)node * D + f0) * 256) * 2];
  for (int i = threadIdx.x; i < nf * 256 * 2; i += blockDim.x) {
    if (lh[i] != 0.f) atomicAdd(&out[i], lh[i]);
  }
}

void gbm_hist_launch(const unsigned char* bins, const float* grad,
                     const float* hess, const int* node_of_row, float* hist,
                     int N, int D, int n_nodes, hipStream_t stream) {
  dim3 block(256);
  const int fb = (D + GBM_FB - 1) / GBM_FB;
  // z-dim row-split sized to fill the 256-CU chip even for few nodes
  int zsplit = max(1, 2048 / max(1, fb * n_nodes));
  dim3 grid(fb, n_nodes, zsplit);
  hipLaunchKernelGGL(gbm_hist_kernel, grid, block, 0, stream, bins, grad,
                     hess, node_of_row, hist, N, D, n_nodes);
}

// ---------------------------------------------------------------------
// Compiled-forest inference (predict/forest.py CompiledForest).
//
// The forest is compiled on the host to float thresholds ("go left if
// x <= thr", NaN follows nan_left), so inference needs no binning pass:
// the kernel reads X directly and touches only the features on each
// row's path. Every node is one 16-byte record
//   .x  float bits: split threshold, or the leaf value
//   .y  feature id (-1 = leaf)
//   .z  left child (tree-local), or the leaf's ordinal inside its tree
//   .w  right child (tree-local) | nan_left << 31
// so one 128-bit load fetches a node.
//
// Work split: thread = GBF_ROWS rows (interleaved walks give the X
// gathers ILP), block = 256 threads = one tile of 1024 rows. The forest
// is visited in host-built chunks of consecutive whole trees whose
// records fit the 48 KiB LDS buffer (3 blocks per CU out of 160 KiB);
// the block stages a chunk with coalesced 16-byte-per-lane loads, syncs,
// walks it, syncs, next chunk. A tree larger than the buffer is its own
// chunk and is walked from global memory. Chunks are visited in tree
// order and each row is owned by one thread, so the per-row fp32 sum is
// the tree-order sum from 0 — no atomics, bit-reproducible.
//
// The walk loop is bounded by the compiled maximum depth; child indices
// are validated on the host to be in range and greater than the parent,
// so every node read is in bounds whatever X holds.
//
// Grid: one block per tile, clamped to GBF_MAX_GRID blocks with a
// grid-stride loop over tiles; the second trip starts at
// N > GBF_MAX_GRID * 1024 = 1,048,576 rows.
#define GBF_BLOCK 256
#define GBF_ROWS 4
#define GBF_TILE (GBF_BLOCK * GBF_ROWS)
#define GBF_CAP 3072  // nodes per LDS chunk (48 KiB)
#define GBF_MAX_GRID 1024
#define GBF_KC 8  // register accumulators for K <= 8 classes

enum { GBF_MARGIN = 0, GBF_LEAF = 1, GBF_FID = 2 };

// Walks trees [first, first + nt) for this thread's rows. `nd` is the
// chunk's node base (LDS or global); tree t starts at tree_off[t] - nbeg.
template <int MODE, int KC, bool NODES_IN_LDS>
__device__ __forceinline__ void gbf_walk_chunk(
    const int4* nd, int first, int nt, int nbeg,
    const int* __restrict__ tree_off, const int* __restrict__ tree_class,
    const int* __restrict__ leaf_base, const float* const (&xr)[GBF_ROWS],
    const long (&row)[GBF_ROWS], const bool (&ok)[GBF_ROWS],
    float (&acc)[GBF_ROWS][KC > 0 ? KC : 1], void* out, int T, int K,
    int max_depth, int fid_offset) {
  for (int t = first; t < first + nt; ++t) {
    const int4* tn = nd + (tree_off[t] - nbeg);
    int idx[GBF_ROWS];
    int4 cur[GBF_ROWS];
#pragma unroll
    for (int j = 0; j < GBF_ROWS; ++j) {
      idx[j] = 0;
      cur[j] = tn[0];
    }
    for (int d = 0; d < max_depth; ++d) {
      bool any = false;
#pragma unroll
      for (int j = 0; j < GBF_ROWS; ++j) {
        const bool internal = cur[j].y >= 0;
        any |= internal;
        const float v = xr[j][internal ? cur[j].y : 0];
        const bool left = (v != v) ? (cur[j].w < 0)
                                   : (v <= __int_as_float(cur[j].x));
        const int nxt = left ? cur[j].z : (cur[j].w & 0x7fffffff);
        idx[j] = internal ? nxt : idx[j];
      }
      if (!any) break;
#pragma unroll
      for (int j = 0; j < GBF_ROWS; ++j) cur[j] = tn[idx[j]];
    }
    if (MODE == GBF_MARGIN) {
      const int cls = tree_class[t];
#pragma unroll
      for (int j = 0; j < GBF_ROWS; ++j) {
        const float val = __int_as_float(cur[j].x);
        if (KC == 1) {
          acc[j][0] += val;
        } else if (KC > 1) {
#pragma unroll
          for (int k = 0; k < KC; ++k)
            acc[j][k] = (k == cls) ? acc[j][k] + val : acc[j][k];
        } else if (ok[j]) {  // K > GBF_KC: thread-owned RMW on zeroed out
          ((float*)out)[(size_t)row[j] * K + cls] += val;
        }
      }
    } else {
      const int lb = (MODE == GBF_FID) ? fid_offset + leaf_base[t] : 0;
#pragma unroll
      for (int j = 0; j < GBF_ROWS; ++j)
        if (ok[j])
          ((int*)out)[(size_t)row[j] * T + t] =
              (MODE == GBF_FID) ? lb + cur[j].z : idx[j];
    }
  }
}

// X[N, D] fp32, nodes[n_nodes] records, tree_off[T+1], tree_class[T],
// leaf_base[T], chunks[n_chunks] = {first tree, n trees, first node,
// fits-LDS flag}. out: MODE margin -> float [N, K] (zeroed by the caller
// when KC == 0); leaf / fid -> int32 [N, T].
template <int MODE, int KC>
__global__ __launch_bounds__(GBF_BLOCK) void gbm_forest_kernel(
    const float* __restrict__ X, const int4* __restrict__ nodes,
    const int* __restrict__ tree_off, const int* __restrict__ tree_class,
    const int* __restrict__ leaf_base, const int4* __restrict__ chunks,
    int n_chunks, void* __restrict__ out, long N, int D, int T, int K,
    int max_depth, int fid_offset) {
  __shared__ int4 s_nodes[GBF_CAP];
  const long n_tiles = (N + GBF_TILE - 1) / GBF_TILE;
  for (long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    long row[GBF_ROWS];
    bool ok[GBF_ROWS];
    const float* xr[GBF_ROWS];
    float acc[GBF_ROWS][KC > 0 ? KC : 1];
#pragma unroll
    for (int j = 0; j < GBF_ROWS; ++j) {
      row[j] = tile * GBF_TILE + j * GBF_BLOCK + threadIdx.x;
      ok[j] = row[j] < N;
      // rows past N walk row 0 (valid memory, N > 0) and store nothing
      xr[j] = X + (size_t)(ok[j] ? row[j] : 0) * D;
#pragma unroll
      for (int k = 0; k < (KC > 0 ? KC : 1); ++k) acc[j][k] = 0.f;
    }
    for (int c = 0; c < n_chunks; ++c) {
      const int4 ch = chunks[c];
      const int nn = tree_off[ch.x + ch.y] - ch.z;
      // block-uniform; the size guard keeps LDS writes in bounds even for
      // a malformed chunk table
      if (ch.w != 0 && nn <= GBF_CAP) {
        __syncthreads();  // previous chunk's readers are done
        for (int i = threadIdx.x; i < nn; i += GBF_BLOCK)
          s_nodes[i] = nodes[ch.z + i];
        __syncthreads();
        gbf_walk_chunk<MODE, KC, true>(s_nodes, ch.x, ch.y, ch.z, tree_off,
                                       tree_class, leaf_base, xr, row, ok,
                                       acc, out, T, K, max_depth,
                                       fid_offset);
      } else {
        gbf_walk_chunk<MODE, KC, false>(nodes + ch.z, ch.x, ch.y, ch.z,
                                        tree_off, tree_class, leaf_base, xr,
                                        row, ok, acc, out, T, K, max_depth,
                                        fid_offset);
      }
    }
    if (MODE == GBF_MARGIN && KC > 0) {
#pragma unroll
      for (int j = 0; j < GBF_ROWS; ++j) {
        if (!ok[j]) continue;
#pragma unroll
        for (int k = 0; k < KC; ++k)
          if (k < K) ((float*)out)[(size_t)row[j] * K + k] = acc[j][k];
      }
    }
  }
}

int gbm_forest_chunk_capacity() { return GBF_CAP; }
int gbm_forest_max_register_classes() { return GBF_KC; }
long gbm_forest_rows_per_grid() { return (long)GBF_MAX_GRID * GBF_TILE; }

void gbm_forest_launch(const float* X, const void* nodes, const int* tree_off,
                       const int* tree_class, const int* leaf_base,
                       const void* chunks, int n_chunks, void* out, long N,
                       int D, int T, int K, int max_depth, int fid_offset,
                       int mode, hipStream_t stream) {
  if (N <= 0 || T <= 0 || n_chunks <= 0) return;
  const long n_tiles = (N + GBF_TILE - 1) / GBF_TILE;
  dim3 block(GBF_BLOCK);
  dim3 grid((unsigned)(n_tiles < GBF_MAX_GRID ? n_tiles : GBF_MAX_GRID));
#define GBF_LAUNCH(M, KCV)                                                  \
  hipLaunchKernelGGL((gbm_forest_kernel<M, KCV>), grid, block, 0, stream, X, \
                     (const int4*)nodes, tree_off, tree_class, leaf_base,   \
                     (const int4*)chunks, n_chunks, out, N, D, T, K,        \
                     max_depth, fid_offset)
  if (mode == GBF_LEAF) {
    GBF_LAUNCH(GBF_LEAF, 0);
  } else if (mode == GBF_FID) {
    GBF_LAUNCH(GBF_FID, 0);
  } else if (K == 1) {
    GBF_LAUNCH(GBF_MARGIN, 1);
  } else if (K <= GBF_KC) {
    GBF_LAUNCH(GBF_MARGIN, GBF_KC);
  } else {
    GBF_LAUNCH(GBF_MARGIN, 0);
  }
#undef GBF_LAUNCH
}

}  // namespace lightctr
