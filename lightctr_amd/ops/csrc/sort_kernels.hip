// Bit-range radix sort for feature-id streams (MI355X / gfx950).
//
// The sorted segment-reduce backward (fm_kernels.hip) needs the batch's
// fids sorted with an index permutation every step. torch.sort runs a
// full 32-bit radix (4 passes over keys+values); feature ids are bounded
// by the table size (<= 2^24 for the Criteo-shaped config, <= U for
// localized ids), so rocPRIM's device radix sort with an explicit
// [0, end_bit) range drops a pass — pure HBM-bytes savings on a
// bandwidth-bound primitive. rocPRIM's LSD sort is stable, which the
// segment-reduce does not even require (any order within an equal-key
// run accumulates the same), so correctness is a strict superset.
//
// Values are int32 (nnz < 2^31): half the payload torch.sort's int64
// indices move through the 2-3 radix passes. Host-side wrappers live
// here because rocPRIM instantiates device kernels (must be compiled by
// hipcc); tensor plumbing stays in bindings.cpp.
#include <algorithm>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "common.h"

namespace lightctr {

__global__ void iota_i32_kernel(int* __restrict__ out, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = i;
}

// The index payload stays a real buffer: handed a counting iterator for the
// values, rocPRIM first copies BOTH inputs into its temp storage (two
// transform launches, 5.8 + 5.9 us at nnz = 2.56 M) so that every pass
// reads pointers — 4.8 us/step slower than this 6.1 us fill
// (profiles/r3_01_fm_segment.txt).
void iota_i32_launch(int* out, int n, hipStream_t stream) {
  if (n <= 0) return;
  int threads = 256;
  int blocks = (n + threads - 1) / threads;
  hipLaunchKernelGGL(iota_i32_kernel, dim3(blocks), dim3(threads), 0, stream,
                     out, n);
}

size_t radix_sort_pairs_i32_temp_bytes(int n, int end_bit) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const int*)nullptr,
                                  (int*)nullptr, (const int*)nullptr,
                                  (int*)nullptr, (size_t)n, 0u,
                                  (unsigned)end_bit, (hipStream_t)0, false);
  return bytes;
}

void radix_sort_pairs_i32_launch(void* temp, size_t temp_bytes,
                                 const int* keys_in, int* keys_out,
                                 const int* vals_in, int* vals_out, int n,
                                 int end_bit, hipStream_t stream) {
  LCTR_CHECK_HIP(rocprim::radix_sort_pairs(temp, temp_bytes, keys_in,
                                           keys_out, vals_in, vals_out,
                                           (size_t)n, 0u, (unsigned)end_bit,
                                           stream, false));
}

// Same sort with an 8-byte payload: the FM training forward writes one
// record {row, bits of x} per entry, and the segment backward reads the
// sorted records in place of a permutation. The payload is handed over as a
// pointer, so no iota fill and no temp-storage copy of the inputs.
using SortRec = unsigned long long;

size_t radix_sort_pairs_rec_temp_bytes(int n, int end_bit) {
  size_t bytes = 0;
  (void)rocprim::radix_sort_pairs(nullptr, bytes, (const int*)nullptr,
                                  (int*)nullptr, (const SortRec*)nullptr,
                                  (SortRec*)nullptr, (size_t)n, 0u,
                                  (unsigned)end_bit, (hipStream_t)0, false);
  return bytes;
}

void radix_sort_pairs_rec_launch(void* temp, size_t temp_bytes,
                                 const int* keys_in, int* keys_out,
                                 const int* rec_in, int* rec_out, int n,
                                 int end_bit, hipStream_t stream) {
  LCTR_CHECK_HIP(rocprim::radix_sort_pairs(
      temp, temp_bytes, keys_in, keys_out, (const SortRec*)rec_in,
      (SortRec*)rec_out, (size_t)n, 0u, (unsigned)end_bit, stream, false));
}

// ---------------------------------------------------------------------------
// Single-purpose onesweep sort for the (fid, record) stream.
//
// Stable LSD radix sort, 8 bits per pass, of int32 keys in [0, 2^end_bit)
// with an 8-byte record payload: one memset, one histogram kernel and one
// scatter kernel per pass (rocPRIM's onesweep at this size: seven fills, a
// histogram, a scan and three passes).
//
// Control block (zeroed by the one memset, at the start of the work
// allocation, a multiple of 16 bytes): kOsMaxPasses x 256 digit counters and
// one ticket counter per pass. Behind it, one look-back state array per pass,
// [tiles][256] words, zeroed by the histogram kernel: a scatter kernel polls
// them, and it starts only after the histogram kernel has ended.
//
// Histogram: every block counts all digit places of its keys in LDS and
// flushes one global atomic per non-empty bin. The exclusive scan of a place
// is done by that pass's tile 0 (the block holding ticket 0), which folds the
// digit bases into the inclusive prefix it publishes; every later tile gets
// them through the look-back chain and never reads the histogram.
//
// Scatter pass (decoupled look-back):
//   * the tile id is a ticket (one atomicAdd, broadcast through LDS), so a
//     tile only waits on tiles whose blocks have already started: no
//     co-residency needed, grid = number of tiles;
//   * a state is one word {2-bit status | 30-bit count} per (tile, digit),
//     stored and polled with relaxed agent-scope atomics (the data is the
//     flag; no fence on the path). The aggregate is published as soon as the
//     tile's digit counts are known, the inclusive prefix as soon as the
//     look-back ends, before the scatter;
//   * every spin is bounded: on give-up the block ORs a code into `status`
//     (caller-owned, never zeroed here) and returns;
//   * ranking is wave-level digit matching (a per-wave table of 64-bit lane
//     masks in LDS) with per-wave digit counters in LDS; a wave owns a
//     contiguous chunk of the tile and walks it in 64-entry rows, so ties stay
//     in input order;
//   * keys and records are reordered by digit in LDS and written out with
//     consecutive lanes on consecutive addresses. The reorder buffers reuse
//     the ranking tables' bytes: 50 KB per 4096-entry tile, 3 blocks per CU,
//     so the flagship's 624 tiles are resident at once.
//
// Fed by a CSR batch (onesweep_sort_csr_launch), pass 0 is the CSR
// instantiation of the scatter kernel: it reads fids and vals, 8 bytes an
// entry, and makes each record {row, bits of x} in registers, the row looked
// up in row_ptr. The records never exist in batch order and the histogram
// kernel is the keys-only one (profiles/r8_01_fm_csr_scatter.txt).
// ---------------------------------------------------------------------------
constexpr int kOsRadix = 256;
constexpr int kOsMaxPasses = 4;
constexpr int kOsCtrlWords = kOsMaxPasses * kOsRadix + kOsMaxPasses;
static_assert(kOsCtrlWords * 4 % 16 == 0, "memset block is 16-byte padded");
static_assert(kOsCtrlWords / 4 <= 1024, "one block zeroes the control block");
constexpr unsigned kOsCountMask = 0x3fffffffu;
constexpr unsigned kOsAggregate = 1u << 30;
constexpr unsigned kOsPrefix = 2u << 30;
constexpr unsigned kOsSpinLimit = 1u << 20;
constexpr int kOsHistMaxThreads = 1024;
constexpr int kOsHistMaxBlocks = 256;
// tile shape and look-back window: the winners of the sweep in
// profiles/r6_01_fm_sort.txt (tiles of 2048 / 4096 / 8192 entries, 256- and
// 512-thread blocks, windows of 1..64); only this shape is built
constexpr int kOsThreads = 512;
constexpr int kOsItems = 8;
constexpr int kOsWindow = 4;

#define OS_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__global__ __launch_bounds__(kOsHistMaxThreads) void onesweep_hist_kernel(
    const int* __restrict__ keys, int n, int passes, unsigned keymask,
    unsigned* ghist, uint4* state, long state_vec4) {
  __shared__ unsigned h[kOsMaxPasses * kOsRadix];
  const int tid = threadIdx.x, threads = blockDim.x;
  for (int i = tid; i < passes * kOsRadix; i += threads) h[i] = 0;
  const long gstride = (long)gridDim.x * threads;
  for (long i = (long)blockIdx.x * threads + tid; i < state_vec4; i += gstride)
    state[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  const int stride = (int)gstride;
#pragma unroll 4
  for (int i = blockIdx.x * threads + tid; i < n; i += stride) {
    const unsigned k = (unsigned)keys[i] & keymask;
#pragma unroll
    for (int p = 0; p < kOsMaxPasses; ++p)
      if (p < passes) atomicAdd(&h[p * kOsRadix + ((k >> (8 * p)) & 255u)], 1u);
  }
  __syncthreads();
  for (int i = tid; i < passes * kOsRadix; i += threads) {
    const unsigned c = h[i];
    if (c) atomicAdd(&ghist[i], c);
  }
}

// exclusive scan of one value per thread over threads 0..255 (threads past
// 255 pass 0 and ignore the result); wsum: 4 words of LDS, one use per array
__device__ __forceinline__ unsigned os_scan256(unsigned v, unsigned* wsum,
                                               int tid) {
  const int lane = tid & 63, w = tid >> 6;
  unsigned incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  if (tid < kOsRadix && lane == 63) wsum[w] = incl;
  __syncthreads();
  unsigned add = 0;
  if (tid < kOsRadix)
    for (int k = 0; k < w; ++k) add += wsum[k];
  return incl - v + add;
}

// LDS of a scatter block: the reorder buffers (8 + 4 bytes per entry), which
// take over the space of the ranking phase's per-wave digit masks and counters
// and the tile's digit bases, then the per-digit output offsets and a few
// words of scan and hand-over scratch.
template <int THREADS, int IPT>
constexpr int os_smem_bytes() {
  constexpr int rank_bytes = (THREADS / 64) * kOsRadix * 12 + kOsRadix * 4;
  constexpr int tile_bytes = THREADS * IPT * 12;
  return (tile_bytes > rank_bytes ? tile_bytes : rank_bytes) + kOsRadix * 4 +
         48;
}

// Row of a CSR entry, for the pass that reads the batch itself: row(t) is the
// last r in [0, B-1] with row_ptr[r] <= t, which for a well-formed row_ptr is
// the one row with row_ptr[r] <= t < row_ptr[r+1], empty rows on either side
// included.
//
// One round of a wave-wide 64-ary search for it over the candidates [lo, hi]
// (wave-uniform, lo <= hi <= B-1): lane l probes lo + (l+1) * step, the 64
// probes cut the span into pieces of at most step - 1, and the number of
// probes that hold picks the piece. 65536 rows take three rounds. Counting
// the probes (not taking the first that fails) keeps the piece inside
// [lo, hi] whatever row_ptr holds.
__device__ __forceinline__ void os_row_search_round(
    const int* __restrict__ row_ptr, int t, int lane, int& lo, int& hi) {
  const int step = ((hi - lo) >> 6) + 1;
  // hi - lo < 2^30 and lane < 64: the probe fits a long, and an int once it
  // is known to be <= hi
  const long p = (long)lo + (long)(lane + 1) * step;
  const bool hit = p <= (long)hi && row_ptr[p] <= t;
  const int c = __popcll(__ballot(hit));
  lo += c * step;
  hi = min(hi, lo + step - 1);
}

template <int THREADS, int IPT, bool CSR>
__global__ __launch_bounds__(THREADS) void onesweep_scatter_kernel(
    const int* __restrict__ keys_in,
    const unsigned long long* __restrict__ rec_in, int* __restrict__ keys_out,
    unsigned long long* __restrict__ rec_out, int n, int shift,
    unsigned keymask, const unsigned* __restrict__ ghist, unsigned* ticket,
    unsigned* state, int* status, const int* __restrict__ row_ptr,
    const float* __restrict__ vals, int B) {
  constexpr int TILE = THREADS * IPT, NW = THREADS / 64;
  static_assert(THREADS >= kOsRadix && THREADS % 64 == 0, "one thread/digit");
  constexpr int rank_bytes = NW * kOsRadix * 12 + kOsRadix * 4;
  constexpr int main_bytes = TILE * 12 > rank_bytes ? TILE * 12 : rank_bytes;
  extern __shared__ __attribute__((aligned(16))) unsigned char os_smem[];
  // reorder phase
  unsigned long long* lrec = (unsigned long long*)os_smem;  // [TILE]
  unsigned* lkeys = (unsigned*)(os_smem + TILE * 8);        // [TILE]
  // ranking phase, same bytes
  unsigned long long* wmask = (unsigned long long*)os_smem;   // [NW][256]
  unsigned* wcnt = (unsigned*)(os_smem + NW * kOsRadix * 8);  // [NW][256]
  unsigned* lbase = wcnt + NW * kOsRadix;                     // [256]
  // both phases
  int* off = (int*)(os_smem + main_bytes);         // [256]
  unsigned* wsum_a = (unsigned*)(off + kOsRadix);  // [4]
  unsigned* wsum_b = wsum_a + 4;                   // [4]
  unsigned* misc = wsum_b + 4;                     // ticket, give-up

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) {
    misc[0] = atomicAdd(ticket, 1u);
    misc[1] = 0;
  }
  // masks and counters are contiguous: NW * 256 * 3 words
  for (int i = tid; i < NW * kOsRadix * 3; i += THREADS)
    ((unsigned*)os_smem)[i] = 0;
  __syncthreads();
  const int tile = (int)misc[0];
  const int tile_base = tile * TILE;
  const int valid_n = min(TILE, n - tile_base);

  // a wave owns entries [w * IPT * 64, (w + 1) * IPT * 64) of the tile and
  // reads them in rows of 64: item i of lane l is entry i * 64 + l of it
  unsigned key[IPT];
  unsigned long long rec[IPT];
  unsigned rank[IPT];
  const int wbase = tile_base + w * (IPT * 64) + lane;
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const int idx = wbase + i * 64;
    const bool v = idx < n;
    key[i] = v ? (unsigned)keys_in[idx] : 0u;
    if constexpr (CSR)  // bits of x for now, the row joins them below
      rec[i] = v ? (unsigned long long)__float_as_uint(vals[idx]) << 32 : 0ull;
    else
      rec[i] = v ? rec_in[idx] : 0ull;
  }
  if constexpr (CSR) {
    // rec = {row(idx), bits of vals[idx]}, what fm_records writes. Nothing
    // here stands in front of the loads above, and the first probes depend on
    // the ticket alone. The wave searches for r0 = row(c0), the row of its
    // chunk's first entry, then loads the starts of the 64 rows behind r0 with
    // one load. If the chunk's last entry c1 lies in front of the last of
    // them (it does unless the rows average under 8 entries), the starts go
    // to 256 bytes of LDS that the ranking phase leaves idle, and every
    // entry counts the starts at or in front of it by a search there: a
    // uniform number of halvings (four at 39 entries a row), the IPT items
    // interleaved, no further global load.
    const int c0 = __builtin_amdgcn_readfirstlane(wbase - lane);
    if (c0 < n) {
      const int c1 = min(c0 + IPT * 64, n) - 1;
      int r0 = 0, hi0 = B - 1;
      while (hi0 > r0) os_row_search_round(row_ptr, c0, lane, r0, hi0);
      const int wr = r0 + 1 + lane;  // rows past B-1 count as never starting
      const int start = wr < B ? row_ptr[wr] : 0x7fffffff;
      // rows of the window that start in the chunk: r0 + cnt <= B-1
      const int cnt = __popcll(__ballot(start <= c1));
      int row[IPT];
      if (cnt < 64) {
        static_assert(rank_bytes + NW * 256 <= main_bytes, "idle LDS");
        int* win = (int*)(os_smem + rank_bytes) + w * 64;
        win[lane] = start;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < IPT; ++i) row[i] = 0;
        for (int len = cnt + 1; len > 1;) {
          const int half = len >> 1;
#pragma unroll
          for (int i = 0; i < IPT; ++i)
            if (win[row[i] + half - 1] <= wbase + i * 64) row[i] += half;
          len -= half;
        }
#pragma unroll
        for (int i = 0; i < IPT; ++i) row[i] += r0;
      } else {
        // 64 rows or more start in the chunk (short and empty rows): search
        // for r1 = row(c1) as well, then every entry searches row_ptr over
        // [r0, r1] itself
        int r1 = r0, hi1 = B - 1;
        while (hi1 > r1) os_row_search_round(row_ptr, c1, lane, r1, hi1);
#pragma unroll
        for (int i = 0; i < IPT; ++i) row[i] = r0;
        for (int len = r1 - r0 + 1; len > 1;) {
          const int half = len >> 1;
#pragma unroll
          for (int i = 0; i < IPT; ++i)
            if (row_ptr[row[i] + half] <= wbase + i * 64) row[i] += half;
          len -= half;
        }
      }
#pragma unroll
      for (int i = 0; i < IPT; ++i) rec[i] |= (unsigned long long)(unsigned)row[i];
    }
  }

  // rank within the wave's chunk, row by row: the entries of a row with the
  // same digit find each other (m: every lane ORs its bit into the digit's
  // word of the wave's mask table and reads the word back; the eight-ballot
  // form measured 2 us slower per pass), each ranks itself behind the wave's count
  // of that digit so far plus its peers in lower lanes, and the lowest peer
  // advances the count. LDS serves a wave's accesses in program order; the
  // wavefront-scope fences emit nothing and keep the compiler from moving or
  // reusing the accesses across rows.
  unsigned* mycnt = wcnt + w * kOsRadix;
  unsigned long long* mymask = wmask + w * kOsRadix;
  const unsigned long long lane_bit = 1ull << lane;
  const unsigned long long lanes_below = lane_bit - 1ull;
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const bool v = wbase + i * 64 < n;
    const unsigned d = ((key[i] & keymask) >> shift) & 255u;
    if (v) atomicOr(&mymask[d], lane_bit);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const unsigned long long m = v ? mymask[d] : 0ull;
    const unsigned below = __popcll(m & lanes_below);
    unsigned prev = 0;
    if (v) prev = mycnt[d];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (v && below == 0) {
      mycnt[d] = prev + (unsigned)__popcll(m);
      mymask[d] = 0ull;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    rank[i] = prev + below;
  }
  __syncthreads();

  // digit d (thread d): tile count, and the per-wave counters turned into
  // exclusive prefixes over the waves
  unsigned cnt = 0;
  if (tid < kOsRadix) {
    for (int k = 0; k < NW; ++k) {
      const unsigned c = wcnt[k * kOsRadix + tid];
      wcnt[k * kOsRadix + tid] = cnt;
      cnt += c;
    }
    if (tile != 0)
      __hip_atomic_store(&state[(size_t)tile * kOsRadix + tid],
                         kOsAggregate | cnt, OS_RLX_AGENT);
  }
  const unsigned lb = os_scan256(cnt, wsum_a, tid);
  if (tid < kOsRadix) lbase[tid] = lb;
  // tile 0 scans this place's histogram: its prefix carries the digit bases
  unsigned excl = 0;
  if (tile == 0)
    excl = os_scan256(tid < kOsRadix ? ghist[tid] : 0u, wsum_b, tid);
  __syncthreads();

  // place of every entry in the tile ordered by digit; the counters' bytes
  // then become the reorder buffers
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    const unsigned d = ((key[i] & keymask) >> shift) & 255u;
    rank[i] += lbase[d] + wcnt[w * kOsRadix + d];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < IPT; ++i) {
    if (wbase + i * 64 < n && rank[i] < (unsigned)TILE) {
      lkeys[rank[i]] = key[i];
      lrec[rank[i]] = rec[i];
    }
  }

  // look-back over lower tickets, one digit per thread; a round loads the
  // next kOsWindow states at once (independent loads) and walks them in order
  if (tid < kOsRadix) {
    bool fail = false;
    if (tile != 0) {
      int t = tile - 1;
      unsigned spins = 0;
      for (;;) {
        unsigned s[kOsWindow];
#pragma unroll
        for (int k = 0; k < kOsWindow; ++k)
          s[k] = t - k >= 0 ? __hip_atomic_load(
                                  &state[(size_t)(t - k) * kOsRadix + tid],
                                  OS_RLX_AGENT)
                            : 0u;
        int used = 0;
        bool done = false;
#pragma unroll
        for (int k = 0; k < kOsWindow; ++k) {
          const unsigned st = s[k] >> 30;
          if (!done && used == k && st != 0u) {
            excl += s[k] & kOsCountMask;
            used = k + 1;
            done = st == 2u;
          }
        }
        if (done) break;
        t -= used;
        if (t < 0) {  // tile 0 only ever publishes a prefix
          fail = true;
          break;
        }
        if (used == 0) {
          ++spins;
          if (spins >= kOsSpinLimit ||
              ((spins & 1023u) == 0u &&
               __hip_atomic_load(status, OS_RLX_AGENT) != 0)) {
            fail = true;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
    }
    if (fail) {
      atomicOr(status, 1);
      misc[1] = 1u;
    } else {
      __hip_atomic_store(&state[(size_t)tile * kOsRadix + tid],
                         kOsPrefix | ((excl + cnt) & kOsCountMask),
                         OS_RLX_AGENT);
    }
    off[tid] = (int)(excl - lb);
  }
  __syncthreads();
  if (misc[1]) return;

  // entry j of the reordered tile goes to (digit base + tiles before) + its
  // place in the tile's run of that digit
  for (int j = tid; j < valid_n; j += THREADS) {
    const unsigned k = lkeys[j];
    const unsigned d = ((k & keymask) >> shift) & 255u;
    const int dst = off[d] + j;
    if ((unsigned)dst < (unsigned)n) {
      keys_out[dst] = (int)k;
      rec_out[dst] = lrec[j];
    }
  }
}

template <int THREADS, int IPT, bool CSR>
void os_scatter_launch(int tiles, const int* keys_in, const SortRec* rec_in,
                       int* keys_out, SortRec* rec_out, int n, int shift,
                       unsigned keymask, const unsigned* ghist,
                       unsigned* ticket, unsigned* state, int* status,
                       const int* row_ptr, const float* vals, int B,
                       hipStream_t stream) {
  constexpr int smem = os_smem_bytes<THREADS, IPT>();
  static_assert(smem <= 160 * 1024, "tile does not fit the LDS");
  auto kernel = onesweep_scatter_kernel<THREADS, IPT, CSR>;
  if (smem > 64 * 1024) {
    static const hipError_t raised = hipFuncSetAttribute(
        (const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, smem);
    LCTR_CHECK_HIP(raised);
  }
  hipLaunchKernelGGL(kernel, dim3(tiles), dim3(THREADS), smem, stream, keys_in,
                     rec_in, keys_out, rec_out, n, shift, keymask, ghist,
                     ticket, state, status, row_ptr, vals, B);
}

int onesweep_sort_tile() { return kOsThreads * kOsItems; }

static int os_passes(int end_bit) { return (end_bit + 7) / 8; }

// bytes of the work buffer: control block + one state array per pass
size_t onesweep_sort_work_bytes(int n, int end_bit) {
  const size_t tile = kOsThreads * kOsItems;
  const size_t tiles = ((size_t)n + tile - 1) / tile;
  return (size_t)kOsCtrlWords * 4 +
         (size_t)os_passes(end_bit) * tiles * kOsRadix * 4;
}

// The histogram kernel and the scatter passes shared by both front ends, behind
// whatever zeroed the control block. The passes ping-pong so that the last one
// lands in the output pair. With a row_ptr, pass 0 takes its records from the
// CSR batch (rec_in is not read); every later pass reads what the one before
// it wrote.
static void os_hist_and_passes(unsigned* ghist, const int* keys_in,
                               int* keys_out, int* keys_tmp,
                               const SortRec* rec_in, SortRec* rec_out,
                               SortRec* rec_tmp, int n, int end_bit,
                               int* status, const int* row_ptr,
                               const float* vals, int B, hipStream_t stream) {
  const int passes = os_passes(end_bit);
  const int tile = kOsThreads * kOsItems;
  const int tiles = (n + tile - 1) / tile;
  const unsigned keymask = (1u << end_bit) - 1u;
  const int hist_blocks = std::min(
      kOsHistMaxBlocks,
      (n + kOsHistMaxThreads * 8 - 1) / (kOsHistMaxThreads * 8));
  hipLaunchKernelGGL(onesweep_hist_kernel, dim3(hist_blocks),
                     dim3(kOsHistMaxThreads), 0, stream, keys_in, n, passes,
                     keymask, ghist, (uint4*)(ghist + kOsCtrlWords),
                     (long)(passes * (size_t)tiles * kOsRadix / 4));
  unsigned* tickets = ghist + kOsMaxPasses * kOsRadix;
  unsigned* state = ghist + kOsCtrlWords;
  const size_t pass_words = (size_t)tiles * kOsRadix;
  const int* ksrc = keys_in;
  const SortRec* rsrc = rec_in;
  for (int p = 0; p < passes; ++p) {
    const bool to_out = ((passes - 1 - p) & 1) == 0;
    int* kdst = to_out ? keys_out : keys_tmp;
    SortRec* rdst = to_out ? rec_out : rec_tmp;
    if (p == 0 && row_ptr)
      os_scatter_launch<kOsThreads, kOsItems, true>(
          tiles, ksrc, nullptr, kdst, rdst, n, 0, keymask, ghist, tickets,
          state, status, row_ptr, vals, B, stream);
    else
      os_scatter_launch<kOsThreads, kOsItems, false>(
          tiles, ksrc, rsrc, kdst, rdst, n, 8 * p, keymask,
          ghist + p * kOsRadix, tickets + p, state + p * pass_words, status,
          nullptr, nullptr, 0, stream);
    ksrc = kdst;
    rsrc = rdst;
  }
}

// keys_in is never written; keys_tmp / rec_tmp (n entries each) are needed
// from two passes on.
void onesweep_sort_rec_launch(void* work, const int* keys_in, int* keys_out,
                              int* keys_tmp, const int* rec_in, int* rec_out,
                              int* rec_tmp, int n, int end_bit, int* status,
                              hipStream_t stream) {
  if (n <= 0) return;
  LCTR_CHECK_HIP(hipMemsetAsync(work, 0, (size_t)kOsCtrlWords * 4, stream));
  os_hist_and_passes((unsigned*)work, keys_in, keys_out, keys_tmp,
                     (const SortRec*)rec_in, (SortRec*)rec_out,
                     (SortRec*)rec_tmp, n, end_bit, status, nullptr, nullptr, 0,
                     stream);
}

// Zeroes the control block in place of the memset: run beside the forward on
// a second stream, the CSR sort is then kernels only, also as a branch of a
// captured graph (profiles/r7_01_fm_overlap.txt, section 4).
__global__ __launch_bounds__(kOsCtrlWords / 4) void onesweep_zero_kernel(
    uint4* ctrl) {
  ctrl[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

// The same sort fed by a CSR batch (n = row_ptr[B] entries): pass 0 reads the
// keys and values of the batch and makes each record {row, bits of x} in
// registers, so no record exists in CSR order and the histogram is the
// keys-only one. keys_tmp / rec_tmp from two passes on, as above.
void onesweep_sort_csr_launch(void* work, const int* row_ptr,
                              const int* keys_in, const float* vals, int B,
                              int* keys_out, int* keys_tmp, int* rec_out,
                              int* rec_tmp, int n, int end_bit, int* status,
                              hipStream_t stream) {
  if (n <= 0 || B <= 0) return;
  hipLaunchKernelGGL(onesweep_zero_kernel, dim3(1), dim3(kOsCtrlWords / 4), 0,
                     stream, (uint4*)work);
  os_hist_and_passes((unsigned*)work, keys_in, keys_out, keys_tmp, nullptr,
                     (SortRec*)rec_out, (SortRec*)rec_tmp, n, end_bit, status,
                     row_ptr, vals, B, stream);
}

// ---------------------------------------------------------------------------
// Work list of the segment backward (fm_kernels.hip,
// fm_segment_apply_kernel). Entry e of the sorted stream starts a piece if
// it is a run head (e == 0 or sorted[e] != sorted[e-1]) or a multiple of
// CAP; a select over 0..n-1 compacts the piece starts in order and leaves
// their count on the device. Every entry is flagged independently, so run
// detection costs one fully parallel pass instead of a serial walk.
// The flag of entry 0 also resets `zero_me` (the consumer's spill counter):
// this pass is ordered before its consumer on the stream, which saves the
// step a one-element fill launch.
// ---------------------------------------------------------------------------
struct PieceStartFlag {
  const int* sorted;
  int cap_mask;  // CAP - 1, CAP a power of two
  int* zero_me;
  __device__ bool operator()(int e) const {
    if (e == 0) {
      if (zero_me) *zero_me = 0;
      return true;
    }
    return (e & cap_mask) == 0 || sorted[e] != sorted[e - 1];
  }
};

using PieceFlagIter =
    rocprim::transform_iterator<rocprim::counting_iterator<int>,
                                PieceStartFlag, bool>;

size_t segment_worklist_temp_bytes(int n) {
  size_t bytes = 0;
  const rocprim::counting_iterator<int> idx(0);
  (void)rocprim::select(nullptr, bytes, idx,
                        PieceFlagIter(idx, PieceStartFlag{nullptr, 0, nullptr}),
                        (int*)nullptr, (int*)nullptr, (size_t)n,
                        (hipStream_t)0, false);
  return bytes;
}

void segment_worklist_launch(void* temp, size_t temp_bytes, const int* sorted,
                             int n, int cap, int* piece_start, int* n_pieces,
                             int* zero_me, hipStream_t stream) {
  const rocprim::counting_iterator<int> idx(0);
  LCTR_CHECK_HIP(rocprim::select(
      temp, temp_bytes, idx,
      PieceFlagIter(idx, PieceStartFlag{sorted, cap - 1, zero_me}),
      piece_start, n_pieces, (size_t)n, stream, false));
}

}  // namespace lightctr
