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
