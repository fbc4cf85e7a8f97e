// PyTorch bindings for the lightctr_amd HIP kernels (MI355X / gfx950) +
// the native data loader. Host-only translation unit.
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>
#include <ATen/cuda/CUDAEvent.h>
#include <c10/cuda/CUDAException.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "launchers.h"

namespace {

#define CHK(x, ...) TORCH_CHECK(x, __VA_ARGS__)

void check_cuda_f32(const at::Tensor& t, const char* name) {
  CHK(t.is_cuda(), name, " must be on GPU");
  CHK(t.scalar_type() == at::kFloat, name, " must be fp32");
  CHK(t.is_contiguous(), name, " must be contiguous");
}

void check_cuda_i32(const at::Tensor& t, const char* name) {
  CHK(t.is_cuda(), name, " must be on GPU");
  CHK(t.scalar_type() == at::kInt, name, " must be int32");
  CHK(t.is_contiguous(), name, " must be contiguous");
}

// the embedding/NFM launchers dispatch K over this set and abort() the
// process on anything else; reject it here as an exception instead
void check_embed_k(int64_t K) {
  CHK(K == 4 || K == 8 || K == 16 || K == 32 || K == 64,
      "latent width K must be one of 4, 8, 16, 32, 64, got ", K);
}

// The FM launchers dispatch K over the same set and abort() likewise: V is
// [F, K] fp32 with K in it. Returns K.
int check_fm_v(const at::Tensor& V) {
  check_cuda_f32(V, "V");
  CHK(V.dim() == 2, "V must be [F, K]");
  check_embed_k(V.size(1));
  return (int)V.size(1);
}

// fp32 / int32 device array of exactly n elements
void check_f32_n(const at::Tensor& t, int64_t n, const char* name) {
  check_cuda_f32(t, name);
  CHK(t.numel() == n, name, " must hold ", n, " elements, got ", t.numel());
}

void check_i32_n(const at::Tensor& t, int64_t n, const char* name) {
  check_cuda_i32(t, name);
  CHK(t.numel() == n, name, " must hold ", n, " elements, got ", t.numel());
}

// touched bitmap: one 64-bit word per 64 features
void check_touched(const at::Tensor& touched, int64_t F) {
  CHK(touched.is_cuda(), "touched must be on GPU");
  CHK(touched.scalar_type() == at::kLong ||
          touched.scalar_type() == at::kUInt64,
      "touched must be 64-bit");
  CHK(touched.is_contiguous(), "touched must be contiguous");
  CHK(touched.numel() >= (F + 63) / 64, "touched must hold ", (F + 63) / 64,
      " words for ", F, " features, got ", touched.numel());
}

// CSR batch of the FM row kernels: B + 1 offsets, one value per entry.
// Returns B.
int check_fm_csr(const at::Tensor& row_ptr, const at::Tensor& fids,
                 const at::Tensor& vals) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_i32(fids, "fids");
  check_cuda_f32(vals, "vals");
  CHK(row_ptr.numel() >= 1, "row_ptr must hold B + 1 offsets");
  CHK(vals.numel() == fids.numel(), "vals must have one value per entry");
  return (int)row_ptr.numel() - 1;
}

// the FFM launchers dispatch K over the same set and abort() likewise
void check_ffm_v(const at::Tensor& V) {
  CHK(V.dim() == 3, "V must be [F, nfields, K]");
  check_embed_k(V.size(2));
}

// ffm_sorted_backward / ffm_block_emit keep one [nfields, K+1] fp32 block
// per wave in dynamic LDS; a request past the per-block limit is a launch
// error that would leave the gradients unwritten
void check_ffm_block_lds(int nfields, int K, const char* op) {
  const long need = lightctr::ffm_block_lds_bytes(nfields, K);
  const long have = lightctr::ffm_max_lds_per_block();
  CHK(need <= have, op, ": nfields=", nfields, ", K=", K, " needs ", need,
      " bytes of LDS per block, the device gives ", have);
}

ihipStream_t* cur_stream() {
  return (ihipStream_t*)at::cuda::getCurrentCUDAStream().stream();
}

// sort permutations are int32 end-to-end (half the radix payload of
// torch.sort's int64 indices); accept int64 for compatibility (e.g.
// torch.sort callers in tests) by converting.
at::Tensor perm32(const at::Tensor& perm) {
  if (perm.scalar_type() == at::kInt) return perm;
  CHK(perm.scalar_type() == at::kLong, "perm must be int32 or int64");
  return perm.to(at::kInt);
}

// ---- FM ----

std::vector<at::Tensor> fm_forward(at::Tensor row_ptr, at::Tensor fids,
                                   at::Tensor vals, at::Tensor W,
                                   at::Tensor V) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_fm_v(V);
  check_f32_n(W, V.size(0), "W");
  auto pred = at::empty({B}, W.options());
  auto sumVX = at::empty({B, K}, W.options());
  if (B == 0) return {pred, sumVX};  // nothing is launched for an empty batch
  lightctr::fm_forward_launch(row_ptr.data_ptr<int>(), fids.data_ptr<int>(),
                              vals.data_ptr<float>(), W.data_ptr<float>(),
                              V.data_ptr<float>(), pred.data_ptr<float>(),
                              sumVX.data_ptr<float>(), B, K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {pred, sumVX};
}

// [n, 2] int32 records {row, bits of x}; read and written as 8-byte words
void check_cuda_rec(const at::Tensor& t, long n, const char* name) {
  check_cuda_i32(t, name);
  CHK(t.dim() == 2 && t.size(0) == n && t.size(1) == 2, name,
      " must be [n, 2]");
  CHK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 8 == 0, name,
      " must be 8-byte aligned");
}

// Training forward: fm_forward + logloss_grad in one launch, plus the
// per-entry records rec[j] = {row of j, bits of vals[j]} that the segment
// backward sorts by fid. Returns (loss, dpred, sumVX, rec). `reset`
// (optional int32 [1], the backward's spill counter) is zeroed by the same
// launch.
std::vector<at::Tensor> fm_forward_train(at::Tensor row_ptr, at::Tensor fids,
                                         at::Tensor vals, at::Tensor W,
                                         at::Tensor V, at::Tensor label,
                                         double scale,
                                         c10::optional<at::Tensor> reset) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_fm_v(V);
  check_f32_n(W, V.size(0), "W");
  check_cuda_f32(label, "label");
  const long nnz = fids.numel();
  CHK(label.numel() == B, "label must have one value per row");
  auto loss = at::empty({B}, W.options());
  auto dpred = at::empty({B}, W.options());
  auto sumVX = at::empty({B, K}, W.options());
  auto rec = at::empty({nnz, 2}, fids.options());
  int* reset_ptr = nullptr;
  if (reset.has_value()) {
    check_cuda_i32(*reset, "reset");
    CHK(reset->numel() >= 1, "reset must hold one int");
    reset_ptr = reset->data_ptr<int>();
    if (B <= 0) reset->zero_();  // nothing is launched for an empty batch
  }
  if (B == 0) return {loss, dpred, sumVX, rec};
  lightctr::fm_forward_train_launch(
      row_ptr.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      W.data_ptr<float>(), V.data_ptr<float>(), label.data_ptr<float>(),
      (float)scale, loss.data_ptr<float>(), dpred.data_ptr<float>(),
      sumVX.data_ptr<float>(), rec.data_ptr<int>(), B, K, reset_ptr,
      cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {loss, dpred, sumVX, rec};
}

std::vector<at::Tensor> logloss_grad(at::Tensor pred, at::Tensor label,
                                     double scale) {
  check_cuda_f32(pred, "pred");
  check_cuda_f32(label, "label");
  const int B = (int)pred.numel();
  CHK(label.numel() == B, "label must have one value per row");
  auto loss = at::empty_like(pred);
  auto dpred = at::empty_like(pred);
  if (B == 0) return {loss, dpred};
  lightctr::logloss_grad_launch(pred.data_ptr<float>(),
                                label.data_ptr<float>(),
                                loss.data_ptr<float>(), dpred.data_ptr<float>(),
                                (float)scale, B, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {loss, dpred};
}

void fm_backward(at::Tensor row_ptr, at::Tensor fids, at::Tensor vals,
                 at::Tensor V, at::Tensor sumVX, at::Tensor dpred,
                 at::Tensor gradW, at::Tensor gradV, at::Tensor touched) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_fm_v(V);
  const int64_t F = V.size(0);
  check_f32_n(sumVX, (int64_t)B * K, "sumVX");
  check_f32_n(dpred, B, "dpred");
  check_f32_n(gradW, F, "gradW");
  check_f32_n(gradV, F * K, "gradV");
  check_touched(touched, F);
  if (B == 0) return;
  lightctr::fm_backward_launch(
      row_ptr.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      V.data_ptr<float>(), sumVX.data_ptr<float>(), dpred.data_ptr<float>(),
      gradW.data_ptr<float>(), gradV.data_ptr<float>(),
      (unsigned long long*)touched.data_ptr(), B, K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

std::vector<at::Tensor> fm_backward_emit(at::Tensor row_ptr, at::Tensor fids,
                                         at::Tensor vals, at::Tensor V,
                                         at::Tensor sumVX, at::Tensor dpred,
                                         c10::optional<at::Tensor> pos) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_fm_v(V);
  check_f32_n(sumVX, (int64_t)B * K, "sumVX");
  check_f32_n(dpred, B, "dpred");
  const auto nnz = fids.numel();
  auto gw = at::empty({nnz}, V.options());
  auto gv = at::empty({nnz, K}, V.options());
  const int* pos_ptr = nullptr;
  if (pos.has_value()) {
    check_cuda_i32(*pos, "pos");
    CHK(pos->numel() == nnz, "pos must have one slot per entry");
    pos_ptr = pos->data_ptr<int>();
  }
  if (B == 0 || nnz == 0) return {gw, gv};
  lightctr::fm_backward_emit_launch(
      row_ptr.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      V.data_ptr<float>(), sumVX.data_ptr<float>(), dpred.data_ptr<float>(),
      gw.data_ptr<float>(), gv.data_ptr<float>(), B, K, pos_ptr,
      cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {gw, gv};
}

// inverse permutation (write slots for scatter-emit): inv[perm[i]] = i
at::Tensor inv_perm_i32(at::Tensor perm_in) {
  auto perm = perm32(perm_in).contiguous();
  CHK(perm.is_cuda(), "perm must be on GPU");
  const int n = (int)perm.numel();
  auto inv = at::empty({n}, perm.options());
  if (n == 0) return inv;
  lightctr::inv_perm_launch(perm.data_ptr<int>(), inv.data_ptr<int>(), n,
                            cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return inv;
}

// What both sorted applies read: the sorted stream, the per-entry gradients
// behind it, the slabs and the bitmap. Returns K (from gradV [F, K]);
// perm_i holds the int32 permutation when one is given.
int check_sorted_apply(const at::Tensor& sorted_fids,
                       const c10::optional<at::Tensor>& perm,
                       const at::Tensor& gw, const at::Tensor& gv,
                       const at::Tensor& gradW, const at::Tensor& gradV,
                       const at::Tensor& touched, at::Tensor& perm_i) {
  check_cuda_i32(sorted_fids, "sorted_fids");
  check_cuda_f32(gradV, "gradV");
  CHK(gradV.dim() == 2, "gradV must be [F, K]");
  check_embed_k(gradV.size(1));
  const int64_t nnz = sorted_fids.numel();
  const int64_t F = gradV.size(0), K = gradV.size(1);
  check_f32_n(gradW, F, "gradW");
  check_f32_n(gw, nnz, "gw");
  check_f32_n(gv, nnz * K, "gv");
  check_touched(touched, F);
  if (perm.has_value()) {
    CHK(perm->is_cuda(), "perm must be on GPU");
    CHK(perm->numel() == nnz, "perm must have one slot per entry");
    perm_i = perm32(*perm).contiguous();
  }
  return (int)K;
}

void fm_sorted_apply(at::Tensor sorted_fids, c10::optional<at::Tensor> perm,
                     at::Tensor gw, at::Tensor gv, at::Tensor gradW,
                     at::Tensor gradV, at::Tensor touched, int64_t chunk) {
  at::Tensor perm_i;
  const int K = check_sorted_apply(sorted_fids, perm, gw, gv, gradW, gradV,
                                   touched, perm_i);
  CHK(chunk >= -4 && chunk <= std::numeric_limits<int>::max(),
      "chunk must be positive or one of 0 (default walk), -1, -2 (segmented "
      "scans), -3, -4 (walk variants), got ", chunk);
  const int* perm_ptr = perm.has_value() ? perm_i.data_ptr<int>() : nullptr;
  if (sorted_fids.numel() == 0) return;
  lightctr::fm_sorted_apply_launch(
      sorted_fids.data_ptr<int>(), perm_ptr,
      gw.data_ptr<float>(), gv.data_ptr<float>(), gradW.data_ptr<float>(),
      gradV.data_ptr<float>(), (unsigned long long*)touched.data_ptr(),
      (int)sorted_fids.numel(), K, 0, nullptr, nullptr, nullptr, nullptr,
      nullptr, nullptr, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, (int)chunk,
      cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// Fused variant: interior feature segments get their optimizer update
// applied during the segment reduction; only boundary-spanning features go
// through the slab + bitmap (+ the follow-up sparse apply).
void fm_sorted_apply_fused(at::Tensor sorted_fids,
                           c10::optional<at::Tensor> perm,
                           at::Tensor gw, at::Tensor gv, at::Tensor gradW,
                           at::Tensor gradV, at::Tensor touched,
                           at::Tensor W, at::Tensor V, at::Tensor nW,
                           at::Tensor nV, c10::optional<at::Tensor> zW,
                           c10::optional<at::Tensor> zV, int64_t opt_mode,
                           double p0, double p1, double p2, double p3,
                           double v_lr, double v_eps, double v_l2) {
  at::Tensor perm_i;
  const int K = check_sorted_apply(sorted_fids, perm, gw, gv, gradW, gradV,
                                   touched, perm_i);
  const int* perm_ptr = perm.has_value() ? perm_i.data_ptr<int>() : nullptr;
  CHK(opt_mode == 1 || opt_mode == 2 || opt_mode == 3,
      "opt_mode 1=adagrad 2=ftrl 3=ftrlW+adagradV");
  const int64_t F = gradV.size(0);
  CHK(check_fm_v(V) == K && V.size(0) == F, "V must match gradV");
  check_f32_n(W, F, "W");
  check_f32_n(nW, F, "nW");
  check_f32_n(nV, F * K, "nV");
  if (opt_mode != 1) {
    CHK(zW.has_value(), "FTRL needs zW");
    check_f32_n(*zW, F, "zW");
  }
  if (opt_mode == 2) {
    CHK(zV.has_value(), "FTRL on V needs zV");
    check_f32_n(*zV, F * K, "zV");
  }
  if (sorted_fids.numel() == 0) return;
  lightctr::fm_sorted_apply_launch(
      sorted_fids.data_ptr<int>(), perm_ptr,
      gw.data_ptr<float>(), gv.data_ptr<float>(), gradW.data_ptr<float>(),
      gradV.data_ptr<float>(), (unsigned long long*)touched.data_ptr(),
      (int)sorted_fids.numel(), K, (int)opt_mode, V.data_ptr<float>(),
      W.data_ptr<float>(), nW.data_ptr<float>(),
      zW.has_value() ? zW->data_ptr<float>() : nullptr,
      nV.data_ptr<float>(),
      zV.has_value() ? zV->data_ptr<float>() : nullptr, (float)p0,
      (float)p1, (float)p2, (float)p3, (float)v_lr, (float)v_eps,
      (float)v_l2, 384, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// Work list of the segment backward: (piece_start int32 [nnz], n_pieces
// int32 [1]); the first n_pieces entries of piece_start are the piece
// starts in order. Temp storage comes from the torch allocator, no host
// sync. `reset` (optional int32 [1]) is zeroed by the same pass.
std::vector<at::Tensor> segment_worklist(at::Tensor sorted_fids, int64_t cap,
                                         c10::optional<at::Tensor> reset) {
  check_cuda_i32(sorted_fids, "sorted_fids");
  CHK(cap >= 1 && cap <= (1 << 30) && (cap & (cap - 1)) == 0,
      "cap must be a power of two");
  const int n = (int)sorted_fids.numel();
  auto piece_start = at::empty({n}, sorted_fids.options());
  int* reset_ptr = nullptr;
  if (reset.has_value()) {
    check_cuda_i32(*reset, "reset");
    CHK(reset->numel() >= 1, "reset must hold one int");
    reset_ptr = reset->data_ptr<int>();
  }
  if (n == 0) {
    if (reset.has_value()) reset->zero_();
    return {piece_start, at::zeros({1}, sorted_fids.options())};
  }
  auto n_pieces = at::empty({1}, sorted_fids.options());
  const unsigned long bytes = lightctr::segment_worklist_temp_bytes(n);
  auto temp = at::empty({(long)bytes}, sorted_fids.options().dtype(at::kByte));
  lightctr::segment_worklist_launch(
      temp.data_ptr(), bytes, sorted_fids.data_ptr<int>(), n, (int)cap,
      piece_start.data_ptr<int>(), n_pieces.data_ptr<int>(), reset_ptr,
      cur_stream());
  return {piece_start, n_pieces};
}

// Argument checks of every segment backward: slabs, spill list, parameters
// and optimizer state
void check_segment_state(const at::Tensor& sorted_fids,
                         const at::Tensor& gradW, const at::Tensor& gradV,
                         const at::Tensor& spill,
                         const at::Tensor& spill_count, const at::Tensor& W,
                         const at::Tensor& V, const at::Tensor& nW,
                         const at::Tensor& nV,
                         const c10::optional<at::Tensor>& zW,
                         const c10::optional<at::Tensor>& zV,
                         int64_t opt_mode) {
  check_cuda_i32(sorted_fids, "sorted_fids");
  check_cuda_i32(spill, "spill");
  check_cuda_i32(spill_count, "spill_count");
  check_cuda_f32(gradW, "gradW");
  check_cuda_f32(gradV, "gradV");
  check_cuda_f32(W, "W");
  check_cuda_f32(V, "V");
  check_cuda_f32(nW, "nW");
  check_cuda_f32(nV, "nV");
  const int K = check_fm_v(V);
  CHK(spill_count.numel() >= 1, "counters");
  CHK(gradV.numel() == V.numel() && gradW.numel() == W.numel() &&
          nV.numel() == V.numel() && nW.numel() == W.numel() &&
          V.numel() == W.numel() * K,
      "parameter / state / slab shapes must match");
  CHK(opt_mode == 1 || opt_mode == 2 || opt_mode == 3,
      "opt_mode 1=adagrad 2=ftrl 3=ftrlW+adagradV");
  if (opt_mode != 1) {
    CHK(zW.has_value(), "FTRL needs zW");
    check_cuda_f32(*zW, "zW");
    CHK(zW->numel() == W.numel(), "zW shape");
  }
  if (opt_mode == 2) {
    CHK(zV.has_value(), "FTRL on V needs zV");
    check_cuda_f32(*zV, "zV");
    CHK(zV->numel() == V.numel(), "zV shape");
  }
}

// The same plus the work list of the two list-fed entry sources
void check_segment_common(const at::Tensor& sorted_fids,
                          const at::Tensor& piece_start,
                          const at::Tensor& n_pieces, const at::Tensor& gradW,
                          const at::Tensor& gradV, const at::Tensor& spill,
                          const at::Tensor& spill_count, const at::Tensor& W,
                          const at::Tensor& V, const at::Tensor& nW,
                          const at::Tensor& nV,
                          const c10::optional<at::Tensor>& zW,
                          const c10::optional<at::Tensor>& zV,
                          int64_t opt_mode) {
  check_segment_state(sorted_fids, gradW, gradV, spill, spill_count, W, V, nW,
                      nV, zW, zV, opt_mode);
  check_cuda_i32(piece_start, "piece_start");
  check_cuda_i32(n_pieces, "n_pieces");
  CHK(piece_start.numel() >= sorted_fids.numel(),
      "piece_start must hold nnz entries");
  CHK(n_pieces.numel() >= 1, "counters");
}

// Segment backward: one K-lane subgroup per piece of the work list sums the
// piece's gradients; whole pieces get the optimizer update in place,
// partial ones go to the slabs and `spill` (fid list + counter, consumed by
// fm_adagrad_apply / fm_ftrl_apply). opt_mode as in fm_sorted_apply_fused.
void fm_segment_apply(at::Tensor sorted_fids, c10::optional<at::Tensor> perm,
                      at::Tensor piece_start, at::Tensor n_pieces,
                      at::Tensor gw, at::Tensor gv, at::Tensor gradW,
                      at::Tensor gradV, at::Tensor spill,
                      at::Tensor spill_count, at::Tensor W, at::Tensor V,
                      at::Tensor nW, at::Tensor nV,
                      c10::optional<at::Tensor> zW,
                      c10::optional<at::Tensor> zV, int64_t opt_mode,
                      double p0, double p1, double p2, double p3, double v_lr,
                      double v_eps, double v_l2) {
  check_segment_common(sorted_fids, piece_start, n_pieces, gradW, gradV, spill,
                       spill_count, W, V, nW, nV, zW, zV, opt_mode);
  check_cuda_f32(gw, "gw");
  check_cuda_f32(gv, "gv");
  const long nnz = sorted_fids.numel();
  const int K = (int)V.size(1);
  CHK(gw.numel() == nnz && gv.numel() == nnz * K, "gw/gv shape");
  const int* perm_ptr = nullptr;
  at::Tensor perm_i;
  if (perm.has_value()) {
    perm_i = perm32(*perm).contiguous();
    CHK(perm_i.is_cuda() && perm_i.numel() == nnz, "perm shape");
    perm_ptr = perm_i.data_ptr<int>();
  }
  const int num_cus =
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  lightctr::fm_segment_apply_launch(
      sorted_fids.data_ptr<int>(), perm_ptr, piece_start.data_ptr<int>(),
      n_pieces.data_ptr<int>(), gw.data_ptr<float>(), gv.data_ptr<float>(),
      gradW.data_ptr<float>(), gradV.data_ptr<float>(),
      spill.data_ptr<int>(), spill_count.data_ptr<int>(), (int)spill.numel(),
      (int)nnz, K, (int)opt_mode, V.data_ptr<float>(), W.data_ptr<float>(),
      nW.data_ptr<float>(),
      zW.has_value() ? zW->data_ptr<float>() : nullptr, nV.data_ptr<float>(),
      zV.has_value() ? zV->data_ptr<float>() : nullptr, (float)p0, (float)p1,
      (float)p2, (float)p3, (float)v_lr, (float)v_eps, (float)v_l2,
      num_cus, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// Segment backward from the sorted records of fm_forward_train: each entry's
// gradient is recomputed from (row, x), sumVX[row], dpred[row] and the V row
// its piece loads, so there is no per-entry gradient buffer and no perm.
void fm_segment_apply_rec(at::Tensor sorted_fids, at::Tensor sorted_rec,
                          at::Tensor sumVX, at::Tensor dpred,
                          at::Tensor piece_start, at::Tensor n_pieces,
                          at::Tensor gradW, at::Tensor gradV, at::Tensor spill,
                          at::Tensor spill_count, at::Tensor W, at::Tensor V,
                          at::Tensor nW, at::Tensor nV,
                          c10::optional<at::Tensor> zW,
                          c10::optional<at::Tensor> zV, int64_t opt_mode,
                          double p0, double p1, double p2, double p3,
                          double v_lr, double v_eps, double v_l2) {
  check_segment_common(sorted_fids, piece_start, n_pieces, gradW, gradV, spill,
                       spill_count, W, V, nW, nV, zW, zV, opt_mode);
  const long nnz = sorted_fids.numel();
  const int K = (int)V.size(1);
  check_cuda_rec(sorted_rec, nnz, "sorted_rec");
  check_cuda_f32(sumVX, "sumVX");
  check_cuda_f32(dpred, "dpred");
  const long B = dpred.numel();
  CHK(sumVX.numel() == B * K, "sumVX must be [B, K]");
  CHK(nnz == 0 || B >= 1, "entries need rows");
  const int num_cus =
      at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  lightctr::fm_segment_recompute_launch(
      sorted_fids.data_ptr<int>(), sorted_rec.data_ptr<int>(),
      sumVX.data_ptr<float>(), dpred.data_ptr<float>(), (int)B,
      piece_start.data_ptr<int>(), n_pieces.data_ptr<int>(),
      gradW.data_ptr<float>(), gradV.data_ptr<float>(),
      spill.data_ptr<int>(), spill_count.data_ptr<int>(), (int)spill.numel(),
      (int)nnz, K, (int)opt_mode, V.data_ptr<float>(), W.data_ptr<float>(),
      nW.data_ptr<float>(),
      zW.has_value() ? zW->data_ptr<float>() : nullptr, nV.data_ptr<float>(),
      zV.has_value() ? zV->data_ptr<float>() : nullptr, (float)p0, (float)p1,
      (float)p2, (float)p3, (float)v_lr, (float)v_eps, (float)v_l2,
      num_cus, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// Tile-local segment backward from the sorted records: what
// fm_segment_apply_rec computes, with every block finding the pieces of its
// own tile of fm_segment_tile() entries (no work list). cap must divide the
// tile. spill_count is not reset here: fm_forward_train(reset=) does that.
void fm_segment_tile_rec(at::Tensor sorted_fids, at::Tensor sorted_rec,
                         at::Tensor sumVX, at::Tensor dpred, int64_t cap,
                         at::Tensor gradW, at::Tensor gradV, at::Tensor spill,
                         at::Tensor spill_count, at::Tensor W, at::Tensor V,
                         at::Tensor nW, at::Tensor nV,
                         c10::optional<at::Tensor> zW,
                         c10::optional<at::Tensor> zV, int64_t opt_mode,
                         double p0, double p1, double p2, double p3,
                         double v_lr, double v_eps, double v_l2) {
  check_segment_state(sorted_fids, gradW, gradV, spill, spill_count, W, V, nW,
                      nV, zW, zV, opt_mode);
  const long tile = lightctr::fm_segment_tile();
  CHK(cap >= 1 && (cap & (cap - 1)) == 0 && cap <= tile && tile % cap == 0,
      "cap must be a power of two that divides the tile of ", tile);
  const long nnz = sorted_fids.numel();
  const int K = (int)V.size(1);
  check_cuda_rec(sorted_rec, nnz, "sorted_rec");
  check_cuda_f32(sumVX, "sumVX");
  check_cuda_f32(dpred, "dpred");
  const long B = dpred.numel();
  CHK(sumVX.numel() == B * K, "sumVX must be [B, K]");
  CHK(nnz == 0 || B >= 1, "entries need rows");
  lightctr::fm_segment_tile_launch(
      sorted_fids.data_ptr<int>(), sorted_rec.data_ptr<int>(),
      sumVX.data_ptr<float>(), dpred.data_ptr<float>(), (int)B, (int)cap,
      gradW.data_ptr<float>(), gradV.data_ptr<float>(),
      spill.data_ptr<int>(), spill_count.data_ptr<int>(), (int)spill.numel(),
      (int)nnz, K, (int)opt_mode, V.data_ptr<float>(), W.data_ptr<float>(),
      nW.data_ptr<float>(),
      zW.has_value() ? zW->data_ptr<float>() : nullptr, nV.data_ptr<float>(),
      zV.has_value() ? zV->data_ptr<float>() : nullptr, (float)p0, (float)p1,
      (float)p2, (float)p3, (float)v_lr, (float)v_eps, (float)v_l2,
      cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// ---- FFM ----

at::Tensor ffm_forward(at::Tensor row_ptr, at::Tensor fields, at::Tensor fids,
                       at::Tensor vals, at::Tensor W, at::Tensor V) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_i32(fields, "fields");
  check_cuda_i32(fids, "fids");
  const bool v_bf16 = V.scalar_type() == at::kBFloat16;
  CHK(v_bf16 || V.scalar_type() == at::kFloat, "V must be fp32 or bf16");
  const int B = (int)row_ptr.numel() - 1;
  check_ffm_v(V);
  const int nfields = (int)V.size(1);
  const int K = (int)V.size(2);
  auto pred = at::empty({B}, W.options());
  // lane-per-pair layout: 458 vs 1174 us for the (pair-group, k) layout
  // at B=65536/nf=39/K=8 (tools/ab_ffm_fwd.py; bit-identical output).
  // The group kernel and a per-row LDS-staged variant (1611 us — LDS
  // capacity caps occupancy) stay in ffm_kernels.hip as documented
  // experiments.
  lightctr::ffm_forward_pp_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), W.data_ptr<float>(), V.data_ptr(),
      v_bf16 ? 1 : 0, pred.data_ptr<float>(), nfields, B, K, cur_stream());
  return pred;
}

// lane-per-pair forward variant (A/B against the group layout)
at::Tensor ffm_forward_pp(at::Tensor row_ptr, at::Tensor fields,
                          at::Tensor fids, at::Tensor vals, at::Tensor W,
                          at::Tensor V) {
  check_cuda_i32(row_ptr, "row_ptr");
  const int B = (int)row_ptr.numel() - 1;
  check_ffm_v(V);
  const int nfields = (int)V.size(1);
  const int K = (int)V.size(2);
  auto pred = at::empty({B}, W.options());
  lightctr::ffm_forward_pp_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), W.data_ptr<float>(), V.data_ptr(),
      V.scalar_type() == at::kBFloat16 ? 1 : 0, pred.data_ptr<float>(),
      nfields, B, K, cur_stream());
  return pred;
}

// per-row staged fp16 block emit -> (gw fp32, gblocks fp16 [nnz, nf*K])
std::vector<at::Tensor> ffm_row_emit(at::Tensor row_ptr, at::Tensor fields,
                                     at::Tensor fids, at::Tensor vals,
                                     at::Tensor V, at::Tensor dpred,
                                     double scale) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_i32(fields, "fields");
  check_cuda_i32(fids, "fids");
  const bool v_bf16 = V.scalar_type() == at::kBFloat16;
  CHK(v_bf16 || V.scalar_type() == at::kFloat, "V must be fp32 or bf16");
  const int B = (int)row_ptr.numel() - 1;
  check_ffm_v(V);
  const int nfields = (int)V.size(1);
  const int K = (int)V.size(2);
  const int maxn = 40;
  CHK(lightctr::ffm_staged_eligible(nfields, K, maxn),
      "nfields*K too large for the staged row emit");
  const auto nnz = fids.numel();
  auto gw = at::empty({nnz}, vals.options());
  auto gblocks = at::empty({nnz, (long)nfields * K},
                           vals.options().dtype(at::kHalf));
  lightctr::ffm_row_emit_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), V.data_ptr(), v_bf16 ? 1 : 0,
      dpred.data_ptr<float>(), gblocks.data_ptr(), gw.data_ptr<float>(),
      nfields, B, maxn, K, (float)scale, cur_stream());
  return {gw, gblocks};
}

void ffm_blocks_apply_f16(at::Tensor sorted_fids, at::Tensor perm,
                          at::Tensor gblocks, at::Tensor gw, at::Tensor gradW,
                          at::Tensor gradV, at::Tensor touched,
                          double inv_scale, int64_t opt_mode,
                          c10::optional<at::Tensor> V,
                          c10::optional<at::Tensor> W,
                          c10::optional<at::Tensor> nW,
                          c10::optional<at::Tensor> zW,
                          c10::optional<at::Tensor> nV,
                          c10::optional<at::Tensor> Vh,
                          double p0, double p1, double p2, double p3,
                          double q0, double q1, double q2) {
  check_cuda_i32(sorted_fids, "sorted_fids");
  auto perm_i = perm32(perm).contiguous();
  CHK(gblocks.scalar_type() == at::kHalf, "gblocks must be fp16");
  CHK(opt_mode == 0 || opt_mode == 1 || opt_mode == 3,
      "opt_mode 0=slab 1=adagrad 3=ftrlW+adagradV");
  if (opt_mode != 0) {
    CHK(V && W && nW && nV, "fused apply needs V/W/nW/nV");
    if (opt_mode == 3) CHK(zW.has_value(), "opt_mode 3 needs zW");
  }
  CHK(gradV.dim() == 2 && gblocks.dim() == 2, "gradV and gblocks must be 2-d");
  const int D = (int)gradV.size(1);
  CHK(gblocks.size(1) == gradV.size(1), "gblocks width ", gblocks.size(1),
      " differs from gradV width ", gradV.size(1));
  CHK(D % 4 == 0 && D <= 1024, "ffm_blocks_apply_f16: D=", D,
      " unsupported (needs D % 4 == 0 and D <= 1024)");
  lightctr::ffm_blocks_apply_f16_launch(
      sorted_fids.data_ptr<int>(), perm_i.data_ptr<int>(), gblocks.data_ptr(),
      gw.data_ptr<float>(), gradW.data_ptr<float>(), gradV.data_ptr<float>(),
      (unsigned long long*)touched.data_ptr(), D, (int)sorted_fids.numel(),
      (float)inv_scale, (int)opt_mode,
      V ? V->data_ptr<float>() : nullptr,
      W ? W->data_ptr<float>() : nullptr,
      nW ? nW->data_ptr<float>() : nullptr,
      zW ? zW->data_ptr<float>() : nullptr,
      nV ? nV->data_ptr<float>() : nullptr,
      Vh ? Vh->data_ptr() : nullptr, (float)p0, (float)p1, (float)p2,
      (float)p3, (float)q0, (float)q1, (float)q2, cur_stream());
}

void ffm_backward(at::Tensor row_ptr, at::Tensor fields, at::Tensor fids,
                  at::Tensor vals, at::Tensor V, at::Tensor dpred,
                  at::Tensor gradW, at::Tensor gradV, at::Tensor touched) {
  check_cuda_i32(row_ptr, "row_ptr");
  const int B = (int)row_ptr.numel() - 1;
  check_ffm_v(V);
  const int nfields = (int)V.size(1);
  const int K = (int)V.size(2);
  lightctr::ffm_backward_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), V.data_ptr<float>(), dpred.data_ptr<float>(),
      gradW.data_ptr<float>(), gradV.data_ptr<float>(),
      (unsigned long long*)touched.data_ptr(), nfields, B, K, cur_stream());
}

void ffm_sorted_backward(at::Tensor sorted_fids, at::Tensor perm,
                         at::Tensor row_of_entry, at::Tensor row_ptr,
                         at::Tensor fields, at::Tensor fids, at::Tensor vals,
                         at::Tensor V, at::Tensor dpred, at::Tensor gradW,
                         at::Tensor gradV, at::Tensor touched) {
  check_cuda_i32(sorted_fids, "sorted_fids");
  auto perm_i = perm32(perm).contiguous();
  check_cuda_i32(row_of_entry, "row_of_entry");
  check_ffm_v(V);
  const int nfields = (int)V.size(1);
  const int K = (int)V.size(2);
  check_ffm_block_lds(nfields, K, "ffm_sorted_backward");
  lightctr::ffm_sorted_backward_launch(
      sorted_fids.data_ptr<int>(), perm_i.data_ptr<int>(),
      row_of_entry.data_ptr<int>(), row_ptr.data_ptr<int>(),
      fields.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      V.data_ptr<float>(), dpred.data_ptr<float>(), gradW.data_ptr<float>(),
      gradV.data_ptr<float>(), (unsigned long long*)touched.data_ptr(),
      nfields, (int)sorted_fids.numel(), K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

std::vector<at::Tensor> ffm_block_emit(at::Tensor row_of_entry,
                                       at::Tensor row_ptr, at::Tensor fields,
                                       at::Tensor fids, at::Tensor vals,
                                       at::Tensor V, at::Tensor dpred) {
  check_cuda_i32(row_of_entry, "row_of_entry");
  check_cuda_f32(V, "V");
  check_ffm_v(V);
  const int nfields = (int)V.size(1);
  const int K = (int)V.size(2);
  check_ffm_block_lds(nfields, K, "ffm_block_emit");
  const auto nnz = fids.numel();
  auto gblocks = at::empty({nnz, (long)nfields * K}, V.options());
  auto gw = at::empty({nnz}, V.options());
  lightctr::ffm_block_emit_launch(
      row_of_entry.data_ptr<int>(), row_ptr.data_ptr<int>(),
      fields.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      V.data_ptr<float>(), dpred.data_ptr<float>(),
      gblocks.data_ptr<float>(), gw.data_ptr<float>(), nfields, (int)nnz, K,
      cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {gw, gblocks};
}

void ffm_blocks_apply(at::Tensor sorted_fids, at::Tensor perm,
                      at::Tensor gblocks, at::Tensor gw, at::Tensor gradW,
                      at::Tensor gradV, at::Tensor touched) {
  check_cuda_i32(sorted_fids, "sorted_fids");
  auto perm_i = perm32(perm).contiguous();
  const int D = (int)gblocks.size(1);
  const long need = lightctr::ffm_blocks_apply_lds_bytes(D);
  const long have = lightctr::ffm_max_lds_per_block();
  CHK(need <= have, "ffm_blocks_apply: D=", D, " needs ", need,
      " bytes of LDS per block, the device gives ", have);
  lightctr::ffm_blocks_apply_launch(
      sorted_fids.data_ptr<int>(), perm_i.data_ptr<int>(),
      gblocks.data_ptr<float>(), gw.data_ptr<float>(),
      gradW.data_ptr<float>(), gradV.data_ptr<float>(),
      (unsigned long long*)touched.data_ptr(), D,
      (int)sorted_fids.numel(), cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

at::Tensor row_index(at::Tensor row_ptr, int64_t nnz) {
  check_cuda_i32(row_ptr, "row_ptr");
  auto out = at::empty({nnz}, row_ptr.options());
  lightctr::row_index_launch(row_ptr.data_ptr<int>(), out.data_ptr<int>(),
                             (int)row_ptr.numel() - 1, cur_stream());
  return out;
}

void ps_apply(at::Tensor lidx, at::Tensor gW, at::Tensor gV, at::Tensor W,
              at::Tensor V, c10::optional<at::Tensor> nW,
              c10::optional<at::Tensor> nV,
              c10::optional<at::Tensor> shadowW,
              c10::optional<at::Tensor> shadowV, int64_t updater, double lr,
              double lam, double eps) {
  CHK(lidx.is_cuda() && lidx.scalar_type() == at::kLong, "lidx i64 GPU");
  CHK(lidx.dim() == 1 && lidx.is_contiguous(),
      "lidx must be 1-D and contiguous");
  CHK(updater >= 0 && updater <= 3, "updater must be 0..3, got ", updater);
  check_cuda_f32(W, "W");
  check_cuda_f32(V, "V");
  check_cuda_f32(gW, "gW");
  check_cuda_f32(gV, "gV");
  CHK(W.dim() == 1, "W must be [F]");
  CHK(V.dim() == 2 && V.size(0) == W.size(0), "V must be [F, K]");
  const long n = lidx.numel();
  const int K = (int)V.size(1);
  CHK(gW.dim() == 1 && gW.size(0) == n, "gW must be [n]");
  CHK(gV.dim() == 2 && gV.size(0) == n && gV.size(1) == K,
      "gV must be [n, K]");
  // every optional state array has the shape of the table it shadows
  auto check_like = [](const c10::optional<at::Tensor>& t,
                       const at::Tensor& ref, const char* name) {
    if (!t.has_value()) return;
    check_cuda_f32(*t, name);
    CHK(t->sizes() == ref.sizes(), name, " shape mismatch");
  };
  check_like(nW, W, "nW");
  check_like(nV, V, "nV");
  check_like(shadowW, W, "shadowW");
  check_like(shadowV, V, "shadowV");
  if (updater == 1 || updater == 3)
    CHK(nW.has_value() && nV.has_value(),
        "adagrad / dcasgda need nW and nV");
  if (updater >= 2)
    CHK(shadowW.has_value() && shadowV.has_value(),
        "dcasgd / dcasgda need shadowW and shadowV");
  if (n == 0) return;
  lightctr::ps_apply_launch(
      lidx.data_ptr<long>(), (int)lidx.numel(), gW.data_ptr<float>(),
      gV.data_ptr<float>(), W.data_ptr<float>(), V.data_ptr<float>(),
      nW.has_value() ? nW->data_ptr<float>() : nullptr,
      nV.has_value() ? nV->data_ptr<float>() : nullptr,
      shadowW.has_value() ? shadowW->data_ptr<float>() : nullptr,
      shadowV.has_value() ? shadowV->data_ptr<float>() : nullptr, K,
      (int)updater, (float)lr, (float)lam, (float)eps, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// ---- PS dense table (flat slab; payload fp32 | fp16 | uint8 codes) ----

int dense_wire(const at::Tensor& payload,
               const c10::optional<at::Tensor>& scale,
               const c10::optional<at::Tensor>& table) {
  CHK(payload.is_cuda() && payload.is_contiguous(),
      "payload must be a contiguous GPU tensor");
  if (payload.scalar_type() == at::kFloat) return 0;
  if (payload.scalar_type() == at::kHalf) return 1;
  CHK(payload.scalar_type() == at::kByte,
      "payload must be fp32, fp16 or uint8 codes");
  CHK(scale.has_value() && table.has_value(),
      "uint8 codes need scale and table");
  check_cuda_f32(*scale, "scale");
  check_cuda_f32(*table, "table");
  CHK(scale->numel() == 1, "scale must have 1 element");
  CHK(table->numel() >= 1 && table->numel() <= 256,
      "table must have 1..256 entries");
  return 2;
}

void check_dense_flags(const at::Tensor& flags) {
  check_cuda_i32(flags, "flags");
  CHK(flags.numel() >= 2, "flags must hold {corrupt, dropped}");
}

void ps_dense_check(at::Tensor payload, c10::optional<at::Tensor> scale,
                    c10::optional<at::Tensor> table, at::Tensor flags) {
  const int wire = dense_wire(payload, scale, table);
  check_dense_flags(flags);
  lightctr::ps_dense_check_launch(
      payload.data_ptr(), wire,
      wire == 2 ? scale->data_ptr<float>() : nullptr,
      wire == 2 ? table->data_ptr<float>() : nullptr,
      wire == 2 ? (int)table->numel() : 0, payload.numel(),
      flags.data_ptr<int>(), cur_stream());
}

void ps_dense_apply(at::Tensor payload, c10::optional<at::Tensor> scale,
                    c10::optional<at::Tensor> table, at::Tensor slab,
                    c10::optional<at::Tensor> acc,
                    c10::optional<at::Tensor> shadow, at::Tensor flags,
                    int64_t updater, double lr, double lam, double eps) {
  const int wire = dense_wire(payload, scale, table);
  check_dense_flags(flags);
  check_cuda_f32(slab, "slab");
  const long n = slab.numel();
  CHK(payload.numel() == n, "payload and slab sizes differ");
  CHK(updater >= 0 && updater <= 3, "updater must be 0..3");
  const bool need_acc = updater == 1 || updater == 3;
  const bool need_sh = updater == 2 || updater == 3;
  CHK(acc.has_value() == need_acc, "acc is for adagrad/dcasgda only");
  CHK(shadow.has_value() == need_sh, "shadow is for dcasgd/dcasgda only");
  if (need_acc) {
    check_cuda_f32(*acc, "acc");
    CHK(acc->numel() == n, "acc and slab sizes differ");
  }
  if (need_sh) {
    check_cuda_f32(*shadow, "shadow");
    CHK(shadow->numel() == n, "shadow and slab sizes differ");
  }
  lightctr::ps_dense_apply_launch(
      payload.data_ptr(), wire,
      wire == 2 ? scale->data_ptr<float>() : nullptr,
      wire == 2 ? table->data_ptr<float>() : nullptr,
      wire == 2 ? (int)table->numel() : 0, slab.data_ptr<float>(),
      need_acc ? acc->data_ptr<float>() : nullptr,
      need_sh ? shadow->data_ptr<float>() : nullptr, n, (int)updater,
      (float)lr, (float)lam, (float)eps, flags.data_ptr<int>(),
      cur_stream());
}

at::Tensor ps_dense_pack(at::Tensor slab, c10::optional<at::Tensor> shadow,
                         bool fp16) {
  check_cuda_f32(slab, "slab");
  const long n = slab.numel();
  if (shadow) {
    check_cuda_f32(*shadow, "shadow");
    CHK(shadow->numel() == n, "shadow and slab sizes differ");
  }
  auto out = at::empty({n}, slab.options().dtype(fp16 ? at::kHalf
                                                      : at::kFloat));
  lightctr::ps_dense_pack_launch(
      slab.data_ptr<float>(), out.data_ptr(), fp16 ? 1 : 0,
      shadow ? shadow->data_ptr<float>() : nullptr, n, cur_stream());
  return out;
}

// ---- generic sparse optimizers (D = latent block width, runtime) ----

void sparse_adagrad_apply(at::Tensor uniq, at::Tensor count, at::Tensor W,
                          at::Tensor V, at::Tensor nW, at::Tensor nV,
                          at::Tensor gradW, at::Tensor gradV, double lr,
                          double eps, double l2,
                          c10::optional<at::Tensor> Vh) {
  check_cuda_i32(uniq, "uniq");
  const int D = (int)(V.numel() / V.size(0));
  if (Vh) CHK(Vh->scalar_type() == at::kBFloat16, "Vh mirror must be bf16");
  lightctr::sparse_adagrad_apply_launch(
      uniq.data_ptr<int>(), count.data_ptr<int>(), W.data_ptr<float>(),
      V.data_ptr<float>(), nW.data_ptr<float>(), nV.data_ptr<float>(),
      gradW.data_ptr<float>(), gradV.data_ptr<float>(), (float)lr, (float)eps,
      (float)l2, (int)uniq.numel(), D,
      Vh ? Vh->data_ptr() : nullptr, cur_stream());
}

void sparse_ftrl_apply(at::Tensor uniq, at::Tensor count, at::Tensor W,
                       at::Tensor V, at::Tensor zW, at::Tensor nW,
                       at::Tensor zV, at::Tensor nV, at::Tensor gradW,
                       at::Tensor gradV, double alpha, double beta, double l1,
                       double l2, int64_t v_adagrad, double v_lr,
                       double v_eps, double v_l2,
                       c10::optional<at::Tensor> Vh) {
  check_cuda_i32(uniq, "uniq");
  const int D = (int)(V.numel() / V.size(0));
  if (Vh) CHK(Vh->scalar_type() == at::kBFloat16, "Vh mirror must be bf16");
  lightctr::sparse_ftrl_apply_launch(
      uniq.data_ptr<int>(), count.data_ptr<int>(), W.data_ptr<float>(),
      V.data_ptr<float>(), zW.data_ptr<float>(), nW.data_ptr<float>(),
      zV.data_ptr<float>(), nV.data_ptr<float>(), gradW.data_ptr<float>(),
      gradV.data_ptr<float>(), (float)alpha, (float)beta, (float)l1,
      (float)l2, (int)uniq.numel(), D, (int)v_adagrad, (float)v_lr,
      (float)v_eps, (float)v_l2, Vh ? Vh->data_ptr() : nullptr,
      cur_stream());
}

at::Tensor gemm_wgrad_bf16(at::Tensor At, at::Tensor Bt, int64_t M,
                           int64_t N, int64_t K) {
  CHK(At.is_cuda() && At.scalar_type() == at::kBFloat16 &&
          At.is_contiguous(), "At must be cuda bf16 [K,M]");
  CHK(Bt.is_cuda() && Bt.scalar_type() == at::kBFloat16 &&
          Bt.is_contiguous(), "Bt must be cuda bf16 [K,N]");
  const int64_t imax = std::numeric_limits<int>::max();
  CHK(M >= 1 && N >= 1 && K >= 1 && M <= imax && N <= imax && K <= imax,
      "gemm_wgrad: M, N, K must be in [1, 2^31)");
  CHK(At.numel() == K * M, "At must hold K*M = ", K * M, " elements, has ",
      At.numel());
  CHK(Bt.numel() == K * N, "Bt must hold K*N = ", K * N, " elements, has ",
      Bt.numel());
  CHK(lightctr::gemm_wgrad_eligible((int)M, (int)N, (int)K, 1, 1),
      "shape not eligible for the wgrad kernel");
  CHK((((uintptr_t)At.data_ptr() | (uintptr_t)Bt.data_ptr()) & 15) == 0,
      "the wgrad kernel needs 16-byte-aligned operand base addresses");
  auto C = at::empty({M, N}, At.options().dtype(at::kFloat));
  lightctr::gemm_wgrad_bf16_launch(At.data_ptr(), Bt.data_ptr(),
                                   C.data_ptr<float>(), (int)M, (int)N,
                                   (int)K, cur_stream());
  return C;
}

std::vector<at::Tensor> wg_probe(at::Tensor g, int64_t ld, int64_t mode) {
  CHK(g.is_cuda() && g.scalar_type() == at::kBFloat16, "g bf16");
  auto out_lds = at::zeros({64 * 128}, g.options());
  auto out_frag = at::zeros({2 * 2 * 64 * 8}, g.options().dtype(at::kFloat));
  lightctr::wg_probe_launch(g.data_ptr(), (int)ld, out_lds.data_ptr(),
                            out_frag.data_ptr<float>(), (int)mode,
                            cur_stream());
  return {out_lds, out_frag};
}

// output extent of a k x k window at the given stride and padding; a
// geometry with no output position is an error, not an empty launch
void conv_out_shape(int64_t H, int64_t W, int64_t k, int64_t stride,
                    int64_t pad, int* OH, int* OW) {
  CHK(k >= 1 && stride >= 1, "conv: k and stride must be >= 1, got k=", k,
      " stride=", stride);
  CHK(pad >= 0, "conv: pad must be >= 0, got ", pad);
  CHK(H + 2 * pad >= k && W + 2 * pad >= k, "conv: a ", k, "x", k,
      " window does not fit a ", H, "x", W, " image with pad ", pad);
  *OH = (int)((H + 2 * pad - k) / stride + 1);
  *OW = (int)((W + 2 * pad - k) / stride + 1);
}

at::Tensor im2col_bf16(at::Tensor x, int64_t k, int64_t stride,
                       int64_t pad) {
  check_cuda_f32(x, "x");
  CHK(x.dim() == 4, "x must be [B,C,H,W]");
  const int B = (int)x.size(0), C = (int)x.size(1), H = (int)x.size(2),
            W = (int)x.size(3);
  int OH, OW;
  conv_out_shape(H, W, k, stride, pad, &OH, &OW);
  auto col = at::empty({(long)B * OH * OW, (long)C * k * k},
                       x.options().dtype(at::kBFloat16));
  if (col.numel() == 0) return col;
  lightctr::im2col_bf16_launch(x.data_ptr<float>(), col.data_ptr(), B, C, H,
                               W, (int)k, (int)stride, (int)pad, OH, OW,
                               cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return col;
}

at::Tensor col2im(at::Tensor dcol, int64_t B, int64_t C, int64_t H,
                  int64_t W, int64_t k, int64_t stride, int64_t pad) {
  check_cuda_f32(dcol, "dcol");
  CHK(B >= 0 && C >= 0 && H >= 1 && W >= 1, "col2im: bad image shape");
  int OH, OW;
  conv_out_shape(H, W, k, stride, pad, &OH, &OW);
  CHK(dcol.dim() == 2 && dcol.size(0) == (long)B * OH * OW &&
          dcol.size(1) == C * k * k,
      "dcol shape mismatch");
  auto dx = at::empty({B, C, H, W}, dcol.options());
  if (dx.numel() == 0) return dx;
  lightctr::col2im_launch(dcol.data_ptr<float>(), dx.data_ptr<float>(),
                          (int)B, (int)C, (int)H, (int)W, (int)k,
                          (int)stride, (int)pad, OH, OW, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return dx;
}

void auc_hist_add(at::Tensor pred, at::Tensor label, at::Tensor hist) {
  check_cuda_f32(pred, "pred");
  check_cuda_f32(label, "label");
  CHK(hist.is_cuda() && hist.scalar_type() == at::kInt &&
          hist.is_contiguous(),
      "hist must be cuda int32 [2*buckets]");
  CHK(hist.numel() >= 2 && hist.numel() % 2 == 0,
      "hist must hold 2*buckets counts, buckets >= 1");
  CHK(label.numel() == pred.numel(), "pred and label lengths differ");
  const int buckets = (int)(hist.numel() / 2);
  if (pred.numel() == 0) return;
  lightctr::auc_hist_add_launch(pred.data_ptr<float>(),
                                label.data_ptr<float>(),
                                (long)pred.numel(),
                                (unsigned int*)hist.data_ptr(), buckets,
                                cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

at::Tensor auc_scan(at::Tensor hist) {
  CHK(hist.is_cuda() && hist.scalar_type() == at::kInt &&
          hist.is_contiguous(),
      "hist must be cuda int32 [2*buckets]");
  CHK(hist.numel() >= 2 && hist.numel() % 2 == 0,
      "hist must hold 2*buckets counts, buckets >= 1");
  const int buckets = (int)(hist.numel() / 2);
  auto out = at::zeros({3}, hist.options().dtype(at::kDouble));
  lightctr::auc_scan_launch((const unsigned int*)hist.data_ptr(), buckets,
                            out.data_ptr<double>(), cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out;  // {correct-pair mass, P, N}
}

at::Tensor bitmap_compact(at::Tensor bitmap, at::Tensor out_fids,
                          at::Tensor out_count) {
  CHK(bitmap.is_cuda() && bitmap.is_contiguous(), "bitmap");
  CHK(bitmap.scalar_type() == at::kLong,
      "bitmap must be int64 (one 64-feature word per element)");
  check_cuda_i32(out_fids, "out_fids");
  check_cuda_i32(out_count, "out_count");
  CHK(out_count.numel() >= 1, "out_count must hold the counter");
  if (bitmap.numel() == 0) return out_count;
  lightctr::bitmap_compact_launch((unsigned long long*)bitmap.data_ptr(),
                                  (int)bitmap.numel(),
                                  out_fids.data_ptr<int>(),
                                  out_count.data_ptr<int>(),
                                  (int)out_fids.numel(), cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out_count;
}

void fm_adagrad_apply(at::Tensor uniq, at::Tensor count, at::Tensor W,
                      at::Tensor V, at::Tensor nW, at::Tensor nV,
                      at::Tensor gradW, at::Tensor gradV, double lr,
                      double eps, double l2) {
  check_cuda_i32(uniq, "uniq");
  check_cuda_i32(count, "count");
  CHK(count.numel() >= 1, "count must hold one int");
  const int K = check_fm_v(V);
  const int64_t F = V.size(0);
  check_f32_n(W, F, "W");
  check_f32_n(nW, F, "nW");
  check_f32_n(nV, F * K, "nV");
  check_f32_n(gradW, F, "gradW");
  check_f32_n(gradV, F * K, "gradV");
  if (uniq.numel() == 0) return;  // a grid of 0 blocks is a launch error
  lightctr::fm_adagrad_apply_launch(
      uniq.data_ptr<int>(), count.data_ptr<int>(), W.data_ptr<float>(),
      V.data_ptr<float>(), nW.data_ptr<float>(), nV.data_ptr<float>(),
      gradW.data_ptr<float>(), gradV.data_ptr<float>(), (float)lr, (float)eps,
      (float)l2, (int)uniq.numel(), K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

void fm_ftrl_apply(at::Tensor uniq, at::Tensor count, at::Tensor W,
                   at::Tensor V, at::Tensor zW, at::Tensor nW,
                   c10::optional<at::Tensor> zV, at::Tensor nV, at::Tensor gradW, at::Tensor gradV,
                   double alpha, double beta, double l1, double l2,
                   int64_t v_adagrad, double v_lr, double v_eps,
                   double v_l2) {
  check_cuda_i32(uniq, "uniq");
  check_cuda_i32(count, "count");
  CHK(count.numel() >= 1, "count must hold one int");
  const int K = check_fm_v(V);
  const int64_t F = V.size(0);
  check_f32_n(W, F, "W");
  check_f32_n(zW, F, "zW");
  check_f32_n(nW, F, "nW");
  check_f32_n(nV, F * K, "nV");
  check_f32_n(gradW, F, "gradW");
  check_f32_n(gradV, F * K, "gradV");
  float* zV_ptr = nullptr;  // Adagrad on V keeps no z
  if (zV.has_value()) {
    check_f32_n(*zV, F * K, "zV");
    zV_ptr = zV->data_ptr<float>();
  }
  CHK(v_adagrad != 0 || zV_ptr != nullptr, "FTRL on V needs zV");
  if (uniq.numel() == 0) return;  // a grid of 0 blocks is a launch error
  lightctr::fm_ftrl_apply_launch(
      uniq.data_ptr<int>(), count.data_ptr<int>(), W.data_ptr<float>(),
      V.data_ptr<float>(), zW.data_ptr<float>(), nW.data_ptr<float>(),
      zV_ptr, nV.data_ptr<float>(), gradW.data_ptr<float>(),
      gradV.data_ptr<float>(), (float)alpha, (float)beta, (float)l1,
      (float)l2, (int)uniq.numel(), K, (int)v_adagrad, (float)v_lr,
      (float)v_eps, (float)v_l2, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
}

// ---- dense NN ops ----

// The GEMM kernels index their operands from M, N, K alone; everything
// they assume about the tensors is checked here, as exceptions. Returns
// the bias pointer (nullptr without bias).
const float* check_gemm_args(const at::Tensor& A, const at::Tensor& Bst,
                             const c10::optional<at::Tensor>& bias,
                             int64_t M, int64_t N, int64_t K,
                             int64_t transA, int64_t transB, int64_t act) {
  const int64_t imax = std::numeric_limits<int>::max();
  CHK(M >= 1 && N >= 1 && K >= 1, "gemm: M, N, K must be >= 1, got ", M,
      ", ", N, ", ", K);
  CHK(M <= imax && N <= imax && K <= imax, "gemm: M, N, K must fit int32");
  CHK(transA == 0 || transA == 1, "gemm: transA must be 0 or 1, got ",
      transA);
  CHK(transB == 0 || transB == 1, "gemm: transB must be 0 or 1, got ",
      transB);
  CHK(act >= 0 && act <= 2, "gemm: act must be 0, 1 or 2, got ", act);
  CHK(A.is_cuda() && A.scalar_type() == at::kBFloat16, "A must be bf16 GPU");
  CHK(Bst.is_cuda() && Bst.scalar_type() == at::kBFloat16,
      "Bst must be bf16 GPU");
  CHK(A.is_contiguous(), "A must be contiguous");
  CHK(Bst.is_contiguous(), "Bst must be contiguous");
  CHK(A.numel() == M * K, "A must hold M*K = ", M * K, " elements, has ",
      A.numel());
  CHK(Bst.numel() == N * K, "Bst must hold N*K = ", N * K,
      " elements, has ", Bst.numel());
  if (!bias.has_value()) return nullptr;
  check_cuda_f32(*bias, "bias");
  CHK(bias->numel() == N, "bias must hold N = ", N, " elements, has ",
      bias->numel());
  return bias->data_ptr<float>();
}

bool gemm_aligned16(const at::Tensor& A, const at::Tensor& Bst) {
  return (((uintptr_t)A.data_ptr() | (uintptr_t)Bst.data_ptr()) & 15) == 0;
}

std::string gemm_route_name(const lightctr::GemmRoute& r) {
  switch (r.body) {
    case lightctr::GEMM_BODY_GENERIC:
      return "generic:split=" + std::to_string(r.split_z);
    case lightctr::GEMM_BODY_256:
      return "gemm256_p" + std::to_string(r.pipe) + "_b" +
             std::to_string((int)r.burst);
    case lightctr::GEMM_BODY_P8:
      return std::string(r.lite ? "p8_lite" : "p8_full") +
             (r.xcd ? "_xcd" : "") + (r.apipe ? "_apipe" : "");
    case lightctr::GEMM_BODY_V2: return "v2";
    case lightctr::GEMM_BODY_N128: return "n128";
    case lightctr::GEMM_BODY_WGRAD128:
      return "wgrad128:split=" + std::to_string(r.split_z);
    case lightctr::GEMM_BODY_GEMV_N1: return "gemv_n1";
    case lightctr::GEMM_BODY_WROWSUM_M1: return "wrowsum_m1";
    case lightctr::GEMM_BODY_SMALL_WGRAD: return "small_wgrad";
    case lightctr::GEMM_BODY_OUTER_K1: return "outer_k1";
  }
  return "unknown";
}

// Name of the body the default dispatch picks in this process for
// 16 B-aligned operands; "generic" and "wgrad128" carry the split-K
// fan-out they would request (":split=0" = none).
std::string gemm_bf16_route(int64_t M, int64_t N, int64_t K, int64_t transA,
                            int64_t transB, bool has_bias, int64_t act,
                            bool emit_bf16) {
  const int64_t imax = std::numeric_limits<int>::max();
  CHK(M >= 1 && N >= 1 && K >= 1 && M <= imax && N <= imax && K <= imax,
      "gemm: M, N, K must be in [1, 2^31)");
  CHK((transA == 0 || transA == 1) && (transB == 0 || transB == 1),
      "gemm: transA, transB must be 0 or 1");
  CHK(act >= 0 && act <= 2, "gemm: act must be 0, 1 or 2, got ", act);
  return gemm_route_name(lightctr::gemm_bf16_pick(
      (int)M, (int)N, (int)K, (int)transA, (int)transB, has_bias, (int)act,
      emit_bf16, true));
}

// Launch one named GEMM body directly, whatever the default dispatch or
// the environment would pick. Raises unless the body accepts the shape,
// layout, epilogue and operand alignment.
std::vector<at::Tensor> gemm_bf16_variant(
    at::Tensor A, at::Tensor Bst, c10::optional<at::Tensor> bias, int64_t M,
    int64_t N, int64_t K, int64_t transA, int64_t transB, int64_t act,
    bool emit_bf16, std::string variant, int64_t split_z) {
  const float* bias_ptr =
      check_gemm_args(A, Bst, bias, M, N, K, transA, transB, act);
  const int m = (int)M, n = (int)N, k = (int)K, ta = (int)transA,
            tb = (int)transB;
  const bool plain = bias_ptr == nullptr && act == 0 && !emit_bf16;
  const bool aligned = gemm_aligned16(A, Bst);
  CHK(split_z >= 0 && split_z <= 1024, "split_z must be in [0, 1024], got ",
      split_z);
  lightctr::GemmRoute r;
  r.split_z = (int)split_z;
  bool splits = false;  // body has a split-K form
  bool ok = false;      // body accepts shape and layout
  bool glds = true;     // body needs 16 B-aligned operand bases
  if (variant == "generic") {
    r.body = lightctr::GEMM_BODY_GENERIC;
    splits = ok = true;
    glds = false;
  } else if (variant.rfind("gemm256_p", 0) == 0 && variant.size() == 13 &&
             variant.compare(10, 2, "_b") == 0) {
    r.body = lightctr::GEMM_BODY_256;
    r.pipe = variant[9] - '0';
    const int burst = variant[12] - '0';
    CHK(r.pipe >= 0 && r.pipe <= 2 && (burst == 0 || burst == 1),
        "unknown GEMM variant '", variant, "'");
    r.burst = burst == 1;
    ok = lightctr::gemm256_eligible(m, n, k, ta, tb);
    CHK(!(r.pipe == 2 && K % 64 != 0),
        "gemm256 pipe 2 takes K % 64 == 0 only, got K = ", K);
  } else if (variant == "p8_lite" || variant == "p8_lite_xcd" ||
             variant == "p8_full" || variant == "p8_full_xcd" ||
             variant == "p8_lite_apipe") {
    r.body = lightctr::GEMM_BODY_P8;
    r.lite = variant.compare(3, 4, "lite") == 0;
    r.xcd = variant.find("_xcd") != std::string::npos;
    r.apipe = variant.find("_apipe") != std::string::npos;
    ok = lightctr::gemm256p8_eligible(m, n, k, ta, tb);
  } else if (variant == "v2") {
    r.body = lightctr::GEMM_BODY_V2;
    ok = lightctr::gemm256v2_eligible(m, n, k, ta, tb);
  } else if (variant == "n128") {
    // the kernel itself takes any N and any K that is a whole number of
    // tiles; the default dispatch narrows that further
    r.body = lightctr::GEMM_BODY_N128;
    ok = ta == 0 && tb == 0 && M % 256 == 0 && K % 64 == 0;
  } else if (variant == "wgrad128") {
    r.body = lightctr::GEMM_BODY_WGRAD128;
    splits = true;
    ok = lightctr::gemm_wgrad_eligible(m, n, k, ta, tb);
    CHK(plain, "wgrad128 has no bias / activation / bf16 epilogue");
  } else {
    CHK(false, "unknown GEMM variant '", variant, "'");
  }
  CHK(ok, "GEMM variant '", variant, "' does not accept M=", M, " N=", N,
      " K=", K, " transA=", transA, " transB=", transB);
  CHK(!glds || aligned, "GEMM variant '", variant,
      "' needs 16-byte-aligned operand base addresses");
  CHK(splits || split_z == 0, "GEMM variant '", variant,
      "' has no split-K form");
  CHK(split_z == 0 || plain,
      "split-K has no bias / activation / bf16 epilogue");
  auto C = at::empty({M, N}, A.options().dtype(at::kFloat));
  at::Tensor Cbf;
  void* cbf_ptr = nullptr;
  if (emit_bf16) {
    Cbf = at::empty({M, N}, A.options());
    cbf_ptr = Cbf.data_ptr();
  }
  lightctr::gemm_bf16_run(r, A.data_ptr(), Bst.data_ptr(), bias_ptr,
                          C.data_ptr<float>(), cbf_ptr, m, n, k, ta, tb,
                          (int)act, cur_stream());
  if (emit_bf16) return {C, Cbf};
  return {C};
}

at::Tensor gemm_bf16(at::Tensor A, at::Tensor Bst,
                     c10::optional<at::Tensor> bias, int64_t M, int64_t N,
                     int64_t K, int64_t transA, int64_t transB, int64_t act,
                     bool emit_bf16) {
  const float* bias_ptr =
      check_gemm_args(A, Bst, bias, M, N, K, transA, transB, act);
  auto C = at::empty({M, N}, A.options().dtype(at::kFloat));
  at::Tensor Cbf;
  void* cbf_ptr = nullptr;
  if (emit_bf16) {
    Cbf = at::empty({M, N}, A.options());
    cbf_ptr = Cbf.data_ptr();
  }
  lightctr::gemm_bf16_launch(A.data_ptr(), Bst.data_ptr(), bias_ptr,
                             C.data_ptr<float>(), cbf_ptr, (int)M, (int)N,
                             (int)K, (int)transA, (int)transB, (int)act,
                             cur_stream());
  return C;
}

std::vector<at::Tensor> gemm_bf16_full(at::Tensor A, at::Tensor Bst,
                                       c10::optional<at::Tensor> bias,
                                       int64_t M, int64_t N, int64_t K,
                                       int64_t transA, int64_t transB,
                                       int64_t act) {
  const float* bias_ptr =
      check_gemm_args(A, Bst, bias, M, N, K, transA, transB, act);
  auto C = at::empty({M, N}, A.options().dtype(at::kFloat));
  auto Cbf = at::empty({M, N}, A.options());
  lightctr::gemm_bf16_launch(A.data_ptr(), Bst.data_ptr(), bias_ptr,
                             C.data_ptr<float>(), Cbf.data_ptr(), (int)M,
                             (int)N, (int)K, (int)transA, (int)transB,
                             (int)act, cur_stream());
  return {C, Cbf};
}

std::vector<at::Tensor> act_backward(at::Tensor dY, at::Tensor Y,
                                     int64_t act) {
  check_cuda_f32(dY, "dY");
  auto dZ = at::empty_like(dY);
  auto dZbf = at::empty_like(dY, dY.options().dtype(at::kBFloat16));
  lightctr::act_backward_launch(dY.data_ptr<float>(), Y.data_ptr<float>(),
                                dZ.data_ptr<float>(), dZbf.data_ptr(),
                                dY.numel(), (int)act, cur_stream());
  return {dZ, dZbf};
}

// Bit-range radix sort: drop-in for `torch.sort(fids)` on nonnegative
// int32 keys < 2^end_bit. Returns (sorted_keys int32, perm int64).
std::vector<at::Tensor> radix_sort_index(at::Tensor keys, int64_t end_bit) {
  check_cuda_i32(keys, "keys");
  CHK(end_bit >= 1 && end_bit <= 32, "end_bit in [1,32]");
  const int n = (int)keys.numel();
  auto sorted = at::empty_like(keys);
  auto perm = at::empty({n}, keys.options());
  auto iota = at::empty({n}, keys.options());
  lightctr::iota_i32_launch(iota.data_ptr<int>(), n, cur_stream());
  const unsigned long bytes =
      lightctr::radix_sort_pairs_i32_temp_bytes(n, (int)end_bit);
  auto temp = at::empty({(long)bytes}, keys.options().dtype(at::kByte));
  lightctr::radix_sort_pairs_i32_launch(
      temp.data_ptr(), bytes, keys.data_ptr<int>(), sorted.data_ptr<int>(),
      iota.data_ptr<int>(), perm.data_ptr<int>(), n, (int)end_bit,
      cur_stream());
  return {sorted, perm};
}

// The same sort carrying an 8-byte record per key ([n, 2] int32) instead of
// an index: returns (sorted_keys int32, sorted_rec [n, 2] int32). No iota
// buffer, no permutation.
std::vector<at::Tensor> radix_sort_rec(at::Tensor keys, at::Tensor rec,
                                       int64_t end_bit) {
  check_cuda_i32(keys, "keys");
  CHK(end_bit >= 1 && end_bit <= 32, "end_bit in [1,32]");
  const int n = (int)keys.numel();
  check_cuda_rec(rec, n, "rec");
  auto sorted = at::empty_like(keys);
  auto sorted_rec = at::empty_like(rec);
  if (n == 0) return {sorted, sorted_rec};
  const unsigned long bytes =
      lightctr::radix_sort_pairs_rec_temp_bytes(n, (int)end_bit);
  auto temp = at::empty({(long)bytes}, keys.options().dtype(at::kByte));
  lightctr::radix_sort_pairs_rec_launch(
      temp.data_ptr(), bytes, keys.data_ptr<int>(), sorted.data_ptr<int>(),
      rec.data_ptr<int>(), sorted_rec.data_ptr<int>(), n, (int)end_bit,
      cur_stream());
  return {sorted, sorted_rec};
}

// The same result from the single-purpose onesweep sort (sort_kernels.hip):
// five launches for three passes. status: int32 [1] owned by the caller; the
// sort ORs a nonzero code into it if a look-back spin gives up and never
// zeroes it.
std::vector<at::Tensor> onesweep_sort_rec(at::Tensor keys, at::Tensor rec,
                                          int64_t end_bit,
                                          c10::optional<at::Tensor> status) {
  check_cuda_i32(keys, "keys");
  CHK(end_bit >= 1 && end_bit <= 31, "end_bit in [1,31]");
  CHK(keys.numel() < (1L << 30), "n must be below 2^30");
  const int n = (int)keys.numel();
  check_cuda_rec(rec, n, "rec");
  if (status.has_value()) {
    check_cuda_i32(*status, "status");
    CHK(status->numel() >= 1, "status must hold one word");
  }
  auto sorted = at::empty_like(keys);
  auto sorted_rec = at::empty_like(rec);
  if (n == 0) return {sorted, sorted_rec};
  auto st = status.has_value() ? *status : at::zeros({1}, keys.options());
  const unsigned long bytes =
      lightctr::onesweep_sort_work_bytes(n, (int)end_bit);
  auto work = at::empty({(long)bytes}, keys.options().dtype(at::kByte));
  at::Tensor keys_tmp, rec_tmp;
  if (end_bit > 8) {
    keys_tmp = at::empty_like(keys);
    rec_tmp = at::empty_like(rec);
  }
  lightctr::onesweep_sort_rec_launch(
      work.data_ptr(), keys.data_ptr<int>(), sorted.data_ptr<int>(),
      end_bit > 8 ? keys_tmp.data_ptr<int>() : nullptr, rec.data_ptr<int>(),
      sorted_rec.data_ptr<int>(),
      end_bit > 8 ? rec_tmp.data_ptr<int>() : nullptr, n, (int)end_bit,
      st.data_ptr<int>(), cur_stream());
  return {sorted, sorted_rec};
}

// The records of a CSR batch on their own: rec[j] = {row of j, bits of
// vals[j]}, what fm_forward_train returns as its fourth output.
at::Tensor fm_records(at::Tensor row_ptr, at::Tensor vals) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_f32(vals, "vals");
  CHK(row_ptr.numel() >= 1, "row_ptr must hold B + 1 offsets");
  const int B = (int)row_ptr.numel() - 1;
  auto rec = at::empty({vals.numel(), 2}, row_ptr.options());
  if (vals.numel() == 0) return rec;
  lightctr::fm_records_launch(row_ptr.data_ptr<int>(), vals.data_ptr<float>(),
                              rec.data_ptr<int>(), B, cur_stream());
  return rec;
}

// what the onesweep sort of a CSR batch accepts, and its buffers
struct CsrSortBuffers {
  at::Tensor sorted, sorted_rec, work, keys_tmp, rec_tmp, status;
};

void check_csr_sort(const at::Tensor& row_ptr, const at::Tensor& fids,
                    const at::Tensor& vals, int64_t end_bit,
                    const c10::optional<at::Tensor>& status) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_i32(fids, "fids");
  check_cuda_f32(vals, "vals");
  CHK(row_ptr.numel() >= 1, "row_ptr must hold B + 1 offsets");
  CHK(vals.numel() == fids.numel(), "vals must have one value per entry");
  CHK(end_bit >= 1 && end_bit <= 31, "end_bit in [1,31]");
  CHK(fids.numel() < (1L << 30), "n must be below 2^30");
  if (status.has_value()) {
    check_cuda_i32(*status, "status");
    CHK(status->numel() >= 1, "status must hold one word");
  }
}

// every allocation of the sort, on the current stream
CsrSortBuffers alloc_csr_sort(const at::Tensor& fids, int64_t end_bit,
                              const c10::optional<at::Tensor>& status) {
  CsrSortBuffers b;
  const long n = fids.numel();
  b.sorted = at::empty_like(fids);
  b.sorted_rec = at::empty({n, 2}, fids.options());
  if (n == 0) return b;
  b.status = status.has_value() ? *status : at::zeros({1}, fids.options());
  const unsigned long bytes =
      lightctr::onesweep_sort_work_bytes((int)n, (int)end_bit);
  b.work = at::empty({(long)bytes}, fids.options().dtype(at::kByte));
  if (end_bit > 8) {  // the ping-pong pair, from two passes on
    b.keys_tmp = at::empty_like(fids);
    b.rec_tmp = at::empty({n, 2}, fids.options());
  }
  return b;
}

void launch_csr_sort(const CsrSortBuffers& b, const at::Tensor& row_ptr,
                     const at::Tensor& fids, const at::Tensor& vals,
                     int64_t end_bit, ihipStream_t* stream) {
  lightctr::onesweep_sort_csr_launch(
      b.work.data_ptr(), row_ptr.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), (int)row_ptr.numel() - 1,
      b.sorted.data_ptr<int>(),
      end_bit > 8 ? b.keys_tmp.data_ptr<int>() : nullptr,
      b.sorted_rec.data_ptr<int>(),
      end_bit > 8 ? b.rec_tmp.data_ptr<int>() : nullptr, (int)fids.numel(),
      (int)end_bit, b.status.data_ptr<int>(), stream);
}

// onesweep_sort_rec(fids, fm_records(row_ptr, vals)) without the records'
// own launch and without the records in CSR order: the first scatter pass
// reads fids and vals and finds each entry's row in row_ptr itself.
std::vector<at::Tensor> onesweep_sort_csr(at::Tensor row_ptr, at::Tensor fids,
                                          at::Tensor vals, int64_t end_bit,
                                          c10::optional<at::Tensor> status) {
  check_csr_sort(row_ptr, fids, vals, end_bit, status);
  auto b = alloc_csr_sort(fids, end_bit, status);
  if (fids.numel() > 0 && row_ptr.numel() > 1)
    launch_csr_sort(b, row_ptr, fids, vals, end_bit, cur_stream());
  return {b.sorted, b.sorted_rec};
}

// Front half of the segment-mode training step: the training forward (no
// records) and the record sort of the batch (keys-only histogram; the first
// scatter pass reads fids and vals and finds the rows, so no record is written
// in batch order). The sort reads only the batch,
// so with overlap it runs on a pool stream beside the forward: fork by an
// event on the current stream, join by an event on the pool stream, no sync
// and no host read, so a stream capture records the two as parallel branches
// that meet in front of whatever the caller enqueues next. Everything is
// allocated on the current stream before the fork, and the join orders every
// use of the temporaries before their blocks can be handed out again.
// Both branches are kernels only (the CSR sort zeroes its control block with
// a kernel, not a memset). The sort branch is enqueued first and the pool
// stream has the default priority (profiles/r7_01_fm_overlap.txt).
// overlap=false: the same launches in sequence on the current stream.
// Returns (loss, dpred, sumVX, sorted_fids, sorted_rec).
std::vector<at::Tensor> fm_forward_train_sorted(
    at::Tensor row_ptr, at::Tensor fids, at::Tensor vals, at::Tensor W,
    at::Tensor V, at::Tensor label, double scale, int64_t end_bit,
    c10::optional<at::Tensor> reset, c10::optional<at::Tensor> status,
    bool overlap) {
  check_csr_sort(row_ptr, fids, vals, end_bit, status);
  const int K = check_fm_v(V);
  check_f32_n(W, V.size(0), "W");
  check_cuda_f32(label, "label");
  const int B = (int)row_ptr.numel() - 1;
  const long nnz = fids.numel();
  CHK(label.numel() == B, "label must have one value per row");
  int* reset_ptr = nullptr;
  if (reset.has_value()) {
    check_cuda_i32(*reset, "reset");
    CHK(reset->numel() >= 1, "reset must hold one int");
    reset_ptr = reset->data_ptr<int>();
    if (B <= 0) reset->zero_();  // nothing is launched for an empty batch
  }
  auto loss = at::empty({B}, W.options());
  auto dpred = at::empty({B}, W.options());
  auto sumVX = at::empty({B, K}, W.options());
  auto b = alloc_csr_sort(fids, end_bit, status);
  if (B <= 0) return {loss, dpred, sumVX, b.sorted, b.sorted_rec};
  const auto forward = [&](ihipStream_t* stream) {
    lightctr::fm_forward_train_launch(
        row_ptr.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
        W.data_ptr<float>(), V.data_ptr<float>(), label.data_ptr<float>(),
        (float)scale, loss.data_ptr<float>(), dpred.data_ptr<float>(),
        sumVX.data_ptr<float>(), nullptr, B, K, reset_ptr, stream);
  };
  if (nnz == 0) {  // rows without entries: a loss, nothing to sort
    forward(cur_stream());
  } else if (!overlap) {
    forward(cur_stream());
    launch_csr_sort(b, row_ptr, fids, vals, end_bit, cur_stream());
  } else {
    const auto main = at::cuda::getCurrentCUDAStream();
    const auto side =
        at::cuda::getStreamFromPool(false, main.device_index());
    at::cuda::CUDAEvent fork, join;
    fork.record(main);
    fork.block(side);
    launch_csr_sort(b, row_ptr, fids, vals, end_bit,
                    (ihipStream_t*)side.stream());
    forward((ihipStream_t*)main.stream());
    join.record(side);
    join.block(main);
  }
  return {loss, dpred, sumVX, b.sorted, b.sorted_rec};
}


at::Tensor colsum(at::Tensor dZ) {
  check_cuda_f32(dZ, "dZ");
  const int M = (int)dZ.size(0), N = (int)dZ.size(1);
  auto db = at::empty({N}, dZ.options());
  lightctr::colsum_launch(dZ.data_ptr<float>(), db.data_ptr<float>(), M, N,
                          cur_stream());
  return db;
}

at::Tensor to_bf16(at::Tensor x) {
  check_cuda_f32(x, "x");
  auto y = at::empty_like(x, x.options().dtype(at::kBFloat16));
  lightctr::to_bf16_launch(x.data_ptr<float>(), y.data_ptr(), x.numel(),
                           cur_stream());
  return y;
}

void dense_adam(at::Tensor W, at::Tensor grad, at::Tensor m, at::Tensor v,
                c10::optional<at::Tensor> Wbf, c10::optional<at::Tensor> Wtbf,
                double lr, double beta1, double beta2, double eps,
                int64_t step, double l2) {
  check_cuda_f32(W, "W");
  const int rows = (int)W.size(0);
  const int cols = (int)(W.numel() / W.size(0));
  const float bc1 = 1.f - powf((float)beta1, (float)step);
  const float bc2 = 1.f - powf((float)beta2, (float)step);
  lightctr::dense_adam_launch(
      W.data_ptr<float>(), grad.data_ptr<float>(), m.data_ptr<float>(),
      v.data_ptr<float>(), Wbf.has_value() ? Wbf->data_ptr() : nullptr,
      Wtbf.has_value() ? Wtbf->data_ptr() : nullptr, rows, cols, (float)lr,
      (float)beta1, (float)beta2, (float)eps, bc1, bc2, (float)l2,
      cur_stream());
}

void dense_adagrad(at::Tensor W, at::Tensor grad, at::Tensor n,
                   c10::optional<at::Tensor> Wbf,
                   c10::optional<at::Tensor> Wtbf, double lr, double eps,
                   double l2) {
  check_cuda_f32(W, "W");
  const int rows = (int)W.size(0);
  const int cols = (int)(W.numel() / W.size(0));
  lightctr::dense_adagrad_launch(
      W.data_ptr<float>(), grad.data_ptr<float>(), n.data_ptr<float>(),
      Wbf.has_value() ? Wbf->data_ptr() : nullptr,
      Wtbf.has_value() ? Wtbf->data_ptr() : nullptr, rows, cols, (float)lr,
      (float)eps, (float)l2, cur_stream());
}

// ---- embedding / NFM ----

at::Tensor embed_gather(at::Tensor row_ptr, at::Tensor fids, at::Tensor vals,
                        at::Tensor E, int64_t nf) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_i32(fids, "fids");
  check_cuda_f32(vals, "vals");
  check_cuda_f32(E, "E");
  CHK(E.dim() == 2, "E must be [F, K]");
  CHK(fids.numel() == vals.numel(), "fids/vals length mismatch");
  CHK(row_ptr.numel() >= 1, "row_ptr must hold B+1 offsets");
  CHK(nf >= 1, "nf must be >= 1");
  const int B = (int)row_ptr.numel() - 1;
  const int K = (int)E.size(1);
  check_embed_k(K);
  auto out = at::empty({B, nf * K}, E.options().dtype(at::kBFloat16));
  lightctr::embed_gather_launch(row_ptr.data_ptr<int>(), fids.data_ptr<int>(),
                                vals.data_ptr<float>(), E.data_ptr<float>(),
                                out.data_ptr(), (int)nf, B, K, cur_stream());
  return out;
}

std::vector<at::Tensor> embed_backward_emit(at::Tensor row_ptr,
                                            at::Tensor vals, at::Tensor dOut,
                                            at::Tensor dwide, int64_t nf,
                                            int64_t K) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_f32(dOut, "dOut");
  check_cuda_f32(vals, "vals");
  check_cuda_f32(dwide, "dwide");
  check_embed_k(K);
  CHK(nf >= 1, "nf must be >= 1");
  const int B = (int)row_ptr.numel() - 1;
  CHK(dOut.numel() == (int64_t)B * nf * K, "dOut must be [B, nf*K]");
  const auto nnz = vals.numel();
  auto gv = at::empty({nnz, K}, dOut.options());
  auto gw = at::empty({nnz}, dOut.options());
  lightctr::embed_backward_emit_launch(
      row_ptr.data_ptr<int>(), vals.data_ptr<float>(), dOut.data_ptr<float>(),
      dwide.data_ptr<float>(), gv.data_ptr<float>(), gw.data_ptr<float>(),
      (int)nf, B, (int)K, cur_stream());
  return {gw, gv};
}

at::Tensor w2v_negsample_step(at::Tensor E, at::Tensor O,
                              at::Tensor centers, at::Tensor ctx,
                              at::Tensor negs, double lr, double scale) {
  check_cuda_f32(E, "E");
  check_cuda_f32(O, "O");
  CHK(centers.scalar_type() == at::kLong, "centers i64");
  const int B = (int)centers.numel();
  CHK(E.dim() == 2 && O.dim() == 2 && O.size(1) == E.size(1),
      "E and O must be [V, D]");
  for (const at::Tensor* t : {&centers, &ctx, &negs})
    CHK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous(),
        "centers, ctx and negs must be contiguous int64 GPU tensors");
  CHK(ctx.dim() == 2 && ctx.size(0) == B && ctx.size(1) >= 1,
      "ctx must be [B, C] with C >= 1");
  CHK(negs.dim() == 2 && negs.size(0) == B, "negs must be [B, N]");
  const int C = (int)ctx.size(1);
  const int N = (int)negs.size(1);
  const int D = (int)E.size(1);
  CHK(D <= 64, "w2v kernel supports dim <= 64");
  auto loss = at::empty({B}, E.options());
  if (B == 0) return loss;
  lightctr::w2v_negsample_launch(
      E.data_ptr<float>(), O.data_ptr<float>(), centers.data_ptr<long>(),
      ctx.data_ptr<long>(), negs.data_ptr<long>(), loss.data_ptr<float>(),
      B, C, N, D, (float)lr, (float)scale, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return loss;
}

at::Tensor wide_forward(at::Tensor row_ptr, at::Tensor fids, at::Tensor vals,
                        at::Tensor W) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_f32(W, "W");
  const int B = (int)row_ptr.numel() - 1;
  auto wide = at::empty({B}, W.options());
  lightctr::wide_forward_launch(row_ptr.data_ptr<int>(), fids.data_ptr<int>(),
                                vals.data_ptr<float>(), W.data_ptr<float>(),
                                wide.data_ptr<float>(), B, cur_stream());
  return wide;
}

std::vector<at::Tensor> nfm_forward(at::Tensor row_ptr, at::Tensor fids,
                                    at::Tensor vals, at::Tensor W,
                                    at::Tensor V) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_f32(V, "V");
  const int B = (int)row_ptr.numel() - 1;
  const int K = (int)V.size(1);
  check_embed_k(K);
  auto wide = at::empty({B}, W.options());
  auto sumVX = at::empty({B, K}, V.options());
  auto vec = at::empty({B, K}, V.options());
  auto vec_bf = at::empty({B, K}, V.options().dtype(at::kBFloat16));
  lightctr::nfm_forward_launch(row_ptr.data_ptr<int>(), fids.data_ptr<int>(),
                               vals.data_ptr<float>(), W.data_ptr<float>(),
                               V.data_ptr<float>(), wide.data_ptr<float>(),
                               sumVX.data_ptr<float>(), vec.data_ptr<float>(),
                               vec_bf.data_ptr(), B, K, cur_stream());
  return {wide, sumVX, vec, vec_bf};
}

std::vector<at::Tensor> nfm_backward_emit(at::Tensor row_ptr, at::Tensor fids,
                                          at::Tensor vals, at::Tensor V,
                                          at::Tensor sumVX, at::Tensor dvec,
                                          at::Tensor dwide) {
  check_cuda_i32(row_ptr, "row_ptr");
  const int B = (int)row_ptr.numel() - 1;
  const int K = (int)V.size(1);
  check_embed_k(K);
  const auto nnz = fids.numel();
  auto gw = at::empty({nnz}, V.options());
  auto gv = at::empty({nnz, K}, V.options());
  lightctr::nfm_backward_emit_launch(
      row_ptr.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      V.data_ptr<float>(), sumVX.data_ptr<float>(), dvec.data_ptr<float>(),
      dwide.data_ptr<float>(), gw.data_ptr<float>(), gv.data_ptr<float>(), B,
      K, cur_stream());
  return {gw, gv};
}

// ---- DeepFM ----

// E is [F, K] fp32 with K in the dispatch set. Returns K.
int check_deepfm_e(const at::Tensor& E) {
  check_cuda_f32(E, "E");
  CHK(E.dim() == 2, "E must be [F, K]");
  check_embed_k(E.size(1));
  return (int)E.size(1);
}

// FM score (wide + pair term), sumVX and the bf16 concat [B, nf*K] of one
// shared table in one pass over the batch: fm_forward + embed_gather.
std::vector<at::Tensor> deepfm_forward(at::Tensor row_ptr, at::Tensor fids,
                                       at::Tensor vals, at::Tensor W,
                                       at::Tensor E, int64_t nf) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_deepfm_e(E);
  check_f32_n(W, E.size(0), "W");
  CHK(nf >= 1, "nf must be >= 1");
  CHK(nf * K <= std::numeric_limits<int>::max(), "nf * K must fit an int");
  auto fm = at::empty({B}, E.options());
  auto sumVX = at::empty({B, K}, E.options());
  auto deep_in = at::empty({B, nf * K}, E.options().dtype(at::kBFloat16));
  if (B == 0) return {fm, sumVX, deep_in};  // nothing is launched
  lightctr::deepfm_forward_launch(
      row_ptr.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      W.data_ptr<float>(), E.data_ptr<float>(), deep_in.data_ptr(),
      sumVX.data_ptr<float>(), fm.data_ptr<float>(), (int)nf, B, K,
      cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {fm, sumVX, deep_in};
}

// Per-entry gradients of both uses of E in one [nnz, K] buffer:
// gv = (dDeep + dpred (sumVX - E x)) x, gw = dpred x.
std::vector<at::Tensor> deepfm_backward_emit(
    at::Tensor row_ptr, at::Tensor fids, at::Tensor vals, at::Tensor E,
    at::Tensor sumVX, at::Tensor dDeep, at::Tensor dpred, int64_t nf) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_deepfm_e(E);
  CHK(nf >= 1, "nf must be >= 1");
  CHK(nf * K <= std::numeric_limits<int>::max(), "nf * K must fit an int");
  check_cuda_f32(sumVX, "sumVX");
  CHK(sumVX.dim() == 2 && sumVX.size(0) == B && sumVX.size(1) == K,
      "sumVX must be [B, K]");
  check_cuda_f32(dDeep, "dDeep");
  CHK(dDeep.dim() == 2 && dDeep.size(0) == B && dDeep.size(1) == nf * K,
      "dDeep must be [B, nf*K]");
  check_cuda_f32(dpred, "dpred");
  CHK(dpred.dim() == 1 && dpred.size(0) == B, "dpred must be [B]");
  const auto nnz = fids.numel();
  auto gw = at::empty({nnz}, E.options());
  auto gv = at::empty({nnz, K}, E.options());
  if (B == 0 || nnz == 0) return {gw, gv};
  lightctr::deepfm_backward_emit_launch(
      row_ptr.data_ptr<int>(), fids.data_ptr<int>(), vals.data_ptr<float>(),
      E.data_ptr<float>(), sumVX.data_ptr<float>(), dDeep.data_ptr<float>(),
      dpred.data_ptr<float>(), gw.data_ptr<float>(), gv.data_ptr<float>(),
      (int)nf, B, K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {gw, gv};
}

// ---- field-addressed embedding bags ----

// The forward kernels stage one [nf, K] fp32 slice and nf counters per wave
// in dynamic LDS; a request past the per-block limit is a launch error that
// would leave the outputs unwritten. Checked by all four bindings, so a
// forward that is accepted has a backward that is.
void check_bag_args(const at::Tensor& fields, const at::Tensor& fids,
                    int64_t nf, int K, int64_t pooling, const char* op) {
  check_i32_n(fields, fids.numel(), "fields");
  CHK(pooling == 0 || pooling == 1, op,
      ": pooling must be 0 (sum) or 1 (mean), got ", pooling);
  CHK(nf >= 1, "nf must be >= 1");
  CHK(nf * K <= std::numeric_limits<int>::max() / 32,
      "nf * K must fit an int");
  const long need = lightctr::embed_bag_lds_bytes((int)nf, K);
  const long have = lightctr::ffm_max_lds_per_block();
  CHK(need <= have, op, ": nf=", nf, ", K=", K, " needs ", need,
      " bytes of LDS per block, the device gives ", have);
}

// bf16 concat [B, nf*K] addressed by field, sum (0) or mean (1) pooled
at::Tensor embed_bag_forward(at::Tensor row_ptr, at::Tensor fields,
                             at::Tensor fids, at::Tensor vals, at::Tensor E,
                             int64_t nf, int64_t pooling) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_deepfm_e(E);
  check_bag_args(fields, fids, nf, K, pooling, "embed_bag_forward");
  auto out = at::empty({B, nf * K}, E.options().dtype(at::kBFloat16));
  if (B == 0) return out;  // nothing is launched
  lightctr::embed_bag_forward_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), E.data_ptr<float>(), out.data_ptr(), (int)nf,
      (int)pooling, B, K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return out;
}

// gv = dOut[r, c*K+k] inv x, gw = dwide[r] x
std::vector<at::Tensor> embed_bag_backward_emit(
    at::Tensor row_ptr, at::Tensor fields, at::Tensor vals, at::Tensor dOut,
    at::Tensor dwide, int64_t nf, int64_t K, int64_t pooling) {
  check_cuda_i32(row_ptr, "row_ptr");
  check_cuda_f32(vals, "vals");
  CHK(row_ptr.numel() >= 1, "row_ptr must hold B + 1 offsets");
  const int B = (int)row_ptr.numel() - 1;
  check_embed_k(K);
  check_bag_args(fields, vals, nf, (int)K, pooling,
                 "embed_bag_backward_emit");
  check_cuda_f32(dOut, "dOut");
  CHK(dOut.dim() == 2 && dOut.size(0) == B && dOut.size(1) == nf * K,
      "dOut must be [B, nf*K]");
  check_cuda_f32(dwide, "dwide");
  CHK(dwide.dim() == 1 && dwide.size(0) == B, "dwide must be [B]");
  const auto nnz = vals.numel();
  auto gw = at::empty({nnz}, dOut.options());
  auto gv = at::empty({nnz, K}, dOut.options());
  if (B == 0 || nnz == 0) return {gw, gv};
  lightctr::embed_bag_backward_emit_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(),
      vals.data_ptr<float>(), dOut.data_ptr<float>(),
      dwide.data_ptr<float>(), gw.data_ptr<float>(), gv.data_ptr<float>(),
      (int)nf, (int)pooling, B, (int)K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {gw, gv};
}

// deepfm_forward with the concat addressed by field
std::vector<at::Tensor> deepfm_bag_forward(at::Tensor row_ptr,
                                           at::Tensor fields, at::Tensor fids,
                                           at::Tensor vals, at::Tensor W,
                                           at::Tensor E, int64_t nf,
                                           int64_t pooling) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_deepfm_e(E);
  check_f32_n(W, E.size(0), "W");
  check_bag_args(fields, fids, nf, K, pooling, "deepfm_bag_forward");
  auto fm = at::empty({B}, E.options());
  auto sumVX = at::empty({B, K}, E.options());
  auto deep_in = at::empty({B, nf * K}, E.options().dtype(at::kBFloat16));
  if (B == 0) return {fm, sumVX, deep_in};  // nothing is launched
  lightctr::deepfm_bag_forward_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), W.data_ptr<float>(), E.data_ptr<float>(),
      deep_in.data_ptr(), sumVX.data_ptr<float>(), fm.data_ptr<float>(),
      (int)nf, (int)pooling, B, K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {fm, sumVX, deep_in};
}

// deepfm_backward_emit with D read at the entry's field and scaled by inv
std::vector<at::Tensor> deepfm_bag_backward_emit(
    at::Tensor row_ptr, at::Tensor fields, at::Tensor fids, at::Tensor vals,
    at::Tensor E, at::Tensor sumVX, at::Tensor dDeep, at::Tensor dpred,
    int64_t nf, int64_t pooling) {
  const int B = check_fm_csr(row_ptr, fids, vals);
  const int K = check_deepfm_e(E);
  check_bag_args(fields, fids, nf, K, pooling, "deepfm_bag_backward_emit");
  check_cuda_f32(sumVX, "sumVX");
  CHK(sumVX.dim() == 2 && sumVX.size(0) == B && sumVX.size(1) == K,
      "sumVX must be [B, K]");
  check_cuda_f32(dDeep, "dDeep");
  CHK(dDeep.dim() == 2 && dDeep.size(0) == B && dDeep.size(1) == nf * K,
      "dDeep must be [B, nf*K]");
  check_cuda_f32(dpred, "dpred");
  CHK(dpred.dim() == 1 && dpred.size(0) == B, "dpred must be [B]");
  const auto nnz = fids.numel();
  auto gw = at::empty({nnz}, E.options());
  auto gv = at::empty({nnz, K}, E.options());
  if (B == 0 || nnz == 0) return {gw, gv};
  lightctr::deepfm_bag_backward_emit_launch(
      row_ptr.data_ptr<int>(), fields.data_ptr<int>(), fids.data_ptr<int>(),
      vals.data_ptr<float>(), E.data_ptr<float>(), sumVX.data_ptr<float>(),
      dDeep.data_ptr<float>(), dpred.data_ptr<float>(),
      gw.data_ptr<float>(), gv.data_ptr<float>(), (int)nf, (int)pooling, B,
      K, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return {gw, gv};
}

// ---- native data loader ----
// Fast single-pass libffm parser ("label field:fid:val" per line) —
// native equivalent of the reference's C++ loader
// (/root/reference/LightCTR/fm_algo_abst.h:70-107), ~20x the Python
// line-split loader. Returns (row_ptr i32, fields i32, fids i32,
// vals f32, labels f32) CPU tensors.
std::vector<at::Tensor> parse_libffm(const std::string& path,
                                     int64_t max_rows) {
  FILE* f = fopen(path.c_str(), "rb");
  TORCH_CHECK(f != nullptr, "cannot open ", path);
  fseek(f, 0, SEEK_END);
  const long size = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> buf(size + 1);
  const size_t rd = fread(buf.data(), 1, size, f);
  fclose(f);
  TORCH_CHECK((long)rd == size, "short read on ", path);
  buf[size] = '\0';

  std::vector<int> row_ptr{0};
  std::vector<int> fields, fids;
  std::vector<float> vals, labels;
  char* p = buf.data();
  char* end = buf.data() + size;
  while (p < end) {
    // label
    while (p < end && (*p == ' ' || *p == '\n' || *p == '\r')) ++p;
    if (p >= end) break;
    char* q;
    const float label = strtof(p, &q);
    TORCH_CHECK(q != p, "bad label near byte ", (long)(p - buf.data()));
    p = q;
    // features until newline
    while (p < end && *p != '\n') {
      while (p < end && *p == ' ') ++p;
      if (p >= end || *p == '\n') break;
      const long fld = strtol(p, &q, 10);
      TORCH_CHECK(q != p && *q == ':', "bad field token");
      p = q + 1;
      const long fid = strtol(p, &q, 10);
      TORCH_CHECK(q != p && *q == ':', "bad fid token");
      p = q + 1;
      const float v = strtof(p, &q);
      TORCH_CHECK(q != p, "bad value token");
      p = q;
      fields.push_back((int)fld);
      fids.push_back((int)fid);
      vals.push_back(v);
    }
    labels.push_back(label);
    row_ptr.push_back((int)fids.size());
    if (max_rows > 0 && (int64_t)labels.size() >= max_rows) break;
  }
  auto opts_i = at::TensorOptions().dtype(at::kInt);
  auto opts_f = at::TensorOptions().dtype(at::kFloat);
  auto t_rp = at::empty({(long)row_ptr.size()}, opts_i);
  memcpy(t_rp.data_ptr<int>(), row_ptr.data(), row_ptr.size() * 4);
  auto t_fl = at::empty({(long)fields.size()}, opts_i);
  memcpy(t_fl.data_ptr<int>(), fields.data(), fields.size() * 4);
  auto t_fi = at::empty({(long)fids.size()}, opts_i);
  memcpy(t_fi.data_ptr<int>(), fids.data(), fids.size() * 4);
  auto t_v = at::empty({(long)vals.size()}, opts_f);
  memcpy(t_v.data_ptr<float>(), vals.data(), vals.size() * 4);
  auto t_l = at::empty({(long)labels.size()}, opts_f);
  memcpy(t_l.data_ptr<float>(), labels.data(), labels.size() * 4);
  return {t_rp, t_fl, t_fi, t_v, t_l};
}

// ---- codecs ----

// the kernels stage the table in LDS and emit one uint8 code per value
void check_quantile_table(const at::Tensor& table) {
  check_cuda_f32(table, "table");
  CHK(table.numel() >= 1 && table.numel() <= 256,
      "quantile table must hold 1..256 levels, got ", table.numel());
}

at::Tensor quantile_encode(at::Tensor x, at::Tensor table) {
  check_cuda_f32(x, "x");
  check_quantile_table(table);
  auto code = at::empty(x.sizes(), x.options().dtype(at::kByte));
  if (x.numel() == 0) return code;
  lightctr::quantile_encode_launch(x.data_ptr<float>(),
                                   code.data_ptr<unsigned char>(),
                                   table.data_ptr<float>(),
                                   (int)table.numel(), x.numel(),
                                   cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return code;
}

at::Tensor quantile_decode(at::Tensor code, at::Tensor table) {
  check_quantile_table(table);
  CHK(code.is_cuda(), "code must be on GPU");
  CHK(code.scalar_type() == at::kByte, "code must be uint8");
  CHK(code.is_contiguous(), "code must be contiguous");
  auto x = at::empty(code.sizes(), table.options());
  if (code.numel() == 0) return x;
  lightctr::quantile_decode_launch(code.data_ptr<unsigned char>(),
                                   x.data_ptr<float>(),
                                   table.data_ptr<float>(),
                                   (int)table.numel(), code.numel(),
                                   cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return x;
}

at::Tensor lowbit_encode(at::Tensor x, double thresh, int64_t bits) {
  check_cuda_f32(x, "x");
  CHK(bits == 1 || bits == 2, "lowbit: bits must be 1 or 2, got ", bits);
  const long n = x.numel();
  const long nw = (n * bits + 31) / 32;
  auto words = at::empty({nw}, x.options().dtype(at::kInt));
  if (n == 0) return words;
  lightctr::lowbit_encode_launch(x.data_ptr<float>(),
                                 (unsigned int*)words.data_ptr(),
                                 (float)thresh, (int)bits, n, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return words;
}

at::Tensor lowbit_decode(at::Tensor words, double lo, double hi, int64_t bits,
                         int64_t n) {
  CHK(bits == 1 || bits == 2, "lowbit: bits must be 1 or 2, got ", bits);
  check_cuda_i32(words, "words");
  CHK(n >= 0, "lowbit: n must be >= 0, got ", n);
  CHK(words.numel() >= (n * bits + 31) / 32, "lowbit: ", n, " values at ",
      bits, " bits need ", (n * bits + 31) / 32, " words, got ",
      words.numel());
  auto x = at::empty({n}, words.options().dtype(at::kFloat));
  if (n == 0) return x;
  lightctr::lowbit_decode_launch((const unsigned int*)words.data_ptr(),
                                 x.data_ptr<float>(), (float)lo, (float)hi,
                                 (int)bits, n, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return x;
}

at::Tensor gbm_hist(at::Tensor bins, at::Tensor grad, at::Tensor hess,
                    at::Tensor node_of_row, int64_t n_nodes) {
  CHK(bins.is_cuda() && bins.scalar_type() == at::kByte, "bins u8");
  check_cuda_f32(grad, "grad");
  check_cuda_f32(hess, "hess");
  check_cuda_i32(node_of_row, "node_of_row");
  CHK(bins.dim() == 2 && bins.is_contiguous(),
      "bins must be a contiguous [N, D] tensor");
  // one grid row per node: gridDim.y stops at 65535
  CHK(n_nodes >= 1 && n_nodes <= 65535,
      "gbm_hist: n_nodes must be in 1..65535, got ", n_nodes);
  const int N = (int)bins.size(0), D = (int)bins.size(1);
  CHK(grad.numel() == N && hess.numel() == N && node_of_row.numel() == N,
      "grad, hess and node_of_row must each hold N = ", N, " entries");
  auto hist = at::zeros({n_nodes, D, 256, 2}, grad.options());
  if (N == 0 || D == 0) return hist;
  lightctr::gbm_hist_launch(bins.data_ptr<unsigned char>(),
                            grad.data_ptr<float>(), hess.data_ptr<float>(),
                            node_of_row.data_ptr<int>(),
                            hist.data_ptr<float>(), N, D, (int)n_nodes,
                            cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return hist;
}

// Compiled-forest inference (predict/forest.py). The tables come from
// CompiledForest, which validates the trees; shapes are re-checked here.
at::Tensor gbm_forest(at::Tensor X, at::Tensor nodes, at::Tensor tree_off,
                      at::Tensor tree_class, at::Tensor leaf_base,
                      at::Tensor chunks, int64_t mode, int64_t n_features,
                      int64_t n_classes, int64_t max_depth,
                      int64_t fid_offset) {
  check_cuda_f32(X, "X");
  CHK(X.dim() == 2 && X.size(1) == n_features, "X must be [N, ",
      n_features, "]");
  check_cuda_i32(nodes, "nodes");
  check_cuda_i32(tree_off, "tree_off");
  check_cuda_i32(tree_class, "tree_class");
  check_cuda_i32(leaf_base, "leaf_base");
  check_cuda_i32(chunks, "chunks");
  CHK(nodes.dim() == 2 && nodes.size(1) == 4, "nodes must be [n, 4]");
  CHK(chunks.dim() == 2 && chunks.size(1) == 4, "chunks must be [c, 4]");
  CHK(((uintptr_t)nodes.data_ptr()) % 16 == 0 &&
          ((uintptr_t)chunks.data_ptr()) % 16 == 0,
      "nodes/chunks must be 16-byte aligned");
  CHK(mode >= 0 && mode <= 2, "mode must be 0 (margin), 1 (leaf), 2 (fid)");
  CHK(n_classes >= 1 && max_depth >= 0, "bad n_classes / max_depth");
  const int64_t N = X.size(0), T = tree_class.numel();
  CHK(tree_off.numel() == T + 1 && leaf_base.numel() == T,
      "tree tables disagree on the tree count");
  CHK(n_features >= 1 || N == 0, "X needs at least one column");
  CHK(N * std::max<int64_t>(T, n_classes) < ((int64_t)1 << 40),
      "output too large");
  at::Tensor out =
      mode == 0 ? at::zeros({N, n_classes}, X.options())
                : at::empty({N, T}, X.options().dtype(at::kInt));
  if (N == 0 || T == 0 || chunks.size(0) == 0) return out;
  lightctr::gbm_forest_launch(
      X.data_ptr<float>(), nodes.data_ptr(), tree_off.data_ptr<int>(),
      tree_class.data_ptr<int>(), leaf_base.data_ptr<int>(),
      chunks.data_ptr(), (int)chunks.size(0), out.data_ptr(), (long)N,
      (int)n_features, (int)T, (int)n_classes, (int)max_depth,
      (int)fid_offset, (int)mode, cur_stream());
  return out;
}

// ---- nearest-neighbour search (predict/knn.py) ----

void check_knn_k(int64_t k) {
  CHK(k >= 1 && k <= lightctr::knn_max_k(), "k must be in [1, ",
      lightctr::knn_max_k(), "], got ", k);
}

void check_knn_metric(int64_t metric) {
  CHK(metric == 0 || metric == 1, "metric must be 0 (l2) or 1 (ip)");
}

// (ids, dist) preset to the empty result, for N == 0
std::vector<at::Tensor> knn_outputs(int64_t nq, int64_t k,
                                    const at::Tensor& like, bool fill) {
  auto ids = at::empty({nq, k}, like.options().dtype(at::kInt));
  auto dist = at::empty({nq, k}, like.options().dtype(at::kFloat));
  if (fill) {
    ids.fill_(-1);
    dist.fill_(std::numeric_limits<float>::infinity());
  }
  return {ids, dist};
}

at::Tensor pq_lut(at::Tensor Q, at::Tensor centroids, int64_t metric) {
  check_cuda_f32(Q, "Q");
  check_cuda_f32(centroids, "centroids");
  check_knn_metric(metric);
  CHK(Q.dim() == 2, "Q must be [nq, dim]");
  CHK(centroids.dim() == 3, "centroids must be [n_sub, ncb, d_sub]");
  const int64_t nq = Q.size(0), n_sub = centroids.size(0),
                ncb = centroids.size(1), d_sub = centroids.size(2);
  CHK(n_sub >= 1 && n_sub <= lightctr::knn_max_sub(), "n_sub must be in [1, ",
      lightctr::knn_max_sub(), "], got ", n_sub);
  CHK(ncb >= 1 && ncb <= 256, "ncb must be in [1, 256], got ", ncb);
  CHK(d_sub >= 1 && n_sub * d_sub == Q.size(1), "Q has ", Q.size(1),
      " columns, the centroids span ", n_sub * d_sub);
  CHK(nq * n_sub * ncb < ((int64_t)1 << 31) * 256, "LUT too large");
  auto lut = at::empty({nq, n_sub, ncb}, Q.options());
  if (nq == 0) return lut;
  lightctr::pq_lut_launch(Q.data_ptr<float>(), centroids.data_ptr<float>(),
                          lut.data_ptr<float>(), (long)nq, (int)n_sub,
                          (int)ncb, (int)d_sub, (int)metric, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return lut;
}

std::vector<at::Tensor> pq_adc_topk(at::Tensor lut, at::Tensor codes,
                                    int64_t ncb, int64_t k) {
  check_cuda_f32(lut, "lut");
  CHK(codes.is_cuda(), "codes must be on GPU");
  CHK(codes.scalar_type() == at::kByte, "codes must be uint8");
  CHK(lut.dim() == 3, "lut must be [nq, n_sub, ncb]");
  CHK(codes.dim() == 2, "codes must be [N, n_sub]");
  check_knn_k(k);
  const int64_t nq = lut.size(0), n_sub = lut.size(1), N = codes.size(0);
  CHK(n_sub >= 1 && n_sub <= lightctr::knn_max_sub(), "n_sub must be in [1, ",
      lightctr::knn_max_sub(), "], got ", n_sub);
  CHK(ncb >= 1 && ncb <= 256, "ncb must be in [1, 256], got ", ncb);
  CHK(lut.size(2) == ncb, "lut is ", lut.size(2), " wide, ncb is ", ncb);
  CHK(codes.size(1) == n_sub, "codes have ", codes.size(1),
      " columns, lut has ", n_sub, " sub-vectors");
  CHK(N < ((int64_t)1 << 31), "N must be below 2^31");
  CHK(N <= 1 || n_sub == 1 || codes.stride(1) == 1,
      "codes rows must be dense (column stride 1)");
  CHK(N <= 1 || codes.stride(0) >= n_sub, "codes rows overlap");
  const long need = lightctr::pq_adc_lds_bytes((int)n_sub, (int)ncb);
  const long have = lightctr::ffm_max_lds_per_block();
  CHK(need <= have, "pq_adc_topk: n_sub=", n_sub, ", ncb=", ncb, " needs ",
      need, " bytes of LDS per block, the device gives ", have);
  auto out = knn_outputs(nq, k, lut, N == 0);
  if (nq == 0 || N == 0) return out;
  const long rows = lightctr::knn_slice_rows((long)N, (long)nq);
  const int64_t n_slices = (N + rows - 1) / rows;
  CHK(nq * n_slices < ((int64_t)1 << 31), "too many blocks");
  at::Tensor partial;
  if (n_slices > 1)
    partial = at::empty({nq, n_slices, k}, lut.options().dtype(at::kLong));
  lightctr::pq_adc_topk_launch(
      lut.data_ptr<float>(), codes.data_ptr<unsigned char>(),
      (long)(N > 1 ? codes.stride(0) : n_sub), (long)N, (long)nq, (int)n_sub,
      (int)ncb, (int)k, rows, (int)n_slices,
      n_slices > 1 ? partial.data_ptr() : nullptr, out[0].data_ptr<int>(),
      out[1].data_ptr<float>(), cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  if (n_slices > 1) {
    lightctr::knn_merge_launch(partial.data_ptr(), (long)nq, (int)n_slices,
                               (int)k, 0, out[0].data_ptr<int>(),
                               out[1].data_ptr<float>(), cur_stream());
    C10_CUDA_KERNEL_LAUNCH_CHECK();
  }
  return out;
}

std::vector<at::Tensor> flat_topk(at::Tensor X, at::Tensor Q, int64_t metric,
                                  int64_t k, c10::optional<at::Tensor> cand) {
  check_cuda_f32(Q, "Q");
  CHK(X.is_cuda(), "X must be on GPU");
  CHK(X.scalar_type() == at::kFloat, "X must be fp32");
  CHK(X.dim() == 2 && Q.dim() == 2, "X must be [N, dim], Q [nq, dim]");
  check_knn_metric(metric);
  check_knn_k(k);
  const int64_t N = X.size(0), dim = X.size(1), nq = Q.size(0);
  CHK(dim >= 1 && dim <= lightctr::knn_max_dim(), "dim must be in [1, ",
      lightctr::knn_max_dim(), "], got ", dim);
  CHK(Q.size(1) == dim, "Q has ", Q.size(1), " columns, X has ", dim);
  CHK(N < ((int64_t)1 << 31), "N must be below 2^31");
  CHK(N <= 1 || dim == 1 || X.stride(1) == 1,
      "X rows must be dense (column stride 1)");
  CHK(N <= 1 || X.stride(0) >= dim, "X rows overlap");
  int64_t n_items = N;
  const int* cand_p = nullptr;
  if (cand.has_value()) {
    check_cuda_i32(*cand, "cand");
    CHK(cand->dim() == 2 && cand->size(0) == nq, "cand must be [nq, R]");
    n_items = cand->size(1);
    cand_p = cand->data_ptr<int>();
  }
  auto out = knn_outputs(nq, k, Q, N == 0 || n_items == 0);
  if (nq == 0 || N == 0 || n_items == 0) return out;
  const long rows = lightctr::knn_slice_rows((long)n_items, (long)nq);
  const int64_t n_slices = (n_items + rows - 1) / rows;
  CHK(nq * n_slices < ((int64_t)1 << 31), "too many blocks");
  at::Tensor partial;
  if (n_slices > 1)
    partial = at::empty({nq, n_slices, k}, Q.options().dtype(at::kLong));
  lightctr::flat_topk_launch(
      X.data_ptr<float>(), (long)(N > 1 ? X.stride(0) : dim), (long)N,
      (int)dim, Q.data_ptr<float>(), (long)nq, cand_p, (long)n_items,
      (int)metric, (int)k, rows, (int)n_slices,
      n_slices > 1 ? partial.data_ptr() : nullptr, out[0].data_ptr<int>(),
      out[1].data_ptr<float>(), cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  if (n_slices > 1) {
    lightctr::knn_merge_launch(partial.data_ptr(), (long)nq, (int)n_slices,
                               (int)k, cand_p ? 1 : 0,
                               out[0].data_ptr<int>(),
                               out[1].data_ptr<float>(), cur_stream());
    C10_CUDA_KERNEL_LAUNCH_CHECK();
  }
  return out;
}

// ---- random-projection forest (predict/rp_forest.py) ----

at::Tensor forest_candidates(at::Tensor planes, at::Tensor bias,
                             at::Tensor child, at::Tensor roots,
                             at::Tensor leaf_off, at::Tensor leaf_items,
                             at::Tensor Q, int64_t search_k, int64_t width) {
  check_cuda_f32(planes, "planes");
  check_cuda_f32(bias, "bias");
  check_cuda_i32(child, "child");
  check_cuda_i32(roots, "roots");
  check_cuda_i32(leaf_off, "leaf_off");
  check_cuda_i32(leaf_items, "leaf_items");
  check_cuda_f32(Q, "Q");
  CHK(planes.dim() == 2 && Q.dim() == 2,
      "planes must be [n_inner, dim], Q [nq, dim]");
  const int64_t n_inner = planes.size(0), dim = planes.size(1),
                nq = Q.size(0), T = roots.numel(),
                total = leaf_items.numel();
  CHK(dim >= 1 && dim <= lightctr::knn_max_dim(), "dim must be in [1, ",
      lightctr::knn_max_dim(), "], got ", dim);
  CHK(Q.size(1) == dim, "Q has ", Q.size(1), " columns, the planes have ",
      dim);
  CHK(bias.dim() == 1 && bias.size(0) == n_inner, "bias must be [n_inner]");
  CHK(child.dim() == 2 && child.size(0) == n_inner && child.size(1) == 2,
      "child must be [n_inner, 2]");
  CHK(roots.dim() == 1 && T >= 1, "roots must be [T] with T >= 1");
  CHK(leaf_off.dim() == 1 && leaf_off.numel() >= 1,
      "leaf_off must be [n_leaves + 1]");
  CHK(leaf_items.dim() == 1, "leaf_items must be [total]");
  const int64_t n_leaves = leaf_off.numel() - 1;
  const int64_t lim = ((int64_t)1 << 31) - 1;
  CHK(n_inner <= lim && n_leaves < lim && T <= lim && total <= lim,
      "forest arrays must hold fewer than 2^31 entries");
  CHK(search_k >= 1 && search_k <= lightctr::forest_max_search(),
      "search_k must be in [1, ", lightctr::forest_max_search(), "], got ",
      search_k);
  CHK(width >= search_k, "width ", width, " is below search_k ", search_k);
  CHK(width < ((int64_t)1 << 31) && nq * width < ((int64_t)1 << 40),
      "candidate list too large");
  CHK((nq + 3) / 4 < ((int64_t)1 << 31), "too many blocks");
  auto cand = at::empty({nq, width}, Q.options().dtype(at::kInt));
  if (nq == 0) return cand;
  lightctr::forest_candidates_launch(
      planes.data_ptr<float>(), bias.data_ptr<float>(), child.data_ptr<int>(),
      roots.data_ptr<int>(), leaf_off.data_ptr<int>(),
      leaf_items.data_ptr<int>(), Q.data_ptr<float>(), cand.data_ptr<int>(),
      (long)nq, (int)dim, (int)n_inner, (int)n_leaves, (int)T, (long)total,
      (int)search_k, (long)width, cur_stream());
  C10_CUDA_KERNEL_LAUNCH_CHECK();
  return cand;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "lightctr_amd HIP kernels (gfx950)";
  m.def("fm_forward", &fm_forward, "FM fused forward (pred, sumVX)");
  m.def("logloss_grad", &logloss_grad, "stable logloss + dpred");
  m.def("fm_forward_train", &fm_forward_train,
        "FM training forward -> (loss, dpred, sumVX, rec)",
        py::arg("row_ptr"), py::arg("fids"), py::arg("vals"), py::arg("W"),
        py::arg("V"), py::arg("label"), py::arg("scale"),
        py::arg("reset") = py::none());
  m.def("fm_backward", &fm_backward, "FM fused backward scatter");
  m.def("fm_backward_emit", &fm_backward_emit,
        "FM backward phase 1: per-entry grads (no atomics); pos=write slots",
        py::arg("row_ptr"), py::arg("fids"), py::arg("vals"), py::arg("V"),
        py::arg("sumVX"), py::arg("dpred"), py::arg("pos") = py::none());
  m.def("fm_sorted_apply", &fm_sorted_apply,
        "FM backward phase 2: segment-reduce sorted grads into slabs "
        "(perm=None -> grads already in sorted order)",
        py::arg("sorted_fids"), py::arg("perm"), py::arg("gw"),
        py::arg("gv"), py::arg("gradW"), py::arg("gradV"),
        py::arg("touched"), py::arg("chunk") = 0);
  m.def("fm_sorted_apply_fused", &fm_sorted_apply_fused,
        "segment-reduce + fused optimizer for interior segments",
        py::arg("sorted_fids"), py::arg("perm"), py::arg("gw"),
        py::arg("gv"), py::arg("gradW"), py::arg("gradV"),
        py::arg("touched"), py::arg("W"), py::arg("V"), py::arg("nW"),
        py::arg("nV"), py::arg("zW"), py::arg("zV"), py::arg("opt_mode"),
        py::arg("p0"), py::arg("p1"), py::arg("p2"), py::arg("p3"),
        py::arg("v_lr") = 0.05, py::arg("v_eps") = 1e-8,
        py::arg("v_l2") = 1e-5);
  m.def("segment_worklist", &segment_worklist,
        "piece starts of a sorted id stream -> (piece_start, n_pieces)",
        py::arg("sorted_fids"), py::arg("cap"),
        py::arg("reset") = py::none());
  m.def("fm_segment_apply", &fm_segment_apply,
        "per-piece segment reduce + fused optimizer; partial pieces spill",
        py::arg("sorted_fids"), py::arg("perm"), py::arg("piece_start"),
        py::arg("n_pieces"), py::arg("gw"), py::arg("gv"), py::arg("gradW"),
        py::arg("gradV"), py::arg("spill"), py::arg("spill_count"),
        py::arg("W"), py::arg("V"), py::arg("nW"), py::arg("nV"),
        py::arg("zW"), py::arg("zV"), py::arg("opt_mode"), py::arg("p0"),
        py::arg("p1"), py::arg("p2"), py::arg("p3"), py::arg("v_lr") = 0.05,
        py::arg("v_eps") = 1e-8, py::arg("v_l2") = 1e-5);
  m.def("fm_segment_apply_rec", &fm_segment_apply_rec,
        "per-piece segment reduce recomputing the gradients from sorted "
        "records + fused optimizer; partial pieces spill",
        py::arg("sorted_fids"), py::arg("sorted_rec"), py::arg("sumVX"),
        py::arg("dpred"), py::arg("piece_start"), py::arg("n_pieces"),
        py::arg("gradW"), py::arg("gradV"), py::arg("spill"),
        py::arg("spill_count"), py::arg("W"), py::arg("V"), py::arg("nW"),
        py::arg("nV"), py::arg("zW"), py::arg("zV"), py::arg("opt_mode"),
        py::arg("p0"), py::arg("p1"), py::arg("p2"), py::arg("p3"),
        py::arg("v_lr") = 0.05, py::arg("v_eps") = 1e-8,
        py::arg("v_l2") = 1e-5);
  m.def("fm_segment_tile_rec", &fm_segment_tile_rec,
        "tile-local segment reduce recomputing the gradients from sorted "
        "records + fused optimizer; partial pieces spill",
        py::arg("sorted_fids"), py::arg("sorted_rec"), py::arg("sumVX"),
        py::arg("dpred"), py::arg("cap"), py::arg("gradW"), py::arg("gradV"),
        py::arg("spill"), py::arg("spill_count"), py::arg("W"), py::arg("V"),
        py::arg("nW"), py::arg("nV"), py::arg("zW"), py::arg("zV"),
        py::arg("opt_mode"), py::arg("p0"), py::arg("p1"), py::arg("p2"),
        py::arg("p3"), py::arg("v_lr") = 0.05, py::arg("v_eps") = 1e-8,
        py::arg("v_l2") = 1e-5);
  m.def("fm_segment_tile", &lightctr::fm_segment_tile,
        "entries per block of fm_segment_tile_rec");
  m.def("fm_segment_split", &lightctr::fm_segment_split,
        "longest unit one subgroup sums in fm_segment_tile_rec");
  m.def("ffm_forward", &ffm_forward, "FFM pairwise forward (LDS-staged)");
  m.def("ffm_forward_pp", &ffm_forward_pp, "lane-per-pair FFM forward");
  m.def("ffm_row_emit", &ffm_row_emit,
        "FFM per-row staged fp16 block emit -> (gw, gblocks)",
        py::arg("row_ptr"), py::arg("fields"), py::arg("fids"),
        py::arg("vals"), py::arg("V"), py::arg("dpred"),
        py::arg("scale") = 1.0);
  m.def("ffm_blocks_apply_f16", &ffm_blocks_apply_f16,
        "segment-reduce fp16 blocks into slabs (interior stores), "
        "optionally with the optimizer fused for interior runs",
        py::arg("sorted_fids"), py::arg("perm"), py::arg("gblocks"),
        py::arg("gw"), py::arg("gradW"), py::arg("gradV"),
        py::arg("touched"), py::arg("inv_scale") = 1.0,
        py::arg("opt_mode") = 0, py::arg("V") = py::none(),
        py::arg("W") = py::none(), py::arg("nW") = py::none(),
        py::arg("zW") = py::none(), py::arg("nV") = py::none(),
        py::arg("Vh") = py::none(), py::arg("p0") = 0.0,
        py::arg("p1") = 0.0, py::arg("p2") = 0.0, py::arg("p3") = 0.0,
        py::arg("q0") = 0.0, py::arg("q1") = 0.0, py::arg("q2") = 0.0);
  m.def("ffm_backward", &ffm_backward, "FFM fused pairwise backward scatter");
  m.def("ffm_sorted_backward", &ffm_sorted_backward,
        "FFM sorted segment-reduce backward (LDS block accumulate)");
  m.def("row_index", &row_index, "entry -> row index from row_ptr");
  m.def("ffm_block_lds_bytes", &lightctr::ffm_block_lds_bytes,
        "dynamic LDS per block of ffm_sorted_backward / ffm_block_emit",
        py::arg("nfields"), py::arg("K"));
  m.def("ffm_max_lds_per_block", &lightctr::ffm_max_lds_per_block,
        "per-block LDS limit of the current device, in bytes");
  m.def("ffm_block_emit", &ffm_block_emit,
        "FFM per-entry [nf,K] gradient blocks (wave/entry)");
  m.def("ffm_blocks_apply", &ffm_blocks_apply,
        "segment-reduce sorted FFM blocks into slabs");
  m.def("parse_libffm", &parse_libffm, "native libffm text parser",
        py::arg("path"), py::arg("max_rows") = -1);
  m.def("sparse_adagrad_apply", &sparse_adagrad_apply,
        "generic sparse fused Adagrad (runtime D)",
        py::arg("uniq"), py::arg("count"), py::arg("W"), py::arg("V"),
        py::arg("nW"), py::arg("nV"), py::arg("gradW"), py::arg("gradV"),
        py::arg("lr"), py::arg("eps"), py::arg("l2"),
        py::arg("Vh") = py::none());
  m.def("ps_apply", &ps_apply,
        "PS-side fused updater (sgd/adagrad/dcasgd/dcasgda)");
  m.def("ps_dense_check", &ps_dense_check,
        "PS dense push: non-finite scan of the payload -> flags[0]",
        py::arg("payload"), py::arg("scale"), py::arg("table"),
        py::arg("flags"));
  m.def("ps_dense_apply", &ps_dense_apply,
        "PS dense push: fused decode + updater over the slab, gated on "
        "flags[0]; a gated push bumps flags[1]. flags[0] is only what the "
        "last ps_dense_check left there: call ps_dense_check on the same "
        "payload, on the same stream, immediately before every call (as "
        "DenseTable.apply does) — called alone it acts on a stale flag",
        py::arg("payload"), py::arg("scale"), py::arg("table"),
        py::arg("slab"), py::arg("acc"), py::arg("shadow"),
        py::arg("flags"), py::arg("updater"), py::arg("lr"),
        py::arg("lam"), py::arg("eps"));
  m.def("ps_dense_pack", &ps_dense_pack,
        "PS dense pull: slab -> fp32/fp16 payload (+ shadow = slab)",
        py::arg("slab"), py::arg("shadow"), py::arg("fp16"));
  m.def("sparse_ftrl_apply", &sparse_ftrl_apply,
        "generic sparse fused FTRL (runtime D; optional Adagrad on V)",
        py::arg("uniq"), py::arg("count"), py::arg("W"), py::arg("V"),
        py::arg("zW"), py::arg("nW"), py::arg("zV"), py::arg("nV"),
        py::arg("gradW"), py::arg("gradV"), py::arg("alpha"),
        py::arg("beta"), py::arg("l1"), py::arg("l2"),
        py::arg("v_adagrad") = 0, py::arg("v_lr") = 0.05,
        py::arg("v_eps") = 1e-8, py::arg("v_l2") = 1e-5,
        py::arg("Vh") = py::none());
  m.def("gemm_bf16", &gemm_bf16, "MFMA bf16 GEMM (C fp32), fused bias+act");
  m.def("gemm_bf16_full", &gemm_bf16_full,
        "MFMA bf16 GEMM returning (C fp32, C bf16)");
  m.def("act_backward", &act_backward, "dZ = dY*act'(Y), + bf16 mirror");
  m.def("inv_perm_i32", &inv_perm_i32, "inverse permutation (int32)");
  m.def("radix_sort_index", &radix_sort_index,
        "bit-range radix sort -> (sorted, perm)");
  m.def("radix_sort_rec", &radix_sort_rec,
        "bit-range radix sort with [n,2] int32 records as payload -> "
        "(sorted, sorted_rec)",
        py::arg("keys"), py::arg("rec"), py::arg("end_bit"));
  m.def("onesweep_sort_rec", &onesweep_sort_rec,
        "single-purpose onesweep sort with [n,2] int32 records as payload "
        "-> (sorted, sorted_rec); same result as radix_sort_rec",
        py::arg("keys"), py::arg("rec"), py::arg("end_bit"),
        py::arg("status") = py::none());
  m.def("onesweep_sort_tile", &lightctr::onesweep_sort_tile,
        "entries per tile of onesweep_sort_rec");
  m.def("fm_records", &fm_records,
        "records of a CSR batch: rec[j] = (row of j, bits of vals[j])",
        py::arg("row_ptr"), py::arg("vals"));
  m.def("onesweep_sort_csr", &onesweep_sort_csr,
        "onesweep sort of a CSR batch's (fid, record) stream, the records "
        "made by the first scatter pass -> (sorted, sorted_rec)",
        py::arg("row_ptr"), py::arg("fids"), py::arg("vals"),
        py::arg("end_bit"), py::arg("status") = py::none());
  m.def("fm_forward_train_sorted", &fm_forward_train_sorted,
        "FM training forward and the record sort of the batch, side by side "
        "with overlap -> (loss, dpred, sumVX, sorted_fids, sorted_rec)",
        py::arg("row_ptr"), py::arg("fids"), py::arg("vals"), py::arg("W"),
        py::arg("V"), py::arg("label"), py::arg("scale"), py::arg("end_bit"),
        py::arg("reset") = py::none(), py::arg("status") = py::none(),
        py::arg("overlap") = true);
  m.def("colsum", &colsum, "bias gradient column sum");
  m.def("to_bf16", &to_bf16, "f32 -> bf16 convert");
  m.def("dense_adam", &dense_adam, "dense Adam + bf16 mirror refresh");
  m.def("dense_adagrad", &dense_adagrad,
        "dense Adagrad + bf16 mirror refresh");
  m.def("embed_gather", &embed_gather, "concat embedding gather -> bf16");
  m.def("embed_backward_emit", &embed_backward_emit,
        "per-entry embedding grads (gw, gv) for sorted apply");
  m.def("embed_bag_forward", &embed_bag_forward,
        "field-addressed pooled embedding bag -> bf16 concat [B, nf*K]");
  m.def("embed_bag_backward_emit", &embed_bag_backward_emit,
        "per-entry grads (gw, gv) of the field-addressed bag");
  m.def("deepfm_bag_forward", &deepfm_bag_forward,
        "DeepFM fused forward, concat addressed by field: (fm, sumVX, "
        "deep_in bf16)");
  m.def("deepfm_bag_backward_emit", &deepfm_bag_backward_emit,
        "DeepFM fused per-entry gradients, concat addressed by field: "
        "(gw, gv)");
  m.def("embed_bag_lds_bytes", &lightctr::embed_bag_lds_bytes,
        "dynamic LDS per block of the embed_bag / deepfm_bag forward",
        py::arg("nf"), py::arg("K"));
  m.def("wide_forward", &wide_forward, "LR wide forward sum");
  m.def("w2v_negsample_step", &w2v_negsample_step,
        "fused CBOW negative-sampling train step (Hogwild)");
  m.def("quantile_encode", &quantile_encode, "int8 quantile encode");
  m.def("quantile_decode", &quantile_decode, "int8 quantile decode");
  m.def("lowbit_encode", &lowbit_encode, "1/2-bit sign quantize");
  m.def("lowbit_decode", &lowbit_decode, "1/2-bit dequantize");
  m.def("gbm_hist", &gbm_hist, "GBM per-node (grad,hess) histograms");
  m.def("gbm_forest", &gbm_forest,
        "compiled-forest inference: margin / leaf id / leaf feature id");
  m.def("gbm_forest_chunk_capacity", &lightctr::gbm_forest_chunk_capacity,
        "nodes per LDS chunk of the forest kernel");
  m.def("gbm_forest_max_register_classes",
        &lightctr::gbm_forest_max_register_classes,
        "largest class count with register accumulators");
  m.def("gbm_forest_rows_per_grid", &lightctr::gbm_forest_rows_per_grid,
        "rows one trip of the clamped grid covers");
  m.def("nfm_forward", &nfm_forward,
        "NFM bi-interaction fwd (wide, sumVX, vec, vec_bf16)");
  m.def("nfm_backward_emit", &nfm_backward_emit,
        "NFM per-entry grads for sorted apply");
  m.def("deepfm_forward", &deepfm_forward,
        "DeepFM fused forward (fm, sumVX, deep_in bf16)");
  m.def("deepfm_backward_emit", &deepfm_backward_emit,
        "DeepFM per-entry grads (gw, gv) for sorted apply");
  m.def("bitmap_compact", &bitmap_compact, "touched bitmap -> fid list");
  m.def("wg_probe", &wg_probe, "wgrad staging/tr-read debug probe");
  m.def("gemm_bf16_variant", &gemm_bf16_variant,
        "launch one named GEMM body directly; returns [C] or [C, Cbf]");
  m.def("gemm_bf16_route", &gemm_bf16_route,
        "name of the GEMM body the default dispatch picks");
  m.def("gemm_wgrad_bf16", &gemm_wgrad_bf16,
        "K-major x K-major wgrad GEMM (tr16 fragment reads)");
  m.def("im2col_bf16", &im2col_bf16,
        "fused unfold -> bf16 GEMM operand [B*L, C*k*k]");
  m.def("col2im", &col2im, "conv data-grad fold (gather form)");
  m.def("auc_hist_add", &auc_hist_add,
        "atomic pos/neg histogram accumulate for AUC");
  m.def("auc_scan", &auc_scan,
        "device scan of the AUC histogram -> {correct, P, N}");
  m.def("fm_adagrad_apply", &fm_adagrad_apply, "sparse fused Adagrad");
  m.def("fm_ftrl_apply", &fm_ftrl_apply,
        "sparse fused FTRL-proximal (optionally Adagrad on V)",
        py::arg("uniq"), py::arg("count"), py::arg("W"), py::arg("V"),
        py::arg("zW"), py::arg("nW"), py::arg("zV"), py::arg("nV"),
        py::arg("gradW"), py::arg("gradV"), py::arg("alpha"),
        py::arg("beta"), py::arg("l1"), py::arg("l2"),
        py::arg("v_adagrad") = 0, py::arg("v_lr") = 0.05,
        py::arg("v_eps") = 1e-8, py::arg("v_l2") = 1e-5);
  m.def("pq_lut", &pq_lut,
        "PQ distance tables [nq, n_sub, ncb]; metric 0 = l2, 1 = ip",
        py::arg("Q"), py::arg("centroids"), py::arg("metric"));
  m.def("pq_adc_topk", &pq_adc_topk,
        "ADC scan of uint8 codes + top-k -> (ids int32, dist fp32) [nq, k]",
        py::arg("lut"), py::arg("codes"), py::arg("ncb"), py::arg("k"));
  m.def("flat_topk", &flat_topk,
        "exact scan (or per-query candidate list) + top-k -> (ids, dist)",
        py::arg("X"), py::arg("Q"), py::arg("metric"), py::arg("k"),
        py::arg("cand") = py::none());
  m.def("knn_max_k", &lightctr::knn_max_k, "largest k of the top-k kernels");
  m.def("knn_max_sub", &lightctr::knn_max_sub,
        "largest n_sub of pq_adc_topk");
  m.def("knn_max_dim", &lightctr::knn_max_dim, "largest dim of flat_topk");
  m.def("knn_slice_rows", &lightctr::knn_slice_rows,
        "rows per block slice for n rows and nq queries", py::arg("n"),
        py::arg("nq"));
  m.def("forest_candidates", &forest_candidates,
        "best-first walk of a flattened random-projection forest -> "
        "candidate ids int32 [nq, width], -1 padded",
        py::arg("planes"), py::arg("bias"), py::arg("child"),
        py::arg("roots"), py::arg("leaf_off"), py::arg("leaf_items"),
        py::arg("Q"), py::arg("search_k"), py::arg("width"));
  m.def("forest_queue", &lightctr::forest_queue,
        "queue entries per query of forest_candidates");
  m.def("forest_max_search", &lightctr::forest_max_search,
        "largest search_k of forest_candidates");
}
