// Declarations of the HIP kernel launchers, shared between the device
// translation units (*.hip, compiled by hipcc for gfx950) and the host
// bindings (bindings.cpp). hipStream_t == ihipStream_t* on ROCm.
#pragma once

struct ihipStream_t;

namespace lightctr {

// --- fm_kernels.hip ---
void fm_forward_launch(const int* row_ptr, const int* fids, const float* vals,
                       const float* W, const float* V, float* pred,
                       float* sumVX, int B, int K, ihipStream_t* stream);
void logloss_grad_launch(const float* pred, const float* label, float* loss,
                         float* dpred, float scale, int B,
                         ihipStream_t* stream);
void fm_backward_launch(const int* row_ptr, const int* fids, const float* vals,
                        const float* V, const float* sumVX, const float* dpred,
                        float* gradW, float* gradV, unsigned long long* touched,
                        int B, int K, ihipStream_t* stream);
void fm_backward_emit_launch(const int* row_ptr, const int* fids,
                             const float* vals, const float* V,
                             const float* sumVX, const float* dpred, float* gw,
                             float* gv, int B, int K, const int* pos,
                             ihipStream_t* stream);
void inv_perm_launch(const int* perm, int* inv, int n, ihipStream_t* stream);
void fm_sorted_apply_launch(const int* sorted_fids, const int* perm,
                            const float* gw, const float* gv, float* gradW,
                            float* gradV, unsigned long long* touched, int nnz,
                            int K, int opt_mode, float* V, float* W,
                            float* nW, float* zW, float* nV, float* zV,
                            float p0, float p1, float p2, float p3,
                            float q0, float q1, float q2,
                            int chunk, ihipStream_t* stream);
void fm_segment_apply_launch(const int* sorted_fids, const int* perm,
                             const int* piece_start, const int* n_pieces,
                             const float* gw, const float* gv, float* gradW,
                             float* gradV, int* spill, int* spill_count,
                             int spill_cap, int nnz, int K, int opt_mode,
                             float* V, float* W, float* nW, float* zW,
                             float* nV, float* zV, float p0, float p1,
                             float p2, float p3, float q0, float q1, float q2,
                             int num_cus, ihipStream_t* stream);
// rec: [n, 2] int32 records {row, bits of x}, 8-byte aligned; nullptr: the
// forward writes no records (fm_records_launch or the CSR sort makes them)
void fm_forward_train_launch(const int* row_ptr, const int* fids,
                             const float* vals, const float* W, const float* V,
                             const float* label, float scale, float* loss,
                             float* dpred, float* sumVX, int* rec, int B,
                             int K, int* reset, ihipStream_t* stream);
void fm_records_launch(const int* row_ptr, const float* vals, int* rec, int B,
                       ihipStream_t* stream);
void fm_segment_recompute_launch(
    const int* sorted_fids, const int* rec, const float* sumVX,
    const float* dpred, int B, const int* piece_start, const int* n_pieces,
    float* gradW, float* gradV, int* spill, int* spill_count, int spill_cap,
    int nnz, int K, int opt_mode, float* V, float* W, float* nW, float* zW,
    float* nV, float* zV, float p0, float p1, float p2, float p3, float q0,
    float q1, float q2, int num_cus, ihipStream_t* stream);
// tile-local segment reduce: needs cap <= fm_segment_tile() and the tile a
// multiple of cap; no work list
int fm_segment_tile();
int fm_segment_split();
void fm_segment_tile_launch(const int* sorted_fids, const int* rec,
                            const float* sumVX, const float* dpred, int B,
                            int cap, float* gradW, float* gradV, int* spill,
                            int* spill_count, int spill_cap, int nnz, int K,
                            int opt_mode, float* V, float* W, float* nW,
                            float* zW, float* nV, float* zV, float p0,
                            float p1, float p2, float p3, float q0, float q1,
                            float q2, ihipStream_t* stream);
void bitmap_compact_launch(unsigned long long* bitmap, int nwords,
                           int* out_fids, int* out_count, int cap,
                           ihipStream_t* stream);

// --- ffm_kernels.hip ---
void ffm_forward_launch(const int* row_ptr, const int* fields, const int* fids,
                        const float* vals, const float* W, const float* V,
                        float* pred, int nfields, int B, int K,
                        ihipStream_t* stream);
void ffm_backward_launch(const int* row_ptr, const int* fields,
                         const int* fids, const float* vals, const float* V,
                         const float* dpred, float* gradW, float* gradV,
                         unsigned long long* touched, int nfields, int B,
                         int K, ihipStream_t* stream);

void ffm_sorted_backward_launch(const int* sorted_fids, const int* perm,
                                const int* row_of_entry, const int* row_ptr,
                                const int* fields, const int* fids,
                                const float* vals, const float* V,
                                const float* dpred, float* gradW,
                                float* gradV, unsigned long long* touched,
                                int nfields, int nnz, int K,
                                ihipStream_t* stream);
void row_index_launch(const int* row_ptr, int* row_idx, int B,
                      ihipStream_t* stream);
void ffm_block_emit_launch(const int* row_of_entry, const int* row_ptr,
                           const int* fields, const int* fids,
                           const float* vals, const float* V,
                           const float* dpred, float* gblocks, float* gw,
                           int nfields, int nnz, int K, ihipStream_t* stream);
void ffm_forward_pp_launch(const int* row_ptr, const int* fields,
                           const int* fids, const float* vals,
                           const float* W, const void* V, int v_bf16,
                           float* pred, int nfields, int B, int K,
                           ihipStream_t* stream);
bool ffm_staged_eligible(int nfields, int K, int maxn);
// dynamic LDS of ffm_sorted_backward / ffm_block_emit and of
// ffm_blocks_apply, and the per-block LDS limit of the current device
long ffm_block_lds_bytes(int nfields, int K);
long ffm_blocks_apply_lds_bytes(int D);
long ffm_max_lds_per_block();
void ffm_fwd_staged_launch(const int* row_ptr, const int* fields,
                           const int* fids, const float* vals, const float* W,
                           const float* V, float* pred, int nfields, int B,
                           int maxn, int K, ihipStream_t* stream);
void ffm_row_emit_launch(const int* row_ptr, const int* fields,
                         const int* fids, const float* vals, const void* V,
                         int v_bf16, const float* dpred, void* gblocks,
                         float* gw, int nfields, int B, int maxn, int K,
                         float scale, ihipStream_t* stream);
void ffm_blocks_apply_f16_launch(const int* sorted_fids, const int* perm,
                                 const void* gblocks, const float* gw,
                                 float* gradW, float* gradV,
                                 unsigned long long* touched, int D, int nnz,
                                 float inv_scale, int opt_mode, float* V,
                                 float* W, float* nW, float* zW, float* nV,
                                 void* Vh, float p0, float p1, float p2,
                                 float p3, float q0, float q1, float q2,
                                 ihipStream_t* stream);
void ffm_blocks_apply_launch(const int* sorted_fids, const int* perm,
                             const float* gblocks, const float* gw,
                             float* gradW, float* gradV,
                             unsigned long long* touched, int D, int nnz,
                             ihipStream_t* stream);

// --- misc_kernels.hip (generic sparse fused optimizers; D = per-feature
// latent size, runtime) ---
void ps_apply_launch(const long* lidx, int n, const float* gW,
                     const float* gV, float* W, float* V, float* nW,
                     float* nV, float* shadowW, float* shadowV, int K,
                     int updater, float lr, float lam, float eps,
                     ihipStream_t* stream);
void auc_hist_add_launch(const float* pred, const float* label, long n,
                         unsigned int* hist, int buckets,
                         ihipStream_t* stream);
void auc_scan_launch(const unsigned int* hist, int buckets, double* out,
                     ihipStream_t* stream);
void sparse_adagrad_apply_launch(const int* uniq, const int* count, float* W,
                                 float* V, float* nW, float* nV, float* gradW,
                                 float* gradV, float lr, float eps, float l2,
                                 int capacity, int D, void* Vh,
                                 ihipStream_t* stream);
void sparse_ftrl_apply_launch(const int* uniq, const int* count, float* W,
                              float* V, float* zW, float* nW, float* zV,
                              float* nV, float* gradW, float* gradV,
                              float alpha, float beta, float l1, float l2,
                              int capacity, int D, int v_adagrad, float v_lr,
                              float v_eps, float v_l2, void* Vh,
                              ihipStream_t* stream);
void fm_adagrad_apply_launch(const int* uniq, const int* count, float* W,
                             float* V, float* nW, float* nV, float* gradW,
                             float* gradV, float lr, float eps, float l2,
                             int capacity, int K, ihipStream_t* stream);
void fm_ftrl_apply_launch(const int* uniq, const int* count, float* W,
                          float* V, float* zW, float* nW, float* zV, float* nV,
                          float* gradW, float* gradV, float alpha, float beta,
                          float l1, float l2, int capacity, int K,
                          int v_adagrad, float v_lr, float v_eps, float v_l2,
                          ihipStream_t* stream);

// --- gemm_wgrad_kernels.hip ---
bool gemm_wgrad_eligible(int M, int N, int K, int transA, int transB);
// split_z: requested split-K fan-out, 0 = one block per output tile
int gemm_wgrad_default_split(int M, int N, int K);
void gemm_wgrad_bf16_launch_cfg(const void* At, const void* Bt, float* C,
                                int M, int N, int K, int split_z,
                                ihipStream_t* stream);
void gemm_wgrad_bf16_launch(const void* At, const void* Bt, float* C, int M,
                            int N, int K, ihipStream_t* stream);
void wg_probe_launch(const void* g, int ld, void* out_lds, float* out_frag,
                     int mode, ihipStream_t* stream);

// --- gemm_kernels.hip ---
// Every GEMM launcher comes in two parts: `*_launch_cfg` takes the body's
// configuration explicitly (the K-tail flag alone is derived from K), and
// `*_default_cfg` / `*_default_split` give the environment's choice (knobs
// read once per process into function-local statics; the APIPE knobs per
// call). The default dispatch is gemm_bf16_pick, which asks the latter,
// then gemm_bf16_run, which calls the former.
enum GemmBody {
  GEMM_BODY_GENERIC = 0,
  GEMM_BODY_256,
  GEMM_BODY_P8,
  GEMM_BODY_V2,
  GEMM_BODY_N128,
  GEMM_BODY_WGRAD128,
  GEMM_BODY_GEMV_N1,
  GEMM_BODY_WROWSUM_M1,
  GEMM_BODY_SMALL_WGRAD,
  GEMM_BODY_OUTER_K1,
};
struct GemmRoute {
  int body = GEMM_BODY_GENERIC;
  int split_z = 0;     // generic / wgrad128: split-K fan-out, 0 = none
  int pipe = 0;        // gemm256: A-read schedule 0 / 1 / 2
  bool burst = false;  // gemm256
  bool lite = true;    // p8: 2 barriers per K-tile (false: 8)
  bool xcd = false;    // p8: XCD tile remap
  bool apipe = false;  // p8: pipelined A reads (lite, no xcd)
};
GemmRoute gemm_bf16_pick(int M, int N, int K, int transA, int transB,
                         bool has_bias, int act, bool has_cbf,
                         bool aligned16);
void gemm_bf16_run(const GemmRoute& r, const void* A, const void* Bst,
                   const float* bias, float* C, void* Cbf, int M, int N,
                   int K, int transA, int transB, int act,
                   ihipStream_t* stream);
void gemm_bf16_launch(const void* A, const void* Bst, const float* bias,
                      float* C, void* Cbf, int M, int N, int K, int transA,
                      int transB, int act, ihipStream_t* stream);
int gemm_generic_default_split(int M, int N, int K, bool plain);
void gemm_generic_bf16_launch_cfg(const void* A, const void* Bst,
                                  const float* bias, float* C, void* Cbf,
                                  int M, int N, int K, int transA,
                                  int transB, int act, int split_z,
                                  ihipStream_t* stream);

bool gemm256_eligible(int M, int N, int K, int transA, int transB);
void gemm256_default_cfg(int K, bool* burst, int* pipe);
void gemm256_bf16_launch_cfg(const void* A, const void* Bst,
                             const float* bias, float* C, void* Cbf, int M,
                             int N, int K, int act, bool burst, int pipe,
                             ihipStream_t* stream);
bool gemm256p8_eligible(int M, int N, int K, int transA, int transB);
void gemm256p8_default_cfg(bool* lite, bool* xcd, bool* apipe);
void gemm256p8_bf16_launch_cfg(const void* A, const void* Bst,
                               const float* bias, float* C, void* Cbf, int M,
                               int N, int K, int act, bool lite, bool xcd,
                               bool apipe, ihipStream_t* stream);
bool gemm256v2_eligible(int M, int N, int K, int transA, int transB);
void gemm256v2_bf16_launch(const void* A, const void* Bst, const float* bias,
                           float* C, void* Cbf, int M, int N, int K, int act,
                           ihipStream_t* stream);
bool gemm256n128_eligible(int M, int N, int K, int transA, int transB);
void gemm256n128_bf16_launch(const void* A, const void* Bst,
                             const float* bias, float* C, void* Cbf, int M,
                             int N, int K, int act, ihipStream_t* stream);

// --- nn_kernels.hip ---
void small_wgrad_launch(const void* Ast, const void* Bst, float* C, int M,
                        int N, int K, ihipStream_t* stream);
void im2col_bf16_launch(const float* x, void* col, int B, int C, int H,
                        int W, int k, int stride, int pad, int OH, int OW,
                        ihipStream_t* stream);
void col2im_launch(const float* dcol, float* dx, int B, int C, int H, int W,
                   int k, int stride, int pad, int OH, int OW,
                   ihipStream_t* stream);
void gemv_n1_launch(const void* A, const void* b, const float* bias,
                    float* C, void* Cbf, int M, int K, int act,
                    ihipStream_t* stream);
void wrowsum_m1_launch(const void* a, const void* Bst, float* C, int K,
                       int N, ihipStream_t* stream);
void outer_k1_launch(const void* A, const void* Bst, const float* bias,
                     float* C, void* Cbf, long M, long N, int act,
                     ihipStream_t* stream);
void act_backward_launch(const float* dY, const float* Y, float* dZ,
                         void* dZbf, long n, int act, ihipStream_t* stream);
void colsum_launch(const float* dZ, float* db, int M, int N,
                   ihipStream_t* stream);
void to_bf16_launch(const float* x, void* y, long n, ihipStream_t* stream);
void dense_adam_launch(float* W, const float* grad, float* m_t, float* v_t,
                       void* Wbf, void* Wtbf, int rows, int cols, float lr,
                       float beta1, float beta2, float eps, float bc1,
                       float bc2, float l2, ihipStream_t* stream);
void dense_adagrad_launch(float* W, const float* grad, float* n_t, void* Wbf,
                          void* Wtbf, int rows, int cols, float lr, float eps,
                          float l2, ihipStream_t* stream);

// --- embed_kernels.hip ---
void embed_gather_launch(const int* row_ptr, const int* fids,
                         const float* vals, const float* E, void* out_bf,
                         int nf, int B, int K, ihipStream_t* stream);
void embed_backward_emit_launch(const int* row_ptr, const float* vals,
                                const float* dOut, const float* dwide,
                                float* gv, float* gw, int nf, int B, int K,
                                ihipStream_t* stream);
void wide_forward_launch(const int* row_ptr, const int* fids,
                         const float* vals, const float* W, float* wide,
                         int B, ihipStream_t* stream);
void nfm_forward_launch(const int* row_ptr, const int* fids, const float* vals,
                        const float* W, const float* V, float* wide,
                        float* sumVX, float* vec, void* vec_bf, int B, int K,
                        ihipStream_t* stream);
void w2v_negsample_launch(float* E, float* O, const long* centers,
                          const long* ctx, const long* negs, float* loss,
                          int B, int C, int N, int D, float lr, float scale,
                          ihipStream_t* stream);
void nfm_backward_emit_launch(const int* row_ptr, const int* fids,
                              const float* vals, const float* V,
                              const float* sumVX, const float* dvec,
                              const float* dwide, float* gw, float* gv, int B,
                              int K, ihipStream_t* stream);

// --- deepfm_kernels.hip ---
void deepfm_forward_launch(const int* row_ptr, const int* fids,
                           const float* vals, const float* W, const float* E,
                           void* out_bf, float* sumVX, float* fm, int nf,
                           int B, int K, ihipStream_t* stream);
void deepfm_backward_emit_launch(const int* row_ptr, const int* fids,
                                 const float* vals, const float* E,
                                 const float* sumVX, const float* dDeep,
                                 const float* dpred, float* gw, float* gv,
                                 int nf, int B, int K, ihipStream_t* stream);

// --- embed_bag_kernels.hip ---
long embed_bag_lds_bytes(int nf, int K);
void embed_bag_forward_launch(const int* row_ptr, const int* fields,
                              const int* fids, const float* vals,
                              const float* E, void* out_bf, int nf,
                              int pooling, int B, int K,
                              ihipStream_t* stream);
void embed_bag_backward_emit_launch(const int* row_ptr, const int* fields,
                                    const float* vals, const float* dOut,
                                    const float* dwide, float* gw, float* gv,
                                    int nf, int pooling, int B, int K,
                                    ihipStream_t* stream);
void deepfm_bag_forward_launch(const int* row_ptr, const int* fields,
                               const int* fids, const float* vals,
                               const float* W, const float* E, void* out_bf,
                               float* sumVX, float* fm, int nf, int pooling,
                               int B, int K, ihipStream_t* stream);
void deepfm_bag_backward_emit_launch(const int* row_ptr, const int* fields,
                                     const int* fids, const float* vals,
                                     const float* E, const float* sumVX,
                                     const float* dDeep, const float* dpred,
                                     float* gw, float* gv, int nf,
                                     int pooling, int B, int K,
                                     ihipStream_t* stream);

// --- codec_kernels.hip ---
void quantile_encode_launch(const float* x, unsigned char* code,
                            const float* table, int levels, long n,
                            ihipStream_t* stream);
void quantile_decode_launch(const unsigned char* code, float* x,
                            const float* table, int levels, long n,
                            ihipStream_t* stream);
void lowbit_encode_launch(const float* x, unsigned int* words, float thresh,
                          int bits, long n, ihipStream_t* stream);
void lowbit_decode_launch(const unsigned int* words, float* x, float lo,
                          float hi, int bits, long n, ihipStream_t* stream);

// --- ps_dense_kernels.hip (PS dense-table slab; wire 0=fp32 1=fp16 2=u8
// codes; flags = {corrupt-push flag, dropped counter}) ---
void ps_dense_check_launch(const void* payload, int wire, const float* scale,
                           const float* table, int levels, long n,
                           int* flags, ihipStream_t* stream);
void ps_dense_apply_launch(const void* payload, int wire, const float* scale,
                           const float* table, int levels, float* slab,
                           float* acc, float* shadow, long n, int updater,
                           float lr, float lam, float eps, int* flags,
                           ihipStream_t* stream);
void ps_dense_pack_launch(const float* slab, void* out, int fp16,
                          float* shadow, long n, ihipStream_t* stream);

// --- sort_kernels.hip ---
void iota_i32_launch(int* out, int n, ihipStream_t* stream);
unsigned long radix_sort_pairs_i32_temp_bytes(int n, int end_bit);
void radix_sort_pairs_i32_launch(void* temp, unsigned long temp_bytes,
                                 const int* keys_in, int* keys_out,
                                 const int* vals_in, int* vals_out, int n,
                                 int end_bit, ihipStream_t* stream);
// 8-byte payload: rec_in / rec_out are [n, 2] int32, 8-byte aligned
unsigned long radix_sort_pairs_rec_temp_bytes(int n, int end_bit);
void radix_sort_pairs_rec_launch(void* temp, unsigned long temp_bytes,
                                 const int* keys_in, int* keys_out,
                                 const int* rec_in, int* rec_out, int n,
                                 int end_bit, ihipStream_t* stream);
// single-purpose onesweep sort of (key, 8-byte record): one memset, one
// histogram kernel, one scatter kernel per 8-bit pass. 1 <= end_bit <= 31,
// n < 2^30. work: onesweep_sort_work_bytes() bytes; keys_tmp / rec_tmp: n
// entries each, used from two passes on; status: caller-owned word, a
// nonzero code is ORed in if a look-back spin gives up (never zeroed here)
int onesweep_sort_tile();
unsigned long onesweep_sort_work_bytes(int n, int end_bit);
void onesweep_sort_rec_launch(void* work, const int* keys_in, int* keys_out,
                              int* keys_tmp, const int* rec_in, int* rec_out,
                              int* rec_tmp, int n, int end_bit, int* status,
                              ihipStream_t* stream);
// the same sort of a CSR batch's (fid, {row, bits of x}) stream, n =
// row_ptr[B]: the first scatter pass reads keys_in and vals and finds each
// entry's row in row_ptr, so no record exists in CSR order and nothing of the
// sort depends on the model. keys_tmp / rec_tmp from two passes on. Kernels
// only: a one-block kernel zeroes the control block in place of the memset
void onesweep_sort_csr_launch(void* work, const int* row_ptr,
                              const int* keys_in, const float* vals, int B,
                              int* keys_out, int* keys_tmp, int* rec_out,
                              int* rec_tmp, int n, int end_bit, int* status,
                              ihipStream_t* stream);
// work list of the segment backward: compacted piece starts of a sorted
// stream + their count (device side); zero_me (optional) is reset to 0
unsigned long segment_worklist_temp_bytes(int n);
void segment_worklist_launch(void* temp, unsigned long temp_bytes,
                             const int* sorted, int n, int cap,
                             int* piece_start, int* n_pieces, int* zero_me,
                             ihipStream_t* stream);

// --- gbm_kernels.hip ---
void gbm_hist_launch(const unsigned char* bins, const float* grad,
                     const float* hess, const int* node_of_row, float* hist,
                     int N, int D, int n_nodes, ihipStream_t* stream);
// compiled-forest inference; mode 0 = margin (out fp32 [N,K]), 1 = leaf id,
// 2 = leaf feature id (out int32 [N,T]); nodes/chunks are 16-byte records
int gbm_forest_chunk_capacity();
int gbm_forest_max_register_classes();
long gbm_forest_rows_per_grid();
void gbm_forest_launch(const float* X, const void* nodes, const int* tree_off,
                       const int* tree_class, const int* leaf_base,
                       const void* chunks, int n_chunks, void* out, long N,
                       int D, int T, int K, int max_depth, int fid_offset,
                       int mode, ihipStream_t* stream);

// --- knn_kernels.hip ---
// top-k search (predict/knn.py): ids int32 / dist fp32 [nq, k] in ascending
// (dist, id) order, (-1, +inf) past the row count. `partial` is the
// [nq, n_slices, k] 8-byte key buffer of the slices, merged by
// knn_merge_launch when n_slices > 1 (dedup: equal keys count once).
int knn_max_k();
int knn_max_sub();
int knn_max_dim();
long knn_slice_rows(long n, long nq);
long pq_adc_lds_bytes(int n_sub, int ncb);
void pq_lut_launch(const float* Q, const float* C, float* lut, long nq,
                   int n_sub, int ncb, int d_sub, int ip,
                   ihipStream_t* stream);
void pq_adc_topk_launch(const float* lut, const unsigned char* codes,
                        long stride, long N, long nq, int n_sub, int ncb,
                        int k, long slice_rows, int n_slices, void* partial,
                        int* ids, float* dist, ihipStream_t* stream);
void flat_topk_launch(const float* X, long stride, long N, int dim,
                      const float* Q, long nq, const int* cand, long n_items,
                      int ip, int k, long slice_rows, int n_slices,
                      void* partial, int* ids, float* dist,
                      ihipStream_t* stream);
void knn_merge_launch(const void* partial, long nq, int n_slices, int k,
                      int dedup, int* ids, float* dist, ihipStream_t* stream);
// random-projection forest walk (predict/rp_forest.py): cand int32
// [nq, width], per query the items of the leaves a best-first search
// reaches until search_k ids are written, then -1
int forest_queue();
int forest_max_search();
void forest_candidates_launch(const float* planes, const float* bias,
                              const int* child, const int* roots,
                              const int* leaf_off, const int* leaf_items,
                              const float* Q, int* cand, long nq, int dim,
                              int n_inner, int n_leaves, int T, long total,
                              int search_k, long width, ihipStream_t* stream);

}  // namespace lightctr
