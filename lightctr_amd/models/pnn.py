"""PNN (inner-product layer in front of the MLP) — MI355X-native trainer.

Qu et al., "Product-based Neural Networks for User Response Prediction" (ICDM
2016), the inner-product variant with the product layer written out in full
(every pair's inner product feeds the first dense layer, the paper's
l_p^n = sum_ij W^n_ij g_ij without its factorised approximation); the same
operation as DLRM's dot interaction. Wide&Deep's concat row x0 [B, nf*K] (both
layouts, both poolings), viewed as e [B, nf, K]:

    g[b, p(i,j)] = e_i . e_j   (i < j, row-major upper triangle)
    z[b] = [x0[b], g[b], 0 .. 0],  Dz = nf K + nf (nf-1)/2 up to a multiple of 8
    score = wide + MLP(z)

Goes beyond the reference inventory. On the GPU the layer is
ops/csrc/pnn_kernels.hip (pnn_impl="hip"): one launch writes the MLP's bf16
operand row whole, one launch turns the MLP's input gradient into the concat's.
pnn_impl="torch" composes both from tensor ops (ops/pnn_ref.py with the
kernels' rounding points) and is the baseline arm. The CPU path is
ops/pnn_ref.py in fp32. The layer has no parameters: the sparse tail, the
optimisers and the checkpoint are Wide&Deep's, the first dense layer is Dz
wide.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import fm_ref, pnn_ref
from ..ops._extension import require_hip_ops
from .wide_deep import WideDeepHyper, WideDeepModel, WideDeepTrainer


@dataclass
class PNNHyper(WideDeepHyper):
    pass


class PNNModel(WideDeepModel):
    def __init__(self, hyper: PNNHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22, pnn_impl: str = "hip"):
        nf, K = hyper.num_fields, hyper.k
        if not 2 <= nf <= 64:
            raise ValueError(f"num_fields must be in 2..64, got {nf}")
        if K not in (4, 8, 16, 32, 64):
            raise ValueError(f"k must be 4, 8, 16, 32 or 64, got {K}")
        if nf * K > 1024:
            raise ValueError(
                f"num_fields*k must be at most 1024, got {nf * K}")
        if pnn_impl not in ("hip", "torch"):
            raise ValueError(f"unknown pnn_impl {pnn_impl!r}")
        self.pnn_impl = pnn_impl
        super().__init__(hyper, device=device, max_batch_nnz=max_batch_nnz)

    def _mlp_in_dim(self):
        return pnn_ref.pnn_dims(self.h.num_fields, self.h.k)[1]

    # ---- the product layer: z [B, Dz] (bf16 on the GPU) ----
    def _pnn_forward(self, x0):
        nf = self.h.num_fields
        if self._gpu and self.pnn_impl == "hip":
            return require_hip_ops().pnn_forward(x0, nf)
        if self._gpu:
            return pnn_ref.pnn_forward_ref(x0.float(), nf,
                                           rounding="bf16").bfloat16()
        return pnn_ref.pnn_forward_ref(x0, nf)

    # ---- dDeep [B, nf*K] from z and the MLP's input gradient ----
    def _pnn_backward(self, z, dz):
        nf, K = self.h.num_fields, self.h.k
        if self._gpu and self.pnn_impl == "hip":
            return require_hip_ops().pnn_backward(z, dz, nf, K)
        if self._gpu:
            return pnn_ref.pnn_backward_ref(z.float(), dz, nf, K,
                                            rounding="bf16")
        return pnn_ref.pnn_backward_ref(z, dz, nf, K)

    def _score(self, wide, deep_in, train):
        self._z = self._pnn_forward(deep_in)
        return wide + self.mlp.forward(self._z, train=train)[:, 0]

    def train_step(self, row_ptr, fids, vals, labels, fields=None):
        B = row_ptr.numel() - 1
        scale = 1.0 / B
        fields = self._fields(fields)
        if self._gpu:
            pred, _ = self._forward_gpu(row_ptr, fids, vals, fields=fields)
            loss, dpred = require_hip_ops().logloss_grad(pred, labels, scale)
        else:
            pred, _ = self._forward_cpu(row_ptr, fids, vals, fields=fields)
            loss, dpred = fm_ref.logloss_grad_ref(pred, labels, scale)
        dz = self.mlp.backward(dpred.unsqueeze(1)).contiguous()
        dDeep = self._pnn_backward(self._z, dz)
        tail = self._sparse_step_gpu if self._gpu else self._sparse_step_cpu
        tail(row_ptr, fids, vals, fields, dDeep, dpred)
        self.mlp.apply_grads()
        return loss


class PNNTrainer(WideDeepTrainer):
    def __init__(self, dataset, hyper: PNNHyper, device="cpu",
                 batch_size=256, epochs=5, pnn_impl="hip"):
        self.ds = dataset
        self.model = PNNModel(hyper, device=device, pnn_impl=pnn_impl)
        self.batch_size, self.epochs = batch_size, epochs
        self.device = torch.device(device)
