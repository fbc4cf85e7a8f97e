"""Deep & Cross Network — MI355X-native trainer.

Wide&Deep's concat row x0 [B, nf*K] (both layouts) feeds the MLP and, beside
it, L cross layers in the vector form of Wang et al., "Deep & Cross Network
for Ad Click Predictions" (ADKDD 2017):

    x_{l+1} = x0 (x_l . w_l) + b_l + x_l         l = 0 .. L-1
    score   = wide + MLP(x0) + x_L . u

u together with the MLP's last linear layer is the paper's combination layer
over [x_L ; h]. Goes beyond the reference inventory. On the GPU the cross
term is ops/csrc/dcn_kernels.hip: one pass over the bf16 concat forward, one
over it and dDeep backward (cross_impl="hip"); cross_impl="torch" composes
the layers from tensor ops and is the baseline arm. The CPU path is
ops/dcn_ref.py. The sparse tail is Wide&Deep's; Wc, bc and u take the dense
Adam / Adagrad step of the MLP (mlp_optimizer, mlp_lr).
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import dcn_ref, fm_ref
from ..ops._extension import require_hip_ops
from .embed_bag import load_checkpoint
from .wide_deep import WideDeepHyper, WideDeepModel, WideDeepTrainer


@dataclass
class DCNHyper(WideDeepHyper):
    cross_layers: int = 3


class DCNModel(WideDeepModel):
    _CROSS = ("Wc", "bc", "u")

    def __init__(self, hyper: DCNHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22, cross_impl: str = "hip"):
        L, d = hyper.cross_layers, hyper.num_fields * hyper.k
        if not 1 <= L <= 8:
            raise ValueError(f"cross_layers must be in 1..8, got {L}")
        if cross_impl not in ("hip", "torch"):
            raise ValueError(f"unknown cross_impl {cross_impl!r}")
        super().__init__(hyper, device=device, max_batch_nnz=max_batch_nnz)
        self.cross_impl = cross_impl
        if self._gpu and cross_impl == "hip":
            ops = require_hip_ops()
            need = ops.dcn_cross_lds_bytes(L, d)
            have = ops.ffm_max_lds_per_block()
            if need > have:
                raise ValueError(
                    f"cross_layers={L}, num_fields*k={d}: the DCN kernels "
                    f"need {need} bytes of LDS per block, the device gives "
                    f"{have}")
        g = torch.Generator().manual_seed(hyper.seed + 7919)
        sd = d ** -0.5  # N(0, 1/d): x . w is of the size of one entry of x
        self.Wc = (torch.randn(L, d, generator=g) * sd).to(self.device)
        self.u = (torch.randn(d, generator=g) * sd).to(self.device)
        self.bc = torch.zeros(L, d, device=self.device)
        # optimizer state of the three, in the MLP's updater
        self._adam = hyper.mlp_optimizer == "adam"
        self.cross_step = 0
        for n in self._CROSS:
            z = torch.zeros_like(getattr(self, n))
            setattr(self, "m_" + n, z)             # Adam m / Adagrad n
            if self._adam:
                setattr(self, "v_" + n, z.clone())

    # ---- cross term, forward: (cross [B], what the backward needs) ----
    def _cross_forward(self, x0):
        if not self._gpu:
            C, q = dcn_ref.dcn_cross_prep_ref(self.Wc, self.bc, self.u)
            cross, P = dcn_ref.dcn_cross_forward_ref(x0, self.Wc, self.u, q)
            return cross, (x0, P, q, C)
        if self.cross_impl == "torch":
            return dcn_ref.dcn_layers_forward(x0.float(), self.Wc, self.bc,
                                              self.u)
        ops = require_hip_ops()
        C, q = ops.dcn_cross_prep(self.Wc, self.bc, self.u)
        cross, P = ops.dcn_cross_forward(x0, self.Wc, self.u, q)
        return cross, (x0, P, q, C)

    # ---- backward: dDeep += dx0 in place, the dense gradients kept ----
    def _cross_backward(self, saved, dpred, dDeep):
        if self._gpu and self.cross_impl == "hip":
            x0, P, q, C = saved
            self._dcross = require_hip_ops().dcn_cross_backward(
                x0, P, self.Wc, self.u, q, C, dpred, dDeep)
            return
        if self._gpu:
            dx0, *self._dcross = dcn_ref.dcn_layers_backward(
                saved, self.Wc, self.u, dpred)
        else:
            x0, P, q, C = saved
            dx0, *self._dcross = dcn_ref.dcn_cross_backward_ref(
                x0, P, self.Wc, self.u, q, C, dpred)
        dDeep += dx0

    def _cross_apply(self):
        lr, eps = self.h.mlp_lr, 1e-8
        self.cross_step += 1
        ops = require_hip_ops() if self._gpu else None
        for n, gr in zip(self._CROSS, self._dcross):
            p, m = getattr(self, n), getattr(self, "m_" + n)
            if self._adam:
                v, b1, b2 = getattr(self, "v_" + n), 0.9, 0.999
                if ops:
                    ops.dense_adam(p, gr, m, v, None, None, lr, b1, b2, eps,
                                   self.cross_step, 0.0)
                    continue
                m.mul_(b1).add_(gr, alpha=1 - b1)
                v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
                p.sub_(lr * (m / (1 - b1 ** self.cross_step)) /
                       ((v / (1 - b2 ** self.cross_step)).sqrt() + eps))
            elif ops:
                ops.dense_adagrad(p, gr, m, None, None, lr, eps, 0.0)
            else:
                m.add_(gr * gr)
                p.sub_(lr * gr / (m + eps).sqrt())

    def _score(self, wide, deep_in, train):
        deep = self.mlp.forward(deep_in, train=train)
        cross, self._saved = self._cross_forward(deep_in)
        return wide + deep[:, 0] + cross

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
        dDeep = self.mlp.backward(dpred.unsqueeze(1)).contiguous()
        self._cross_backward(self._saved, dpred, dDeep)
        tail = self._sparse_step_gpu if self._gpu else self._sparse_step_cpu
        tail(row_ptr, fids, vals, fields, dDeep, dpred)
        self.mlp.apply_grads()
        self._cross_apply()
        return loss

    def _cross_state(self):
        names = list(self._CROSS) + ["m_" + n for n in self._CROSS]
        if self._adam:
            names += ["v_" + n for n in self._CROSS]
        return names

    def state_dict(self):
        d = super().state_dict()
        d.update({n: getattr(self, n) for n in self._cross_state()})
        d["cross_step"] = torch.tensor(self.cross_step)
        return d

    def load(self, path):
        d = load_checkpoint(path, self.device)
        super().load(d)
        for n in self._cross_state():
            getattr(self, n).copy_(d[n])
        self.cross_step = int(d["cross_step"])


class DCNTrainer(WideDeepTrainer):
    def __init__(self, dataset, hyper: DCNHyper, device="cpu",
                 batch_size=256, epochs=5, cross_impl="hip"):
        self.ds = dataset
        self.model = DCNModel(hyper, device=device, cross_impl=cross_impl)
        self.batch_size, self.epochs = batch_size, epochs
        self.device = torch.device(device)
