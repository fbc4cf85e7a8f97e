"""DCN-v2 (low-rank matrix cross layers) — MI355X-native trainer.

Wide&Deep's concat row x0 [B, d = nf*K] (both layouts) feeds the MLP and,
beside it, L cross layers in the low-rank matrix form of Wang et al., "DCN V2:
Improved Deep & Cross Network" (WWW 2021), W_l = U_l V_l^T of rank r:

    T_l     = x_l V_l
    x_{l+1} = x0 * (T_l U_l^T + b_l) + x_l       l = 0 .. L-1
    score   = wide + MLP(x0) + x_L . u

Goes beyond the reference inventory. On the GPU the cross term is
ops/csrc/dcn2_kernels.hip: one launch for all L layers forward, one backward,
both on the bf16 matrix unit with the row stream held in fp32 accumulators
(cross_impl="hip"); the weight gradients dU_l = G_l^T T_l and dV_l = X_l^T S_l
go through the MLP's wgrad GEMM. cross_impl="torch" composes the layers from
tensor ops (ops/dcn2_ref.py with the kernels' rounding points, on the same
bf16 weight mirrors) and is the baseline arm. The CPU path is ops/dcn2_ref.py
in fp32. The sparse tail is Wide&Deep's; U, V, bc and u take the dense Adam /
Adagrad step of the MLP (mlp_optimizer, mlp_lr), which also refreshes the
bf16 mirrors of U and V in both operand layouts ([d, r] and [r, d] a layer).
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import dcn2_ref, fm_ref
from ..ops._extension import require_hip_ops
from .embed_bag import load_checkpoint
from .wide_deep import WideDeepHyper, WideDeepModel, WideDeepTrainer


@dataclass
class DCNv2Hyper(WideDeepHyper):
    cross_layers: int = 3
    cross_rank: int = 64


class DCNv2Model(WideDeepModel):
    _CROSS = ("U", "V", "bc", "u")

    def __init__(self, hyper: DCNv2Hyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22, cross_impl: str = "hip"):
        L, r, d = hyper.cross_layers, hyper.cross_rank, \
            hyper.num_fields * hyper.k
        if not 1 <= L <= 8:
            raise ValueError(f"cross_layers must be in 1..8, got {L}")
        if r % 16 or not 16 <= r <= 128:
            raise ValueError(
                f"cross_rank must be a multiple of 16 in 16..128, got {r}")
        if d % 4 or not 4 <= d <= 1024:
            raise ValueError(
                f"num_fields*k must be a multiple of 4 in 4..1024, got {d}")
        if cross_impl not in ("hip", "torch"):
            raise ValueError(f"unknown cross_impl {cross_impl!r}")
        super().__init__(hyper, device=device, max_batch_nnz=max_batch_nnz)
        self.cross_impl = cross_impl
        if self._gpu and cross_impl == "hip":
            ops = require_hip_ops()
            need = ops.dcn2_cross_lds_bytes(L, d, r)
            have = ops.ffm_max_lds_per_block()
            if need > have:
                raise ValueError(
                    f"cross_layers={L}, num_fields*k={d}, cross_rank={r}: "
                    f"the DCN-v2 kernels need {need} bytes of LDS per block, "
                    f"the device gives {have}")
        g = torch.Generator().manual_seed(hyper.seed + 7919)
        # x V is of the size of one entry of x, and so is T U^T
        self.V = (torch.randn(L, d, r, generator=g) * d ** -0.5).to(
            self.device)
        self.U = (torch.randn(L, d, r, generator=g) * r ** -0.5).to(
            self.device)
        self.u = (torch.randn(d, generator=g) * d ** -0.5).to(self.device)
        self.bc = torch.zeros(L, d, device=self.device)
        if self._gpu:
            bf = torch.bfloat16
            for n in ("U", "V"):  # [L, d, r] and, transposed, [L, r, d]
                setattr(self, n + "bf", torch.empty(L, d, r, dtype=bf,
                                                    device=self.device))
                setattr(self, n + "tbf", torch.empty(L, r, d, dtype=bf,
                                                     device=self.device))
            self._refresh_mirrors()
        # optimizer state of the four, in the MLP's updater
        self._adam = hyper.mlp_optimizer == "adam"
        self.cross_step = 0
        for n in self._CROSS:
            z = torch.zeros_like(getattr(self, n))
            setattr(self, "m_" + n, z)             # Adam m / Adagrad n
            if self._adam:
                setattr(self, "v_" + n, z.clone())

    def _refresh_mirrors(self):
        for n in ("U", "V"):
            w = getattr(self, n)
            getattr(self, n + "bf").copy_(w)
            getattr(self, n + "tbf").copy_(w.transpose(1, 2))

    # ---- cross term, forward: (cross [B], what the backward needs) ----
    def _cross_forward(self, x0, train=True):
        if not self._gpu:
            cross, X, T = dcn2_ref.dcn2_cross_forward_ref(
                x0, self.U, self.V, self.bc, self.u)
            return cross, (x0, X, T)
        if self.cross_impl == "torch":
            x0 = x0.float()
            cross, X, T = dcn2_ref.dcn2_cross_forward_ref(
                x0, self.Ubf.float(), self.Vbf.float(), self.bc, self.u,
                rounding="bf16")
            return cross, (x0, X, T)
        out = require_hip_ops().dcn2_cross_forward(
            x0, self.Ubf, self.Vtbf, self.bc, self.u, train)
        return out[0], (x0, *out[1:])

    # ---- backward: dDeep += dx0 in place, the dense gradients kept ----
    def _cross_backward(self, saved, dpred, dDeep):
        x0, X, T = saved
        if self._gpu and self.cross_impl == "hip":
            ops = require_hip_ops()
            G, S, dbc, du = ops.dcn2_cross_backward(
                x0, X, T, self.Ubf, self.Utbf, self.Vbf, self.bc, self.u,
                dpred, dDeep)
            B, d = x0.shape
            r = T.shape[2]
            # dU_l = G_l^T T_l, dV_l = X_l^T S_l: the MLP's wgrad route
            dU = [ops.gemm_bf16(G[l], T[l], None, d, r, B, 1, 1, 0, False)
                  for l in range(G.shape[0])]
            dV = [ops.gemm_bf16(X[l - 1] if l else x0, S[l], None, d, r, B,
                                1, 1, 0, False) for l in range(G.shape[0])]
            self._dcross = (dU, dV, dbc, du)
            return
        if self._gpu:
            dx0, _, _, *self._dcross = dcn2_ref.dcn2_cross_backward_ref(
                x0, X, T, self.Ubf.float(), self.Vbf.float(), self.bc,
                self.u, dpred, rounding="bf16")
        else:
            dx0, _, _, *self._dcross = dcn2_ref.dcn2_cross_backward_ref(
                x0, X, T, self.U, self.V, self.bc, self.u, dpred)
        dDeep += dx0

    def _dense_step(self, p, gr, m, v, pbf=None, ptbf=None):
        lr, eps = self.h.mlp_lr, 1e-8
        ops = require_hip_ops() if self._gpu else None
        if self._adam:
            b1, b2 = 0.9, 0.999
            if ops:
                ops.dense_adam(p, gr, m, v, pbf, ptbf, lr, b1, b2, eps,
                               self.cross_step, 0.0)
                return
            m.mul_(b1).add_(gr, alpha=1 - b1)
            v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
            p.sub_(lr * (m / (1 - b1 ** self.cross_step)) /
                   ((v / (1 - b2 ** self.cross_step)).sqrt() + eps))
        elif ops:
            ops.dense_adagrad(p, gr, m, pbf, ptbf, lr, eps, 0.0)
        else:
            m.add_(gr * gr)
            p.sub_(lr * gr / (m + eps).sqrt())

    def _cross_apply(self):
        self.cross_step += 1
        for n, gr in zip(self._CROSS, self._dcross):
            p, m = getattr(self, n), getattr(self, "m_" + n)
            v = getattr(self, "v_" + n) if self._adam else None
            if n in ("bc", "u"):
                self._dense_step(p, gr, m, v)
                continue
            for l in range(p.shape[0]):  # a layer's [d, r] with its mirrors
                bf = (getattr(self, n + "bf")[l], getattr(self, n + "tbf")[l]
                      ) if self._gpu else ()
                self._dense_step(p[l], gr[l].contiguous(), m[l],
                                 v[l] if self._adam else None, *bf)

    def _score(self, wide, deep_in, train):
        deep = self.mlp.forward(deep_in, train=train)
        cross, self._saved = self._cross_forward(deep_in, train)
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
        if self._gpu:
            self._refresh_mirrors()


class DCNv2Trainer(WideDeepTrainer):
    def __init__(self, dataset, hyper: DCNv2Hyper, device="cpu",
                 batch_size=256, epochs=5, cross_impl="hip"):
        self.ds = dataset
        self.model = DCNv2Model(hyper, device=device, cross_impl=cross_impl)
        self.batch_size, self.epochs = batch_size, epochs
        self.device = torch.device(device)
