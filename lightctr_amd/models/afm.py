"""AFM (attention over the pairwise products) — MI355X-native trainer.

Wide&Deep's concat row x0 [B, nf*K] (both layouts) feeds the MLP and, beside
it, the pair attention of Xiao et al., "Attentional Factorization Machines"
(IJCAI 2017): x0 viewed as e [B, nf, K], A = attn_factor, Wa [K, A], ba [A],
qa [A], ua [K],

    p_ij = e_i * e_j  (i < j),  s_ij = qa . relu(Wa^T p_ij + ba)
    a = softmax over all pairs (s),  afm[b] = ua . sum_ij a_ij p_ij
    score = wide + MLP(x0) + afm

Goes beyond the reference inventory. On the GPU the attention is
ops/csrc/afm_kernels.hip (afm_impl="hip"): one forward and one backward
launch, the products, scores and weights of the pairs formed in registers and
never stored, on the bf16 matrix unit. afm_impl="torch" composes it from
tensor ops (ops/afm_ref.py with the kernels' rounding points, on the same
bf16 weight mirror) and is the baseline arm. The CPU path is ops/afm_ref.py
in fp32. The sparse tail is Wide&Deep's; Wa, ba, qa and ua take the dense
Adam / Adagrad step of the MLP (mlp_optimizer, mlp_lr).

Wa has bf16 mirrors in both orientations that the dense updaters refresh.
Checkpoints hold afm_W, afm_b, afm_q, afm_u and their optimiser state.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import afm_ref, fm_ref
from ..ops._extension import require_hip_ops
from .embed_bag import load_checkpoint
from .wide_deep import WideDeepHyper, WideDeepModel, WideDeepTrainer


@dataclass
class AFMHyper(WideDeepHyper):
    attn_factor: int = 32


class AFMModel(WideDeepModel):
    _PARAMS = ("Wa", "ba", "qa", "ua")

    def __init__(self, hyper: AFMHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22, afm_impl: str = "hip"):
        A, nf, K = hyper.attn_factor, hyper.num_fields, hyper.k
        if A % 16 or not 16 <= A <= 64:
            raise ValueError(
                f"attn_factor must be a multiple of 16 in 16..64, got {A}")
        if not 2 <= nf <= 64:
            raise ValueError(f"num_fields must be in 2..64, got {nf}")
        if K < 1 or nf * K > 1024:
            raise ValueError(
                f"num_fields*k must be in 2..1024, got {nf * K}")
        if K > 64:
            raise ValueError(f"k must be at most 64, got {K}")
        if afm_impl not in ("hip", "torch"):
            raise ValueError(f"unknown afm_impl {afm_impl!r}")
        super().__init__(hyper, device=device, max_batch_nnz=max_batch_nnz)
        self.afm_impl = afm_impl
        g = torch.Generator().manual_seed(hyper.seed + 32452843)
        self.Wa = (torch.randn(K, A, generator=g) * K ** -0.5).to(self.device)
        self.ba = torch.zeros(A, device=self.device)
        self.qa = (torch.randn(A, generator=g) * A ** -0.5).to(self.device)
        self.ua = (torch.randn(K, generator=g) * K ** -0.5).to(self.device)
        if self._gpu:
            bf = torch.bfloat16
            self.Wabf = torch.empty(K, A, dtype=bf, device=self.device)
            self.Watbf = torch.empty(A, K, dtype=bf, device=self.device)
            self._refresh_mirrors()
        self._adam = hyper.mlp_optimizer == "adam"
        self.afm_step = 0
        for n in self._PARAMS:
            z = torch.zeros_like(getattr(self, n))
            setattr(self, "m_" + n, z)             # Adam m / Adagrad n
            if self._adam:
                setattr(self, "v_" + n, z.clone())

    def _refresh_mirrors(self):
        self.Wabf.copy_(self.Wa)
        self.Watbf.copy_(self.Wa.t())

    def _params(self, mirror):
        W = self.Wabf.float() if mirror else self.Wa
        return W, self.ba, self.qa, self.ua

    # ---- attention, forward: (afm [B], what the backward needs) ----
    def _afm_forward(self, x0, train=True):
        nf = self.h.num_fields
        if self._gpu and self.afm_impl == "hip":
            afm, lse = require_hip_ops().afm_forward(
                x0, self.Wabf, self.ba, self.qa, self.ua, nf, train)
            return afm, (x0, lse, afm)
        if self._gpu:
            x0 = x0.float()
            afm, lse = afm_ref.afm_forward_ref(x0, *self._params(True), nf,
                                               rounding="bf16")
        else:
            afm, lse = afm_ref.afm_forward_ref(x0, *self._params(False), nf)
        return afm, (x0, lse, afm)

    # ---- backward: dDeep += dx0 in place, the dense gradients kept ----
    def _afm_backward(self, saved, dpred, dDeep):
        x0, lse, afm = saved
        nf = self.h.num_fields
        if self._gpu and self.afm_impl == "hip":
            self._dafm = tuple(require_hip_ops().afm_backward(
                x0, lse, afm, self.Wabf, self.Watbf, self.ba, self.qa,
                self.ua, dpred, dDeep, nf))
            return
        if self._gpu:
            dx0, *gr = afm_ref.afm_backward_ref(
                x0, lse, afm, *self._params(True), dpred, nf,
                rounding="bf16")
        else:
            dx0, *gr = afm_ref.afm_backward_ref(
                x0, lse, afm, *self._params(False), dpred, nf)
        dDeep += dx0
        self._dafm = tuple(gr)

    def _dense_step(self, p, gr, m, v, pbf=None, ptbf=None):
        lr, eps = self.h.mlp_lr, 1e-8
        ops = require_hip_ops() if self._gpu else None
        if self._adam:
            b1, b2 = 0.9, 0.999
            if ops:
                ops.dense_adam(p, gr, m, v, pbf, ptbf, lr, b1, b2, eps,
                               self.afm_step, 0.0)
                return
            m.mul_(b1).add_(gr, alpha=1 - b1)
            v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
            p.sub_(lr * (m / (1 - b1 ** self.afm_step)) /
                   ((v / (1 - b2 ** self.afm_step)).sqrt() + eps))
        elif ops:
            ops.dense_adagrad(p, gr, m, pbf, ptbf, lr, eps, 0.0)
        else:
            m.add_(gr * gr)
            p.sub_(lr * gr / (m + eps).sqrt())

    def _afm_apply(self):
        self.afm_step += 1
        for n, gr in zip(self._PARAMS, self._dafm):
            bf = (self.Wabf, self.Watbf) if self._gpu and n == "Wa" else ()
            self._dense_step(getattr(self, n), gr.contiguous(),
                             getattr(self, "m_" + n),
                             getattr(self, "v_" + n) if self._adam else None,
                             *bf)

    def _score(self, wide, deep_in, train):
        deep = self.mlp.forward(deep_in, train=train)
        afm, self._saved = self._afm_forward(deep_in, train)
        return wide + deep[:, 0] + afm

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
        self._afm_backward(self._saved, dpred, dDeep)
        tail = self._sparse_step_gpu if self._gpu else self._sparse_step_cpu
        tail(row_ptr, fids, vals, fields, dDeep, dpred)
        self.mlp.apply_grads()
        self._afm_apply()
        return loss

    _NAMES = {"Wa": "W", "ba": "b", "qa": "q", "ua": "u"}

    def _afm_state(self):
        pre = ("", "m_", "v_") if self._adam else ("", "m_")
        return [(f"afm_{s}{self._NAMES[n]}", s + n) for n in self._PARAMS
                for s in pre]

    def state_dict(self):
        d = super().state_dict()
        d.update({key: getattr(self, n) for key, n in self._afm_state()})
        d["afm_step"] = torch.tensor(self.afm_step)
        return d

    def load(self, path):
        d = load_checkpoint(path, self.device)
        super().load(d)
        for key, n in self._afm_state():
            getattr(self, n).copy_(d[key])
        self.afm_step = int(d["afm_step"])
        if self._gpu:
            self._refresh_mirrors()


class AFMTrainer(WideDeepTrainer):
    def __init__(self, dataset, hyper: AFMHyper, device="cpu",
                 batch_size=256, epochs=5, afm_impl="hip"):
        self.ds = dataset
        self.model = AFMModel(hyper, device=device, afm_impl=afm_impl)
        self.batch_size, self.epochs = batch_size, epochs
        self.device = torch.device(device)
