"""xDeepFM (Compressed Interaction Network) — MI355X-native trainer.

Wide&Deep's concat row x0 [B, nf*K] (both layouts) feeds the MLP and, beside
it, the CIN of Lian et al., "xDeepFM" (KDD 2018), which crosses whole field
vectors: x0 viewed as X^0 [B, m = nf, D = K], H_0 = m, H_l = cin_maps,

    X^l[b,h,d] = sum_{i,j} W^l[h,i,j] X^{l-1}[b,i,d] x0[b,j,d]   l = 1 .. L
    cin[b]     = sum_l sum_h u[l,h] sum_d X^l[b,h,d]
    score      = wide + MLP(x0) + cin

(identity activation, every layer feeds the output, no split-half). Goes
beyond the reference inventory. On the GPU the CIN is ops/csrc/cin_kernels.hip
(cin_impl="hip"): one launch for all L layers forward, one backward, one
weight gradient a layer, all on the bf16 matrix unit with the operand
X^{l-1}[b,i,d] x0[b,j,d] formed in registers and never stored.
cin_impl="torch" composes the layers from tensor ops (ops/cin_ref.py with the
kernels' rounding points, on the same bf16 weight mirror) and is the baseline
arm. The CPU path is ops/cin_ref.py in fp32. The sparse tail is Wide&Deep's;
W and u take the dense Adam / Adagrad step of the MLP (mlp_optimizer, mlp_lr).

The weights live in the kernels' order of (i, j) (cin_ref.cin_order: one flat
buffer, [H, Kl] a layer, pad columns at zero with zero gradient), so that the
dense updaters refresh the bf16 mirrors [H, Kl] and [Kl, H] as they do for the
MLP. Checkpoints hold the canonical W^l [H, H_{l-1}, m].
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import cin_ref, fm_ref
from ..ops._extension import require_hip_ops
from .embed_bag import load_checkpoint
from .wide_deep import WideDeepHyper, WideDeepModel, WideDeepTrainer


@dataclass
class XDeepFMHyper(WideDeepHyper):
    cin_layers: int = 2
    cin_maps: int = 64


class XDeepFMModel(WideDeepModel):
    def __init__(self, hyper: XDeepFMHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22, cin_impl: str = "hip"):
        L, H, nf = hyper.cin_layers, hyper.cin_maps, hyper.num_fields
        if not 1 <= L <= 4:
            raise ValueError(f"cin_layers must be in 1..4, got {L}")
        if H % 16 or not 16 <= H <= 128:
            raise ValueError(
                f"cin_maps must be a multiple of 16 in 16..128, got {H}")
        if not 1 <= nf <= 64:
            raise ValueError(f"num_fields must be in 1..64, got {nf}")
        if nf * hyper.k > 1024:
            raise ValueError(
                f"num_fields*k must be at most 1024, got {nf * hyper.k}")
        if cin_impl not in ("hip", "torch"):
            raise ValueError(f"unknown cin_impl {cin_impl!r}")
        super().__init__(hyper, device=device, max_batch_nnz=max_batch_nnz)
        self.cin_impl = cin_impl
        # a layer's slice of the flat buffers, as [H, Kl], and where the
        # canonical (i, j) sit in it
        self._idx, self._span, off = [], [], 0
        for l in range(L):
            idx, cols = cin_ref.cin_order(nf, nf if l == 0 else H)
            self._idx.append(idx.flatten().to(self.device))
            self._span.append((off, off + H * cols, cols))
            off += H * cols
        g = torch.Generator().manual_seed(hyper.seed + 104729)
        W = [torch.randn(H, nf if l == 0 else H, nf, generator=g)
             * ((nf if l == 0 else H) * nf) ** -0.5 for l in range(L)]
        self.Wk = torch.zeros(off, device=self.device)
        self._set_canonical(self.Wk, W)
        self.u = (torch.randn(L, H, generator=g) * H ** -0.5).to(self.device)
        if self._gpu:
            bf = torch.bfloat16
            self.Wkbf = torch.empty(off, dtype=bf, device=self.device)
            self.Wktbf = torch.empty(off, dtype=bf, device=self.device)
            self._refresh_mirrors()
        self._adam = hyper.mlp_optimizer == "adam"
        self.cin_step = 0
        for n in ("Wk", "u"):
            z = torch.zeros_like(getattr(self, n))
            setattr(self, "m_" + n, z)             # Adam m / Adagrad n
            if self._adam:
                setattr(self, "v_" + n, z.clone())

    def _layer(self, flat, l, transposed=False):
        a, b, cols = self._span[l]
        H = self.h.cin_maps
        return flat[a:b].view(cols, H) if transposed else flat[a:b].view(
            H, cols)

    def canonical(self, flat):
        """[W^1 [H, m, m], W^l [H, H, m] ...] of a flat kernel-order buffer"""
        m = self.h.num_fields
        return [self._layer(flat, l)[:, self._idx[l]].view(
            self.h.cin_maps, -1, m) for l in range(self.h.cin_layers)]

    def _set_canonical(self, flat, W):
        flat.zero_()
        for l, w in enumerate(W):
            self._layer(flat, l)[:, self._idx[l]] = w.flatten(1).to(
                flat.device, flat.dtype)

    def _refresh_mirrors(self):
        for l in range(self.h.cin_layers):
            w = self._layer(self.Wk, l)
            self._layer(self.Wkbf, l).copy_(w)
            self._layer(self.Wktbf, l, True).copy_(w.t())

    # ---- CIN, forward: (cin [B], what the backward needs) ----
    def _cin_forward(self, x0, train=True):
        nf = self.h.num_fields
        if self._gpu and self.cin_impl == "hip":
            out = require_hip_ops().cin_forward(x0, self.Wkbf, self.u, nf,
                                                train)
            return out[0], (x0, out[1] if train else None)
        if self._gpu:
            x0 = x0.float()
            cin, X = cin_ref.cin_forward_ref(
                x0, self.canonical(self.Wkbf.float()), self.u, nf,
                rounding="bf16")
        else:
            cin, X = cin_ref.cin_forward_ref(x0, self.canonical(self.Wk),
                                             self.u, nf)
        return cin, (x0, X)

    # ---- backward: dDeep += dx0 in place, the dense gradients kept ----
    def _cin_backward(self, saved, dpred, dDeep):
        x0, X = saved
        nf = self.h.num_fields
        if self._gpu and self.cin_impl == "hip":
            ops = require_hip_ops()
            dX, du = ops.cin_backward(x0, X, self.Wktbf, self.u, dpred,
                                      dDeep, nf)
            self._dcin = (ops.cin_wgrad(x0, X, dX, self.u, nf), du)
            return
        if self._gpu:
            dx0, _, dW, du = cin_ref.cin_backward_ref(
                x0, X, self.canonical(self.Wkbf.float()), self.u, dpred, nf,
                rounding="bf16")
        else:
            dx0, _, dW, du = cin_ref.cin_backward_ref(
                x0, X, self.canonical(self.Wk), self.u, dpred, nf)
        dDeep += dx0
        dWk = torch.empty_like(self.Wk)
        self._set_canonical(dWk, dW)
        self._dcin = (dWk, du)

    def _dense_step(self, p, gr, m, v, pbf=None, ptbf=None):
        lr, eps = self.h.mlp_lr, 1e-8
        ops = require_hip_ops() if self._gpu else None
        if self._adam:
            b1, b2 = 0.9, 0.999
            if ops:
                ops.dense_adam(p, gr, m, v, pbf, ptbf, lr, b1, b2, eps,
                               self.cin_step, 0.0)
                return
            m.mul_(b1).add_(gr, alpha=1 - b1)
            v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
            p.sub_(lr * (m / (1 - b1 ** self.cin_step)) /
                   ((v / (1 - b2 ** self.cin_step)).sqrt() + eps))
        elif ops:
            ops.dense_adagrad(p, gr, m, pbf, ptbf, lr, eps, 0.0)
        else:
            m.add_(gr * gr)
            p.sub_(lr * gr / (m + eps).sqrt())

    def _cin_apply(self):
        self.cin_step += 1
        dWk, du = self._dcin
        self._dense_step(self.u, du, self.m_u,
                         self.v_u if self._adam else None)
        for l in range(self.h.cin_layers):  # a layer's [H, Kl], its mirrors
            bf = (self._layer(self.Wkbf, l),
                  self._layer(self.Wktbf, l, True)) if self._gpu else ()
            self._dense_step(
                self._layer(self.Wk, l), self._layer(dWk, l),
                self._layer(self.m_Wk, l),
                self._layer(self.v_Wk, l) if self._adam else None, *bf)

    def _score(self, wide, deep_in, train):
        deep = self.mlp.forward(deep_in, train=train)
        cin, self._saved = self._cin_forward(deep_in, train)
        return wide + deep[:, 0] + cin

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
        self._cin_backward(self._saved, dpred, dDeep)
        tail = self._sparse_step_gpu if self._gpu else self._sparse_step_cpu
        tail(row_ptr, fids, vals, fields, dDeep, dpred)
        self.mlp.apply_grads()
        self._cin_apply()
        return loss

    def _cin_flat(self):
        return ["Wk", "m_Wk"] + (["v_Wk"] if self._adam else [])

    def _cin_plain(self):
        return ["u", "m_u"] + (["v_u"] if self._adam else [])

    def state_dict(self):
        d = super().state_dict()
        for n in self._cin_flat():  # canonical [H, H_prev, m] a layer
            for l, w in enumerate(self.canonical(getattr(self, n))):
                d[f"cin_{n[:-1]}{l}"] = w.contiguous()
        d.update({"cin_" + n: getattr(self, n) for n in self._cin_plain()})
        d["cin_step"] = torch.tensor(self.cin_step)
        return d

    def load(self, path):
        d = load_checkpoint(path, self.device)
        super().load(d)
        for n in self._cin_flat():
            self._set_canonical(getattr(self, n), [
                d[f"cin_{n[:-1]}{l}"] for l in range(self.h.cin_layers)])
        for n in self._cin_plain():
            getattr(self, n).copy_(d["cin_" + n])
        self.cin_step = int(d["cin_step"])
        if self._gpu:
            self._refresh_mirrors()


class XDeepFMTrainer(WideDeepTrainer):
    def __init__(self, dataset, hyper: XDeepFMHyper, device="cpu",
                 batch_size=256, epochs=5, cin_impl="hip"):
        self.ds = dataset
        self.model = XDeepFMModel(hyper, device=device, cin_impl=cin_impl)
        self.batch_size, self.epochs = batch_size, epochs
        self.device = torch.device(device)
