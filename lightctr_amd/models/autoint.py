"""AutoInt (multi-head self-attention over the fields) — MI355X-native trainer.

Wide&Deep's concat row x0 [B, nf*K] (both layouts) feeds the MLP and, beside
it, the interacting layers of Song et al., "AutoInt" (CIKM 2019): x0 viewed
as X^0 [B, nf, K], D = attn_heads * attn_dim, W^l [d_{l-1}, 4D] with the
columns [Q | K | V | R] and no biases,

    S_h = Q_h K_h^T,  A_h = softmax over keys (S_h)         per head
    X^l = relu(concat_h(A_h V_h) + R)                       l = 1 .. L
    ai[b] = sum_{m,c} u[m,c] X^L[b,m,c]
    score = wide + MLP(x0) + ai

Goes beyond the reference inventory. On the GPU the layers are
ops/csrc/autoint_kernels.hip (attn_impl="hip"): one launch for all L layers
forward with Q, K, V, the scores and the probabilities never stored, a
recomputing backward of one launch a layer and a chunked weight gradient, all
on the bf16 matrix unit. attn_impl="torch" composes the layers from tensor
ops (ops/autoint_ref.py with the kernels' rounding points, on the same bf16
weight mirror) and is the baseline arm. The CPU path is ops/autoint_ref.py in
fp32. The sparse tail is Wide&Deep's; W and u take the dense Adam / Adagrad
step of the MLP (mlp_optimizer, mlp_lr).

W is one flat fp32 buffer, [d_in, 4D] a layer, with bf16 mirrors in both
orientations that the dense updaters refresh. Checkpoints hold attn_W{l}.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import autoint_ref, fm_ref
from ..ops._extension import require_hip_ops
from .embed_bag import load_checkpoint
from .wide_deep import WideDeepHyper, WideDeepModel, WideDeepTrainer


@dataclass
class AutoIntHyper(WideDeepHyper):
    attn_layers: int = 3
    attn_heads: int = 2
    attn_dim: int = 32


class AutoIntModel(WideDeepModel):
    def __init__(self, hyper: AutoIntHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22, attn_impl: str = "hip"):
        L, H, hd = hyper.attn_layers, hyper.attn_heads, hyper.attn_dim
        nf, K = hyper.num_fields, hyper.k
        if not 1 <= L <= 4:
            raise ValueError(f"attn_layers must be in 1..4, got {L}")
        if H not in (1, 2, 4):
            raise ValueError(f"attn_heads must be 1, 2 or 4, got {H}")
        if hd not in (16, 32):
            raise ValueError(f"attn_dim must be 16 or 32, got {hd}")
        if H * hd > 64:
            raise ValueError(
                f"attn_heads*attn_dim must be at most 64, got {H * hd}")
        if not 1 <= nf <= 64:
            raise ValueError(f"num_fields must be in 1..64, got {nf}")
        if K < 1 or nf * K > 1024:
            raise ValueError(
                f"num_fields*k must be in 1..1024, got {nf * K}")
        if K > 64:  # a layer's weights and one example share the LDS
            raise ValueError(f"k must be at most 64, got {K}")
        if attn_impl not in ("hip", "torch"):
            raise ValueError(f"unknown attn_impl {attn_impl!r}")
        super().__init__(hyper, device=device, max_batch_nnz=max_batch_nnz)
        self.attn_impl = attn_impl
        D = H * hd
        self._span, off = [], 0   # a layer's slice of the flat buffers
        for l in range(L):
            din = D if l else K
            self._span.append((off, off + din * 4 * D, din))
            off += din * 4 * D
        g = torch.Generator().manual_seed(hyper.seed + 15485863)
        self.Wa = torch.cat([
            (torch.randn(din, 4 * D, generator=g) * din ** -0.5).flatten()
            for _, _, din in self._span]).to(self.device)
        self.ua = (torch.randn(nf, D, generator=g)
                   * (nf * D) ** -0.5).to(self.device)
        if self._gpu:
            bf = torch.bfloat16
            self.Wabf = torch.empty(off, dtype=bf, device=self.device)
            self.Watbf = torch.empty(off, dtype=bf, device=self.device)
            self._refresh_mirrors()
        self._adam = hyper.mlp_optimizer == "adam"
        self.attn_step = 0
        for n in ("Wa", "ua"):
            z = torch.zeros_like(getattr(self, n))
            setattr(self, "m_" + n, z)             # Adam m / Adagrad n
            if self._adam:
                setattr(self, "v_" + n, z.clone())

    def _layer(self, flat, l, transposed=False):
        a, b, din = self._span[l]
        return flat[a:b].view(-1, din) if transposed else flat[a:b].view(
            din, -1)

    def layers(self, flat):
        """[W^1 [K, 4D], W^l [D, 4D] ...] of a flat buffer (views)"""
        return [self._layer(flat, l) for l in range(self.h.attn_layers)]

    def _refresh_mirrors(self):
        for l in range(self.h.attn_layers):
            w = self._layer(self.Wa, l)
            self._layer(self.Wabf, l).copy_(w)
            self._layer(self.Watbf, l, True).copy_(w.t())

    def _dims(self):
        return self.h.num_fields, self.h.attn_heads, self.h.attn_dim

    # ---- attention, forward: (ai [B], what the backward needs) ----
    def _attn_forward(self, x0, train=True):
        if self._gpu and self.attn_impl == "hip":
            out = require_hip_ops().autoint_forward(
                x0, self.Wabf, self.ua, *self._dims(), train)
            return out[0], (x0, out[1] if train else None)
        if self._gpu:
            x0 = x0.float()
            ai, X = autoint_ref.autoint_forward_ref(
                x0, self.layers(self.Wabf.float()), self.ua, *self._dims(),
                rounding="bf16")
        else:
            ai, X = autoint_ref.autoint_forward_ref(
                x0, self.layers(self.Wa), self.ua, *self._dims())
        return ai, (x0, X)

    # ---- backward: dDeep += dx0 in place, the dense gradients kept ----
    def _attn_backward(self, saved, dpred, dDeep):
        x0, X = saved
        if self._gpu and self.attn_impl == "hip":
            self._dattn = tuple(require_hip_ops().autoint_backward(
                x0, X, self.Wabf, self.Watbf, self.ua, dpred, dDeep,
                *self._dims()))
            return
        if self._gpu:
            dx0, dW, du = autoint_ref.autoint_backward_ref(
                x0, X, self.layers(self.Wabf.float()), self.ua, dpred,
                *self._dims(), rounding="bf16")
        else:
            dx0, dW, du = autoint_ref.autoint_backward_ref(
                x0, X, self.layers(self.Wa), self.ua, dpred, *self._dims())
        dDeep += dx0
        self._dattn = (torch.cat([w.flatten() for w in dW]), du)

    def _dense_step(self, p, gr, m, v, pbf=None, ptbf=None):
        lr, eps = self.h.mlp_lr, 1e-8
        ops = require_hip_ops() if self._gpu else None
        if self._adam:
            b1, b2 = 0.9, 0.999
            if ops:
                ops.dense_adam(p, gr, m, v, pbf, ptbf, lr, b1, b2, eps,
                               self.attn_step, 0.0)
                return
            m.mul_(b1).add_(gr, alpha=1 - b1)
            v.mul_(b2).addcmul_(gr, gr, value=1 - b2)
            p.sub_(lr * (m / (1 - b1 ** self.attn_step)) /
                   ((v / (1 - b2 ** self.attn_step)).sqrt() + eps))
        elif ops:
            ops.dense_adagrad(p, gr, m, pbf, ptbf, lr, eps, 0.0)
        else:
            m.add_(gr * gr)
            p.sub_(lr * gr / (m + eps).sqrt())

    def _attn_apply(self):
        self.attn_step += 1
        dW, du = self._dattn
        self._dense_step(self.ua, du, self.m_ua,
                         self.v_ua if self._adam else None)
        for l in range(self.h.attn_layers):  # a layer's [d_in, 4D], mirrors
            bf = (self._layer(self.Wabf, l),
                  self._layer(self.Watbf, l, True)) if self._gpu else ()
            self._dense_step(
                self._layer(self.Wa, l), self._layer(dW, l),
                self._layer(self.m_Wa, l),
                self._layer(self.v_Wa, l) if self._adam else None, *bf)

    def _score(self, wide, deep_in, train):
        deep = self.mlp.forward(deep_in, train=train)
        ai, self._saved = self._attn_forward(deep_in, train)
        return wide + deep[:, 0] + ai

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
        self._attn_backward(self._saved, dpred, dDeep)
        tail = self._sparse_step_gpu if self._gpu else self._sparse_step_cpu
        tail(row_ptr, fids, vals, fields, dDeep, dpred)
        self.mlp.apply_grads()
        self._attn_apply()
        return loss

    _NAMES = {"Wa": "W", "m_Wa": "m_W", "v_Wa": "v_W", "ua": "u",
              "m_ua": "m_u", "v_ua": "v_u"}

    def _attn_flat(self):
        return ["Wa", "m_Wa"] + (["v_Wa"] if self._adam else [])

    def _attn_plain(self):
        return ["ua", "m_ua"] + (["v_ua"] if self._adam else [])

    def state_dict(self):
        d = super().state_dict()
        for n in self._attn_flat():  # [d_in, 4D] a layer
            for l, w in enumerate(self.layers(getattr(self, n))):
                d[f"attn_{self._NAMES[n]}{l}"] = w.contiguous()
        d.update({"attn_" + self._NAMES[n]: getattr(self, n)
                  for n in self._attn_plain()})
        d["attn_step"] = torch.tensor(self.attn_step)
        return d

    def load(self, path):
        d = load_checkpoint(path, self.device)
        super().load(d)
        for n in self._attn_flat():
            for l, w in enumerate(self.layers(getattr(self, n))):
                w.copy_(d[f"attn_{self._NAMES[n]}{l}"])
        for n in self._attn_plain():
            getattr(self, n).copy_(d["attn_" + self._NAMES[n]])
        self.attn_step = int(d["attn_step"])
        if self._gpu:
            self._refresh_mirrors()


class AutoIntTrainer(WideDeepTrainer):
    def __init__(self, dataset, hyper: AutoIntHyper, device="cpu",
                 batch_size=256, epochs=5, attn_impl="hip"):
        self.ds = dataset
        self.model = AutoIntModel(hyper, device=device, attn_impl=attn_impl)
        self.batch_size, self.epochs = batch_size, epochs
        self.device = torch.device(device)
