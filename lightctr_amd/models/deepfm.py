"""DeepFM — MI355X-native trainer.

One embedding table E[F, K] used twice: as the FM latent factors of the
pairwise term and as the per-field embeddings concatenated into the MLP;
the FM part sits beside a wide/LR term and one logistic loss covers the sum
(Guo et al., "DeepFM", IJCAI 2017). Goes beyond the reference inventory,
which stops at FM, FFM, NFM and the wide + deep trainer; built from the same
parts: fixed-position concat layout of models/wide_deep.py, bf16 MFMA MLP,
sorted segment-reduce backward and the fused sparse optimizers.

    wide[r]  = sum_j W[f_j] x_j
    s[r,k]   = sum_j E[f_j,k] x_j
    fm[r]    = wide[r] + 0.5 sum_k (s[r,k]^2 - sum_j (E[f_j,k] x_j)^2)
    deep_in[r, pos*K+k] = E[f_j,k] x_j        pos = j - row_ptr[r] < nf
    score[r] = fm[r] + MLP(deep_in)[r, 0]

Entries past nf are left out of the concat only. forward_impl="fused" runs
one pass over the batch each way (ops/csrc/deepfm_kernels.hip);
"composed" runs the FM and embedding kernels side by side and is the
baseline tools/bench_deepfm.py measures against.

layout="field" addresses the concat by the entry's field instead of its
position, with pooling="sum" or "mean" over the entries that share a field
(models/embed_bag.py has the definition):

    deep_in[r, c*K+k] = inv(r,c) sum_{j: fields[j] == c} E[f_j,k] x_j

wide, s and fm still run over every entry of the row; an entry whose field
is outside [0, nf) is left out of the concat only. "fused" then runs
ops/csrc/embed_bag_kernels.hip's deepfm_bag_* pair, "composed" fm_forward +
embed_bag_forward and fm_backward_emit + embed_bag_backward_emit + add.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import fm_ref
from ..ops._extension import require_hip_ops, sort_ids
from ..utils.metrics import auc_score
from .embed_bag import (BagLayout, bag_dgather_cpu, bag_gather_cpu,
                        load_checkpoint)
from .mlp import MLP


@dataclass
class DeepFMHyper:
    num_features: int
    num_fields: int = 39
    k: int = 16
    hidden: tuple = (256, 128)
    optimizer: str = "adagrad"  # sparse side
    mlp_optimizer: str = "adam"
    # Wide&Deep's fields; lr alone defaults lower (0.05 there). Adagrad's
    # first steps move every touched element of E by ~lr, and here E also
    # feeds the pair term, which grows with the square of 39 such moves.
    lr: float = 0.01
    mlp_lr: float = 1e-3
    eps: float = 1e-8
    l2: float = 1e-5
    ftrl_alpha: float = 0.15
    ftrl_beta: float = 1.0
    ftrl_l1: float = 1e-4
    ftrl_l2: float = 1e-4
    ftrl_v: str = "adagrad"  # latent updater under ftrl (see models/fm.py)
    dropout: float = 0.0
    init_sigma: float = 0.01
    seed: int = 1234
    layout: str = "position"  # or "field": concat addressed by field
    pooling: str = "sum"      # or "mean"; layout="field" only


def _rows_pos(row_ptr):
    """entry -> (row index, position in row)"""
    B = row_ptr.numel() - 1
    rp = row_ptr.long()
    row_idx = torch.repeat_interleave(torch.arange(B), rp[1:] - rp[:-1])
    pos = torch.arange(int(rp[-1])) - rp[:-1][row_idx]
    return row_idx, pos


class DeepFMModel(BagLayout):
    def __init__(self, hyper: DeepFMHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22, forward_impl: str = "fused"):
        assert forward_impl in ("fused", "composed"), forward_impl
        self.h = hyper
        self.forward_impl = forward_impl
        self.device = torch.device(device)
        F, nf, K = hyper.num_features, hyper.num_fields, hyper.k
        assert K in (4, 8, 16, 32, 64)
        self._init_bag(hyper, self.device)
        g = torch.Generator().manual_seed(hyper.seed)
        self.W = torch.zeros(F, device=self.device)  # wide LR weights
        self.E = (torch.randn(F, K, generator=g) * hyper.init_sigma).to(
            self.device)  # shared table: FM factors and deep embeddings
        self.gradW = torch.zeros_like(self.W)
        self.gradE = torch.zeros_like(self.E)
        self.nW = torch.zeros_like(self.W)
        self.nE = torch.zeros_like(self.E)
        if hyper.optimizer == "ftrl":
            self.zW = torch.zeros_like(self.W)
            self.zE = torch.zeros_like(self.E)
        dims = [nf * K, *hyper.hidden, 1]
        self.mlp = MLP(dims, optimizer=hyper.mlp_optimizer, lr=hyper.mlp_lr,
                       dropout=hyper.dropout, seed=hyper.seed, device=device)
        nwords = (F + 63) // 64
        self.touched = torch.zeros(nwords, dtype=torch.int64,
                                   device=self.device)
        cap = min(F, max_batch_nnz)
        self.uniq = torch.zeros(cap, dtype=torch.int32, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._gpu = self.device.type == "cuda"
        if self._gpu:
            require_hip_ops()

    # -- CPU oracle pieces (plain fp32 torch) -------------------------------
    def _fm_gather_cpu(self, row_ptr, fids, vals, fields=None):
        """(fm [B], sumVX [B, K], deep_in [B, nf*K]) from one set of
        products E[f] x. fields: the concat is addressed by field and
        pooled."""
        B = row_ptr.numel() - 1
        nf, K = self.h.num_fields, self.h.k
        row_idx, pos = _rows_pos(row_ptr)
        f = fids.long()
        vx = self.E[f] * vals.unsqueeze(1)
        sumVX = torch.zeros(B, K).index_add_(0, row_idx, vx)
        sq = torch.zeros(B, K).index_add_(0, row_idx, vx * vx)
        wide = torch.zeros(B).index_add_(0, row_idx, self.W[f] * vals)
        fm = wide + 0.5 * (sumVX * sumVX - sq).sum(dim=1)
        if fields is not None:
            return fm, sumVX, bag_gather_cpu(self.E, row_ptr, fields, fids,
                                             vals, nf, self.h.pooling)
        deep_in = torch.zeros(B, nf * K)
        keep = pos < nf
        deep_in.view(B * nf, K)[(row_idx * nf + pos)[keep]] = vx[keep]
        return fm, sumVX, deep_in

    def _emit_cpu(self, row_ptr, fids, vals, sumVX, dDeep, dpred,
                  fields=None):
        """per-entry (gw [nnz], gv [nnz, K]) in the kernel's operation
        order: gv = (D + d (s - E x)) x; under the field layout D is the
        gradient of the entry's slot times the slot's inv"""
        B = row_ptr.numel() - 1
        nf, K = self.h.num_fields, self.h.k
        row_idx, pos = _rows_pos(row_ptr)
        x = vals.unsqueeze(1)
        d = dpred[row_idx].unsqueeze(1)
        if fields is not None:
            D = bag_dgather_cpu(dDeep, row_ptr, fields, nf, K,
                                self.h.pooling)
        else:
            D = dDeep.reshape(B, nf, K)[row_idx, pos.clamp(max=nf - 1)]
            D = torch.where((pos < nf).unsqueeze(1), D, torch.zeros_like(D))
        gv = (D + d * (sumVX[row_idx] - self.E[fids.long()] * x)) * x
        return dpred[row_idx] * vals, gv

    def _forward_cpu(self, row_ptr, fids, vals, train=True, fields=None):
        fm, sumVX, deep_in = self._fm_gather_cpu(row_ptr, fids, vals, fields)
        deep = self.mlp.forward(deep_in, train=train)
        return fm + deep[:, 0], sumVX

    # -- GPU ----------------------------------------------------------------
    def _forward_gpu(self, row_ptr, fids, vals, train=True, fields=None):
        ops = require_hip_ops()
        nf = self.h.num_fields
        if fields is not None and self.forward_impl == "fused":
            fm, sumVX, deep_in = ops.deepfm_bag_forward(
                row_ptr, fields, fids, vals, self.W, self.E, nf, self._pool)
        elif fields is not None:
            fm, sumVX = ops.fm_forward(row_ptr, fids, vals, self.W, self.E)
            deep_in = ops.embed_bag_forward(row_ptr, fields, fids, vals,
                                            self.E, nf, self._pool)
        elif self.forward_impl == "fused":
            fm, sumVX, deep_in = ops.deepfm_forward(row_ptr, fids, vals,
                                                    self.W, self.E, nf)
        else:
            fm, sumVX = ops.fm_forward(row_ptr, fids, vals, self.W, self.E)
            deep_in = ops.embed_gather(row_ptr, fids, vals, self.E, nf)
        if row_ptr.numel() <= 1:  # empty batch: no GEMM to launch
            return fm, sumVX
        deep = self.mlp.forward(deep_in, train=train)
        return fm + deep[:, 0], sumVX

    def _emit_gpu(self, ops, row_ptr, fids, vals, sumVX, dDeep, dpred,
                  fields=None):
        nf = self.h.num_fields
        if fields is not None and self.forward_impl == "fused":
            return ops.deepfm_bag_backward_emit(row_ptr, fields, fids, vals,
                                                self.E, sumVX, dDeep, dpred,
                                                nf, self._pool)
        if self.forward_impl == "fused":
            return ops.deepfm_backward_emit(row_ptr, fids, vals, self.E,
                                            sumVX, dDeep, dpred, nf)
        gw, gv_fm = ops.fm_backward_emit(row_ptr, fids, vals, self.E, sumVX,
                                         dpred, None)
        # the binding wants a dwide tensor; its gw repeats the FM emit's
        if fields is not None:
            _, gv_deep = ops.embed_bag_backward_emit(
                row_ptr, fields, vals, dDeep, dpred, nf, self.h.k,
                self._pool)
        else:
            _, gv_deep = ops.embed_backward_emit(row_ptr, vals, dDeep, dpred,
                                                 nf, self.h.k)
        return gw, gv_fm + gv_deep

    def predict_proba(self, row_ptr, fids, vals, fields=None):
        fwd = self._forward_gpu if self._gpu else self._forward_cpu
        score, _ = fwd(row_ptr, fids, vals, train=False,
                       fields=self._fields(fields))
        return torch.sigmoid(torch.clamp(score, -16, 16))

    def train_step(self, row_ptr, fids, vals, labels, fields=None):
        B = row_ptr.numel() - 1
        fields = self._fields(fields)
        if B == 0:
            return torch.zeros(0, device=self.device)
        scale = 1.0 / B
        if self._gpu:
            ops = require_hip_ops()
            score, sumVX = self._forward_gpu(row_ptr, fids, vals,
                                             fields=fields)
            loss, dpred = ops.logloss_grad(score, labels, scale)
            dDeep = self.mlp.backward(dpred.unsqueeze(1))  # [B, nf*K]
            gw, gv = self._emit_gpu(ops, row_ptr, fids, vals, sumVX,
                                    dDeep.contiguous(), dpred, fields)
            sorted_fids, perm = sort_ids(fids, self.h.num_features)
            ops.fm_sorted_apply(sorted_fids, perm, gw, gv, self.gradW,
                                self.gradE, self.touched)
            self.count.zero_()
            ops.bitmap_compact(self.touched, self.uniq, self.count)
            live = self.uniq[: min(self.uniq.numel(), fids.numel())]
            if self.h.optimizer == "ftrl":
                ops.fm_ftrl_apply(live, self.count, self.W, self.E,
                                  self.zW, self.nW, self.zE, self.nE,
                                  self.gradW, self.gradE, self.h.ftrl_alpha,
                                  self.h.ftrl_beta, self.h.ftrl_l1,
                                  self.h.ftrl_l2,
                                  1 if self.h.ftrl_v == "adagrad" else 0,
                                  self.h.lr, self.h.eps, self.h.l2)
            else:
                ops.fm_adagrad_apply(live, self.count, self.W, self.E,
                                     self.nW, self.nE, self.gradW, self.gradE,
                                     self.h.lr, self.h.eps, self.h.l2)
            self.mlp.apply_grads()
            return loss
        # CPU oracle
        score, sumVX = self._forward_cpu(row_ptr, fids, vals, fields=fields)
        loss, dpred = fm_ref.logloss_grad_ref(score, labels, scale)
        dDeep = self.mlp.backward(dpred.unsqueeze(1))
        gw, gv = self._emit_cpu(row_ptr, fids, vals, sumVX, dDeep, dpred,
                                fields)
        f = fids.long()
        self.gradW.index_add_(0, f, gw)
        self.gradE.index_add_(0, f, gv)
        uniq = torch.unique(f).int()
        if self.h.optimizer == "ftrl":
            fm_ref.ftrl_apply_ref(uniq, self.W, self.E, self.zW, self.nW,
                                  self.zE, self.nE, self.gradW, self.gradE,
                                  self.h.ftrl_alpha, self.h.ftrl_beta,
                                  self.h.ftrl_l1, self.h.ftrl_l2,
                                  v_adagrad=self.h.ftrl_v == "adagrad",
                                  v_lr=self.h.lr, v_eps=self.h.eps,
                                  v_l2=self.h.l2)
        else:
            fm_ref.adagrad_apply_ref(uniq, self.W, self.E, self.nW, self.nE,
                                     self.gradW, self.gradE, self.h.lr,
                                     self.h.eps, self.h.l2)
        self.mlp.apply_grads()
        return loss

    # -- checkpoint ---------------------------------------------------------
    def state_dict(self):
        d = {"W": self.W, "E": self.E, "nW": self.nW, "nE": self.nE,
             "mlp": self.mlp.state_dict(), "hyper": self.h.__dict__}
        if self.h.optimizer == "ftrl":
            d["zW"], d["zE"] = self.zW, self.zE
        return d

    def save(self, path):
        torch.save(self.state_dict(), path)

    def load(self, path):
        d = load_checkpoint(path, self.device)
        self.W.copy_(d["W"]); self.E.copy_(d["E"])
        self.nW.copy_(d["nW"]); self.nE.copy_(d["nE"])
        if self.h.optimizer == "ftrl" and "zW" in d:
            self.zW.copy_(d["zW"]); self.zE.copy_(d["zE"])
        self.mlp.load_state_dict(d["mlp"])


class DeepFMTrainer:
    def __init__(self, dataset, hyper: DeepFMHyper, device="cpu",
                 batch_size=256, epochs=5, forward_impl="fused"):
        self.ds = dataset
        self.model = DeepFMModel(hyper, device=device,
                                 forward_impl=forward_impl)
        self.batch_size, self.epochs = batch_size, epochs
        self.device = torch.device(device)

    def train(self, log=print):
        ds = self.ds.to(self.device)
        N = ds.num_rows
        for ep in range(self.epochs):
            tot, nb = 0.0, 0
            for s in range(0, N, self.batch_size):
                b = ds.slice_rows(s, min(s + self.batch_size, N))
                loss = self.model.train_step(b.row_ptr, b.fids, b.vals,
                                             b.labels, fields=b.fields)
                tot += float(loss.mean()); nb += 1
            if log:
                log(f"epoch {ep}: loss={tot / max(nb, 1):.5f}")
        return self

    def evaluate(self, dataset=None):
        ds = (dataset or self.ds).to(self.device)
        p = self.model.predict_proba(ds.row_ptr, ds.fids, ds.vals,
                                     fields=ds.fields)
        loss = torch.nn.functional.binary_cross_entropy(
            p.clamp(1e-7, 1 - 1e-7), ds.labels)
        return {"auc": auc_score(p.cpu(), ds.labels.cpu()),
                "logloss": float(loss),
                "accuracy": float(((p > 0.5) == (ds.labels > 0.5))
                                  .float().mean())}
