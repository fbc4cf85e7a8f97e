"""Field-weighted Factorization Machine — MI355X-native trainer.

One latent table V[F, K] as in FM plus one learned scalar per pair of
fields, R[nf, nf] (Pan et al., "Field-weighted Factorization Machines",
WWW 2018): the field-aware pair strengths of FFM at 1/nf of its parameters.
Goes beyond the reference inventory, which stops at FM and FFM.

    pred[r] = sum_j W[f_j] x_j
              + sum_{i<j} R[min(a_i,a_j), max(a_i,a_j)] <V[f_i], V[f_j]> x_i x_j

a_j being the field of entry j; pairs inside one field (multi-hot rows) are
weighted by R[a,a]. Only the upper triangle of R is used and trained; with
R == 1 the model is FM. The GPU path runs ops/csrc/fwfm_kernels.hip
(per-field sums in LDS, O(nf^2 K) a row) and DeepFM's sparse tail
(fm_sorted_apply, bitmap_compact, fused Adagrad / FTRL); R takes a dense
Adagrad step of its own. The CPU path uses ops/fwfm_ref.py.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import fm_ref, fwfm_ref
from ..ops._extension import require_hip_ops, sort_ids
from ..utils.checks import validate_csr_batch
from ..utils.metrics import auc_score
from .embed_bag import load_checkpoint


@dataclass
class FwFMHyper:
    num_features: int
    num_fields: int
    k: int = 16
    optimizer: str = "adagrad"  # adagrad | ftrl, for W and V
    lr: float = 0.1
    eps: float = 1e-8
    l2: float = 1e-5
    ftrl_alpha: float = 0.15
    ftrl_beta: float = 1.0
    ftrl_l1: float = 1e-4
    ftrl_l2: float = 1e-4
    ftrl_v: str = "adagrad"  # latent updater under ftrl (see models/fm.py)
    r_lr: float = 0.01  # dense Adagrad on R (no l2)
    r_init: float = 1.0
    init_sigma: float = 0.01
    seed: int = 1234


class FwFMModel:
    def __init__(self, hyper: FwFMHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22):
        self.h = hyper
        self.device = torch.device(device)
        F, nf, K = hyper.num_features, hyper.num_fields, hyper.k
        assert K in (4, 8, 16, 32, 64)
        assert hyper.optimizer in ("adagrad", "ftrl"), hyper.optimizer
        self._gpu = self.device.type == "cuda"
        if self._gpu:
            ops = require_hip_ops()
            # both kernels keep R and per-wave [nf, K] tiles in LDS
            need = ops.fwfm_lds_bytes(nf, K)
            have = ops.ffm_max_lds_per_block()
            if need > have:
                raise ValueError(
                    f"num_fields={nf}, k={K}: the FwFM kernels need {need} "
                    f"bytes of LDS per block, the device gives {have}")
        g = torch.Generator().manual_seed(hyper.seed)
        self.W = torch.zeros(F, device=self.device)
        self.V = (torch.randn(F, K, generator=g) * hyper.init_sigma).to(
            self.device)
        self.R = torch.full((nf, nf), float(hyper.r_init),
                            device=self.device)
        self.gradW = torch.zeros_like(self.W)
        self.gradV = torch.zeros_like(self.V)
        self.nW = torch.zeros_like(self.W)
        self.nV = torch.zeros_like(self.V)
        self.nR = torch.zeros_like(self.R)
        if hyper.optimizer == "ftrl":
            self.zW = torch.zeros_like(self.W)
            self.zV = torch.zeros_like(self.V)
        nwords = (F + 63) // 64
        self.touched = torch.zeros(nwords, dtype=torch.int64,
                                   device=self.device)
        cap = min(F, max_batch_nnz)
        self.uniq = torch.zeros(cap, dtype=torch.int32, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._fields_checked = False

    def forward(self, row_ptr, fields, fids, vals):
        if self._gpu:
            return require_hip_ops().fwfm_forward(row_ptr, fields, fids,
                                                  vals, self.W, self.V,
                                                  self.R)
        return fwfm_ref.fwfm_forward_ref(row_ptr, fields, fids, vals, self.W,
                                         self.V, self.R)

    def predict_proba(self, row_ptr, fields, fids, vals):
        pred = self.forward(row_ptr, fields, fids, vals)
        return torch.sigmoid(torch.clamp(pred, -16, 16))

    def train_step(self, row_ptr, fields, fids, vals, labels) -> torch.Tensor:
        B = row_ptr.numel() - 1
        if B == 0:
            return torch.zeros(0, device=self.device)
        scale = 1.0 / B
        validate_csr_batch(row_ptr, fids, vals, self.h.num_features,
                           fields, self.h.num_fields)
        if not self._fields_checked:
            # one-time guard, as in FFMModel: the kernels leave an entry
            # with a field outside [0, nf) out of the pair term, which a
            # mislabelled data set should not be trained through silently
            # (costs one sync, once)
            if fields.numel():
                fmin, fmax = int(fields.min()), int(fields.max())
                assert 0 <= fmin and fmax < self.h.num_fields, \
                    f"field ids [{fmin}, {fmax}] outside " \
                    f"num_fields {self.h.num_fields}"
            self._fields_checked = True
        h = self.h
        if self._gpu:
            ops = require_hip_ops()
            pred = ops.fwfm_forward(row_ptr, fields, fids, vals, self.W,
                                    self.V, self.R)
            loss, dpred = ops.logloss_grad(pred, labels, scale)
            gw, gv, dR = ops.fwfm_backward_emit(row_ptr, fields, fids, vals,
                                                self.V, self.R, dpred)
            sorted_fids, perm = sort_ids(fids, h.num_features)
            ops.fm_sorted_apply(sorted_fids, perm, gw, gv, self.gradW,
                                self.gradV, self.touched)
            self.count.zero_()
            ops.bitmap_compact(self.touched, self.uniq, self.count)
            live = self.uniq[: min(self.uniq.numel(), fids.numel())]
            if h.optimizer == "ftrl":
                ops.fm_ftrl_apply(live, self.count, self.W, self.V,
                                  self.zW, self.nW, self.zV, self.nV,
                                  self.gradW, self.gradV, h.ftrl_alpha,
                                  h.ftrl_beta, h.ftrl_l1, h.ftrl_l2,
                                  1 if h.ftrl_v == "adagrad" else 0,
                                  h.lr, h.eps, h.l2)
            else:
                ops.fm_adagrad_apply(live, self.count, self.W, self.V,
                                     self.nW, self.nV, self.gradW, self.gradV,
                                     h.lr, h.eps, h.l2)
            # the lower triangle has zero gradient and never moves
            ops.dense_adagrad(self.R, dR, self.nR, None, None, h.r_lr, h.eps,
                              0.0)
            return loss
        # CPU oracle
        pred = fwfm_ref.fwfm_forward_ref(row_ptr, fields, fids, vals, self.W,
                                         self.V, self.R)
        loss, dpred = fm_ref.logloss_grad_ref(pred, labels, scale)
        gw, gv, dR = fwfm_ref.fwfm_backward_emit_ref(
            row_ptr, fields, fids, vals, self.V, self.R, dpred)
        f = fids.long()
        self.gradW.index_add_(0, f, gw)
        self.gradV.index_add_(0, f, gv)
        uniq = torch.unique(f).int()
        if h.optimizer == "ftrl":
            fm_ref.ftrl_apply_ref(uniq, self.W, self.V, self.zW, self.nW,
                                  self.zV, self.nV, self.gradW, self.gradV,
                                  h.ftrl_alpha, h.ftrl_beta, h.ftrl_l1,
                                  h.ftrl_l2, v_adagrad=h.ftrl_v == "adagrad",
                                  v_lr=h.lr, v_eps=h.eps, v_l2=h.l2)
        else:
            fm_ref.adagrad_apply_ref(uniq, self.W, self.V, self.nW, self.nV,
                                     self.gradW, self.gradV, h.lr, h.eps,
                                     h.l2)
        self.nR.add_(dR * dR)
        self.R.sub_(h.r_lr * dR * torch.rsqrt(self.nR + h.eps))
        return loss

    def state_dict(self) -> dict:
        d = {"W": self.W, "V": self.V, "R": self.R, "nW": self.nW,
             "nV": self.nV, "nR": self.nR, "hyper": self.h.__dict__}
        if self.h.optimizer == "ftrl":
            d["zW"], d["zV"] = self.zW, self.zV
        return d

    def save(self, path: str) -> None:
        torch.save(self.state_dict(), path)

    def load(self, path) -> None:
        d = load_checkpoint(path, self.device)
        for name in ("W", "V", "R", "nW", "nV", "nR"):
            getattr(self, name).copy_(d[name])
        if self.h.optimizer == "ftrl" and "zW" in d:
            self.zW.copy_(d["zW"])
            self.zV.copy_(d["zV"])


class FwFMTrainer:
    """Reference-shaped API: ctor(dataset, hyper) -> train() -> save()."""

    def __init__(self, dataset, hyper: FwFMHyper, device: str = "cpu",
                 batch_size: int = 256, epochs: int = 5):
        self.ds = dataset
        self.model = FwFMModel(hyper, device=device)
        self.batch_size = batch_size
        self.epochs = epochs
        self.device = torch.device(device)

    def train(self, log=print):
        ds = self.ds.to(self.device)
        N = ds.num_rows
        for ep in range(self.epochs):
            tot, nb = 0.0, 0
            for s in range(0, N, self.batch_size):
                b = ds.slice_rows(s, min(s + self.batch_size, N))
                loss = self.model.train_step(b.row_ptr, b.fields, b.fids,
                                             b.vals, b.labels)
                tot += float(loss.mean())
                nb += 1
            if log:
                log(f"epoch {ep}: loss={tot / max(nb, 1):.5f}")
        return self

    def evaluate(self, dataset=None) -> dict:
        ds = (dataset or self.ds).to(self.device)
        p = self.model.predict_proba(ds.row_ptr, ds.fields, ds.fids, ds.vals)
        loss = torch.nn.functional.binary_cross_entropy(
            p.clamp(1e-7, 1 - 1e-7), ds.labels)
        return {
            "auc": auc_score(p.cpu(), ds.labels.cpu()),
            "logloss": float(loss),
            "accuracy": float(((p > 0.5) == (ds.labels > 0.5)).float().mean()),
        }
