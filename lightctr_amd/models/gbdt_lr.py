"""GBDT+LR stacking — the CTR recipe the reference README describes for
its GBM: all features go into the tree ensemble, every leaf is a user
group, and a linear model then classifies on the 0/1 leaf-membership
features.

Stage 1 is GBMModel; its forest is compiled once (predict.CompiledForest)
and ``transform`` turns dense rows into one leaf feature per tree. Stage 2
is the sparse LRModel trained on those CSR batches through the shared
fused ``train_step``.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import torch

from ..predict.forest import CompiledForest
from .gbm import GBMHyper, GBMModel, Tree
from .lr import LRHyper, LRModel


@dataclass
class GBDTLRHyper:
    gbm: GBMHyper = field(default_factory=GBMHyper)
    lr_optimizer: str = "adagrad"
    lr_lr: float = 0.1
    epochs: int = 5
    batch: int = 256
    seed: int = 1234


class GBDTLRModel:
    def __init__(self, hyper: GBDTLRHyper, device: str = "cpu"):
        if hyper.gbm.n_classes > 2:
            raise ValueError("GBDT+LR is binary only (n_classes <= 2)")
        self.h = hyper
        self.device = torch.device(device)
        self.gbm = GBMModel(hyper.gbm, device=device)
        self.forest: CompiledForest | None = None
        self.lr: LRModel | None = None

    def _new_lr(self) -> LRModel:
        return LRModel(LRHyper(num_features=max(self.forest.n_leaves, 1),
                               optimizer=self.h.lr_optimizer,
                               lr=self.h.lr_lr, seed=self.h.seed),
                       device=str(self.device))

    def fit(self, X: torch.Tensor, y: torch.Tensor, log=None):
        X = X.to(self.device)
        y = y.float().to(self.device)
        self.gbm.fit(X, y, log=log)
        self.forest = self.gbm.compile()
        self.lr = self._new_lr()
        N, T = X.shape[0], self.forest.n_trees
        # one forest pass; every epoch re-batches the same leaf features
        fids = self.forest.transform(X).fids.view(N, T)
        g = torch.Generator().manual_seed(self.h.seed)
        for ep in range(self.h.epochs):
            perm = torch.randperm(N, generator=g).to(self.device)
            total, nb = 0.0, 0
            for s in range(0, N, self.h.batch):
                idx = perm[s:s + self.h.batch]
                B = idx.numel()
                row_ptr = torch.arange(0, B * T + 1, T, dtype=torch.int32,
                                       device=self.device)
                bf = fids[idx].reshape(-1).contiguous()
                vals = torch.ones(B * T, device=self.device)
                loss = self.lr.train_step(row_ptr, bf, vals, y[idx])
                if log:
                    total += float(loss.mean())
                    nb += 1
            if log:
                log(f"lr epoch {ep}: loss={total / max(nb, 1):.5f}")
        return self

    def predict_proba(self, X: torch.Tensor) -> torch.Tensor:
        if self.forest is None or self.lr is None:
            raise RuntimeError("GBDTLRModel is not fitted or loaded")
        f = self.forest.transform(X)
        return self.lr.predict_proba(f.row_ptr, f.fids, f.vals)

    # ---- checkpoint: the GBM file contents plus the LR state ----
    def save(self, path: str):
        torch.save({"hyper": {**{k: v for k, v in self.h.__dict__.items()
                                 if k != "gbm"},
                              "gbm": self.h.gbm.__dict__},
                    "gbm": {"hyper": self.gbm.h.__dict__,
                            "bin_edges": self.gbm.bin_edges,
                            "trees": [[t.__dict__ for t in rt]
                                      for rt in self.gbm.trees]},
                    "lr": self.lr.state_dict()}, path)

    def load(self, path: str):
        d = torch.load(path, map_location=self.device, weights_only=False)
        hd = dict(d["hyper"])
        self.h = GBDTLRHyper(gbm=GBMHyper(**hd.pop("gbm")), **hd)
        self.gbm = GBMModel(self.h.gbm, device=str(self.device))
        self.gbm.bin_edges = d["gbm"]["bin_edges"].to(self.device)
        self.gbm.trees = [[Tree(**td) for td in rt]
                          for rt in d["gbm"]["trees"]]
        self.forest = self.gbm.compile()
        self.lr = self._new_lr()
        for name in ("W", "V", "nW", "nV", "zW", "zV"):
            if name in d["lr"] and hasattr(self.lr, name):
                getattr(self.lr, name).copy_(d["lr"][name])
        return self
