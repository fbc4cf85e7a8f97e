"""Factorization Machine — MI355X-native trainer.

Capability parity with the reference Train_FM_Algo
(/root/reference/LightCTR/train/train_fm_algo.{h,cpp}: ctor(data, epochs, k)
-> Train() -> saveModel(), O(nk) sumVX forward, fused grad accumulation,
Adagrad apply) — rebuilt GPU-first:

  * parameters W [F] and V [F,K] are flat fp32 slabs resident in HBM3E
  * the train step is a handful of HIP kernel launches with no device->host
    syncs. Default backward_mode="segment": training forward (loss fused
    in) beside a radix sort of the fids that makes and carries one (row, x)
    record per entry (overlap_sort; the sort reads only the batch and runs
    on a second stream), and a tile-local segment reduce: every block
    finds the pieces
    of its own tile of sorted entries, recomputes the gradients and applies
    the optimizer in place. "segment_list" (the per-piece reduce fed by a
    global work list), "segment_emit" (that reduce fed by a per-entry
    gradient emit), "sorted" (walk into slabs + bitmap compact + sparse
    optimizer) and "atomic" (scatter backward) stay selectable
  * CPU path uses the fp32 torch reference ops (same math; the test oracle)
  * optimizers: adagrad (reference default) and FTRL-proximal (BASELINE
    config #2: "FM k=16 ... FTRL fused update"); both are applied only to
    the features touched by the batch, exactly like the reference's sparse
    updaters.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ..ops import fm_ref
from ..ops._extension import (require_hip_ops, sort_end_bit, sort_ids,
                              sort_ids_rec)
from ..utils.checks import validate_csr_batch
from ..utils.metrics import auc_score


@dataclass
class FMHyper:
    num_features: int
    k: int = 16
    optimizer: str = "adagrad"  # adagrad | ftrl
    lr: float = 0.1
    eps: float = 1e-8
    l2: float = 1e-5
    ftrl_alpha: float = 0.15
    ftrl_beta: float = 1.0
    ftrl_l1: float = 1e-4
    ftrl_l2: float = 1e-4
    # latent-factor updater under optimizer="ftrl": "adagrad" (default —
    # FTRL's L1 starves interactions, measured 0.66 vs 0.79 AUC) | "ftrl"
    ftrl_v: str = "adagrad"
    init_sigma: float = 0.01
    seed: int = 1234


class FMModel:
    """Owns parameters + optimizer state + scratch slabs on one device."""

    def __init__(self, hyper: FMHyper, device: str = "cpu",
                 max_batch_nnz: int = 1 << 22):
        self.h = hyper
        self.device = torch.device(device)
        F, K = hyper.num_features, hyper.k
        assert K in (4, 8, 16, 32, 64), "K must divide the 64-lane wavefront"
        g = torch.Generator().manual_seed(hyper.seed)
        self.W = torch.zeros(F, device=self.device)
        self.V = (
            torch.randn(F, K, generator=g) * hyper.init_sigma
        ).to(self.device)
        self.gradW = torch.zeros_like(self.W)
        self.gradV = torch.zeros_like(self.V)
        # optimizer state
        self.nW = torch.zeros_like(self.W)
        self.nV = torch.zeros_like(self.V)
        if hyper.optimizer == "ftrl":
            self.zW = torch.zeros_like(self.W)
            self.zV = torch.zeros_like(self.V)
        # touched bitmap + compaction buffers
        nwords = (F + 63) // 64
        self.touched = torch.zeros(nwords, dtype=torch.int64, device=self.device)
        cap = min(F, max_batch_nnz)
        self.uniq = torch.zeros(cap, dtype=torch.int32, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._use_hip = self.device.type == "cuda"
        # "segment" (default) | "segment_list" | "segment_emit" | "sorted"
        # | "atomic"
        # segment: sort, then one K-lane subgroup per piece (a run of equal
        # fids cut at multiples of segment_cap) sums its gradients and, for
        # a run that fits one piece, applies the optimizer in place; only
        # runs crossing a cut go through the slabs + the sparse apply, with
        # uniq/count as their spill list. No bitmap pass in this mode.
        # The training forward writes one (row, x) record per entry, the
        # sort carries it as payload and the reduce recomputes each entry's
        # gradient from it: no per-entry gradient buffer, no loss kernel.
        # A block owns a tile of sorted entries and finds its pieces itself
        # (the tile is a multiple of segment_cap; a cap that does not divide
        # it takes the list path).
        # segment_list: the pieces come from a global work list (three
        # library launches) and one subgroup walks each piece.
        # segment_emit: the same reduce fed by fm_backward_emit's per-entry
        # gradients through the sort permutation (the earlier pipeline,
        # kept for A/B).
        self.backward_mode = "segment"
        self.segment_cap = 256  # power of two; sweep in docs/KERNELS.md
        # fused-apply: interior feature segments get their optimizer update
        # inside the segment-reduce kernel. Measured NET-NEGATIVE in both
        # rounds (round 1: optimizer RMWs serialize the segment walk,
        # apply 185->385us vs separate pass 132->37us; round 2, mode 3
        # ftrlW+adagradV: 721 vs 693 us/step — the boundary-fid bitmap
        # pass still runs and the heavier flush costs more than the
        # separate ~110 us sparse apply saves;
        # profiles/r2_06_fm_step_fused_ab.txt). Two-phase stays default;
        # kept selectable + parity tested.
        self.fused_apply = False
        # record sort of the segment modes: "onesweep" (the single-purpose
        # sort of sort_kernels.hip) | "rocprim"; same permutation either way.
        # sort_status is the word a bounded look-back spin of the onesweep
        # sort marks on give-up; it stays 0 in a healthy run.
        self.sort_impl = "onesweep"
        self.sort_status = torch.zeros(1, dtype=torch.int32,
                                       device=self.device)
        # front half of "segment" / "segment_list" with the onesweep sort.
        # True: the sort makes the records itself (its first scatter pass
        # reads fids and vals and looks each entry's row up in row_ptr; no
        # record exists in batch order) and runs on a pool stream beside a
        # forward that writes none; the two join in front of the reduce.
        # "serial": the same launches in
        # sequence on one stream. False: the forward writes the records and
        # the sort follows it (the earlier sequence). All three hand the
        # reduce a bit-identical sorted stream; measurements in
        # profiles/r7_01_fm_overlap.txt.
        self.overlap_sort = True
        if self._use_hip:
            require_hip_ops()  # fail loudly if extension missing on GPU

    # -- forward/inference --------------------------------------------------
    def forward(self, row_ptr, fids, vals):
        if self._use_hip:
            ops = require_hip_ops()
            pred, sumVX = ops.fm_forward(row_ptr, fids, vals, self.W, self.V)
        else:
            pred, sumVX = fm_ref.fm_forward_ref(row_ptr, fids, vals, self.W, self.V)
        return pred, sumVX

    def predict_proba(self, row_ptr, fids, vals):
        pred, _ = self.forward(row_ptr, fids, vals)
        return torch.sigmoid(torch.clamp(pred, -16, 16))

    # -- one fused training step -------------------------------------------
    def train_step(self, row_ptr, fids, vals, labels) -> torch.Tensor:
        """Runs fwd+loss+bwd+optimizer. Returns per-row loss tensor (device);
        caller reduces/syncs only when it wants the number."""
        B = row_ptr.numel() - 1
        scale = 1.0 / B
        validate_csr_batch(row_ptr, fids, vals, self.h.num_features)
        if self._use_hip:
            ops = require_hip_ops()
            # fused_apply is a variant of the walk: asking for it selects
            # the sorted path
            if (self.backward_mode in ("segment", "segment_list")
                    and not self.fused_apply):
                tiled = (self.backward_mode == "segment"
                         and self._cap_tiles(ops))
                end_bit = sort_end_bit(self.h.num_features)
                if (self.overlap_sort and self.sort_impl == "onesweep"
                        and end_bit <= 31 and fids.numel() < (1 << 30)):
                    # the sort makes the records itself and needs nothing
                    # of the model: one call enqueues it and the forward,
                    # on two streams unless overlap_sort == "serial"
                    loss, dpred, sumVX, sorted_fids, sorted_rec = (
                        ops.fm_forward_train_sorted(
                            row_ptr, fids, vals, self.W, self.V, labels,
                            scale, end_bit,
                            reset=self.count if tiled else None,
                            status=self.sort_status,
                            overlap=self.overlap_sort != "serial"))
                    self._segment_reduce(ops, sorted_fids, sorted_rec, sumVX,
                                         dpred, tiled)
                    return loss
                # the work-list pass resets the spill counter; without it
                # the forward does
                loss, dpred, sumVX, rec = ops.fm_forward_train(
                    row_ptr, fids, vals, self.W, self.V, labels, scale,
                    reset=self.count if tiled else None)
                self._segment_backward(ops, fids, sumVX, dpred, rec, tiled)
                return loss
            pred, sumVX = ops.fm_forward(row_ptr, fids, vals, self.W, self.V)
            loss, dpred = ops.logloss_grad(pred, labels, scale)
            if (self.backward_mode == "segment_emit"
                    and not self.fused_apply):
                self._segment_emit_backward(ops, row_ptr, fids, vals, sumVX,
                                            dpred)
                return loss
            if self.backward_mode in ("sorted", "segment", "segment_list",
                                      "segment_emit"):
                # contention-free backward: emit per-entry grads
                # (coalesced), bit-range radix-sort the fids, then
                # segment-reduce into the slabs with interior-store
                # flushes (see profiles/ and fm_kernels.hip for the
                # measured evolution incl. the reverted scatter-emit and
                # segmented-scan variants)
                sorted_fids, perm = sort_ids(fids, self.h.num_features)
                gw, gv = ops.fm_backward_emit(row_ptr, fids, vals, self.V,
                                              sumVX, dpred)
                if self.fused_apply:
                    if (self.h.optimizer == "ftrl"
                            and self.h.ftrl_v == "adagrad"):
                        # round 2: mode 3 = FTRL on W + Adagrad on V (the
                        # default pairing) fused into the segment reduce;
                        # only boundary-spanning fids take the slab +
                        # bitmap + sparse-apply pass
                        ops.fm_sorted_apply_fused(
                            sorted_fids, perm, gw, gv, self.gradW,
                            self.gradV, self.touched, self.W, self.V,
                            self.nW, self.nV, self.zW, None, 3,
                            self.h.ftrl_alpha, self.h.ftrl_beta,
                            self.h.ftrl_l1, self.h.ftrl_l2,
                            v_lr=self.h.lr, v_eps=self.h.eps,
                            v_l2=self.h.l2)
                    elif self.h.optimizer == "ftrl":
                        ops.fm_sorted_apply_fused(
                            sorted_fids, perm, gw, gv, self.gradW,
                            self.gradV, self.touched, self.W, self.V,
                            self.nW, self.nV, self.zW, self.zV, 2,
                            self.h.ftrl_alpha, self.h.ftrl_beta,
                            self.h.ftrl_l1, self.h.ftrl_l2)
                    else:
                        ops.fm_sorted_apply_fused(
                            sorted_fids, perm, gw, gv, self.gradW,
                            self.gradV, self.touched, self.W, self.V,
                            self.nW, self.nV, None, None, 1, self.h.lr,
                            self.h.eps, self.h.l2, 0.0)
                else:
                    ops.fm_sorted_apply(sorted_fids, perm, gw, gv,
                                        self.gradW, self.gradV,
                                        self.touched)
            else:
                ops.fm_backward(row_ptr, fids, vals, self.V, sumVX, dpred,
                                self.gradW, self.gradV, self.touched)
            self.count.zero_()
            ops.bitmap_compact(self.touched, self.uniq, self.count)
            live = self.uniq[: min(self.uniq.numel(), fids.numel())]
            self._sparse_apply(ops, live)
            return loss
        # CPU reference path
        pred, sumVX = fm_ref.fm_forward_ref(row_ptr, fids, vals, self.W, self.V)
        loss, dpred = fm_ref.logloss_grad_ref(pred, labels, scale)
        gW, gV = fm_ref.fm_backward_ref(row_ptr, fids, vals, self.V, sumVX, dpred)
        self.gradW += gW
        self.gradV += gV
        uniq = torch.unique(fids.long()).int()
        if self.h.optimizer == "ftrl":
            fm_ref.ftrl_apply_ref(uniq, self.W, self.V, self.zW, self.nW,
                                  self.zV, self.nV, self.gradW, self.gradV,
                                  self.h.ftrl_alpha, self.h.ftrl_beta,
                                  self.h.ftrl_l1, self.h.ftrl_l2,
                                  v_adagrad=self.h.ftrl_v == "adagrad",
                                  v_lr=self.h.lr, v_eps=self.h.eps,
                                  v_l2=self.h.l2)
        else:
            fm_ref.adagrad_apply_ref(uniq, self.W, self.V, self.nW, self.nV,
                                     self.gradW, self.gradV, self.h.lr,
                                     self.h.eps, self.h.l2)
        return loss

    def _opt_mode(self) -> int:
        """Kernel-side optimizer pairing: 1 Adagrad, 2 FTRL, 3 FTRL-W +
        Adagrad-V."""
        if self.h.optimizer != "ftrl":
            return 1
        return 3 if self.h.ftrl_v == "adagrad" else 2

    def _sparse_apply(self, ops, live):
        """Optimizer over the fid list live[:count]; re-zeroes the slab
        entries it consumes."""
        if self.h.optimizer == "ftrl":
            ops.fm_ftrl_apply(live, self.count, self.W, self.V,
                              self.zW, self.nW, self.zV, self.nV,
                              self.gradW, self.gradV, self.h.ftrl_alpha,
                              self.h.ftrl_beta, self.h.ftrl_l1,
                              self.h.ftrl_l2,
                              1 if self.h.ftrl_v == "adagrad" else 0,
                              self.h.lr, self.h.eps, self.h.l2)
        else:
            ops.fm_adagrad_apply(live, self.count, self.W, self.V,
                                 self.nW, self.nV, self.gradW, self.gradV,
                                 self.h.lr, self.h.eps, self.h.l2)

    def _cap_tiles(self, ops) -> bool:
        """The tile reduce needs whole pieces per tile: segment_cap must
        divide the tile."""
        tile, cap = ops.fm_segment_tile(), int(self.segment_cap)
        return cap <= tile and tile % cap == 0

    def _segment_pieces(self, ops, sorted_fids, worklist=True):
        """Work list (unless the reduce finds its pieces itself) + spill
        list + optimizer arguments shared by the segment modes."""
        nnz = sorted_fids.numel()
        cap = int(self.segment_cap)
        if worklist:
            # the work-list pass also resets the spill counter
            lists = tuple(ops.segment_worklist(sorted_fids, cap, self.count))
        else:
            lists = (cap,)
        # a spilled run crosses a multiple of cap, and is a distinct fid
        spill = self.uniq[: min(self.uniq.numel(), nnz // cap + 1)]
        mode = self._opt_mode()
        if mode == 1:
            knobs = (self.h.lr, self.h.eps, self.h.l2, 0.0)
        else:
            knobs = (self.h.ftrl_alpha, self.h.ftrl_beta, self.h.ftrl_l1,
                     self.h.ftrl_l2)
        tail = (*lists, self.gradW, self.gradV, spill,
                self.count, self.W, self.V, self.nW, self.nV,
                self.zW if mode != 1 else None,
                self.zV if mode == 2 else None, mode, *knobs)
        kw = dict(v_lr=self.h.lr, v_eps=self.h.eps, v_l2=self.h.l2)
        return spill, tail, kw

    def _segment_backward(self, ops, fids, sumVX, dpred, rec, tiled):
        """Recompute reduce: the sort carries the forward's (row, x) records
        and the reduce forms every entry's gradient itself; tiled: without
        a work list (backward_mode="segment"), else list-fed
        ("segment_list")."""
        if fids.numel() == 0:
            return
        sorted_fids, sorted_rec = sort_ids_rec(
            fids, rec, self.h.num_features, impl=self.sort_impl,
            status=self.sort_status)
        self._segment_reduce(ops, sorted_fids, sorted_rec, sumVX, dpred,
                             tiled)

    def _segment_reduce(self, ops, sorted_fids, sorted_rec, sumVX, dpred,
                        tiled):
        """Back half of the segment modes: reduce over the sorted stream,
        then the optimizer over the spilled runs."""
        if sorted_fids.numel() == 0:
            return
        spill, tail, kw = self._segment_pieces(ops, sorted_fids,
                                               worklist=not tiled)
        reduce = (ops.fm_segment_tile_rec if tiled
                  else ops.fm_segment_apply_rec)
        reduce(sorted_fids, sorted_rec, sumVX, dpred, *tail, **kw)
        self._sparse_apply(ops, spill)

    def _segment_emit_backward(self, ops, row_ptr, fids, vals, sumVX, dpred):
        """Emit-fed reduce (backward_mode="segment_emit"): per-entry
        gradients written in CSR order and gathered through the sort
        permutation."""
        if fids.numel() == 0:
            return
        sorted_fids, perm = sort_ids(fids, self.h.num_features)
        gw, gv = ops.fm_backward_emit(row_ptr, fids, vals, self.V, sumVX,
                                      dpred)
        spill, tail, kw = self._segment_pieces(ops, sorted_fids)
        ops.fm_segment_apply(sorted_fids, perm, tail[0], tail[1], gw, gv,
                             *tail[2:], **kw)
        self._sparse_apply(ops, spill)

    # -- checkpoint (reference saveModel/loadModel, fm_algo_abst.h:109-135) --
    def state_dict(self) -> dict:
        d = {"W": self.W, "V": self.V, "nW": self.nW, "nV": self.nV,
             "hyper": self.h.__dict__}
        if self.h.optimizer == "ftrl":
            d["zW"], d["zV"] = self.zW, self.zV
        return d

    def save(self, path: str) -> None:
        torch.save(self.state_dict(), path)

    def load(self, path: str) -> None:
        d = torch.load(path, map_location=self.device, weights_only=True)
        self.W.copy_(d["W"])
        self.V.copy_(d["V"])
        self.nW.copy_(d["nW"])
        self.nV.copy_(d["nV"])
        if self.h.optimizer == "ftrl" and "zW" in d:
            self.zW.copy_(d["zW"])
            self.zV.copy_(d["zV"])


class FMTrainer:
    """Reference-shaped API: ctor(dataset, hyper) -> Train() -> save()."""

    def __init__(self, dataset, hyper: FMHyper, device: str = "cpu",
                 batch_size: int = 256, epochs: int = 5):
        self.ds = dataset
        self.model = FMModel(hyper, device=device)
        self.batch_size = batch_size
        self.epochs = epochs
        self.device = torch.device(device)

    def train(self, log=print):
        ds = self.ds.to(self.device)
        N = ds.num_rows
        for ep in range(self.epochs):
            total_loss = 0.0
            nb = 0
            for s in range(0, N, self.batch_size):
                e = min(s + self.batch_size, N)
                b = ds.slice_rows(s, e)
                loss = self.model.train_step(b.row_ptr, b.fids, b.vals, b.labels)
                total_loss += float(loss.mean())
                nb += 1
            if log:
                log(f"epoch {ep}: loss={total_loss / max(nb, 1):.5f}")
        return self

    def evaluate(self, dataset=None) -> dict:
        ds = (dataset or self.ds).to(self.device)
        p = self.model.predict_proba(ds.row_ptr, ds.fids, ds.vals)
        loss = torch.nn.functional.binary_cross_entropy(
            p.clamp(1e-7, 1 - 1e-7), ds.labels
        )
        return {
            "auc": auc_score(p.cpu(), ds.labels.cpu()),
            "logloss": float(loss),
            "accuracy": float(((p > 0.5) == (ds.labels > 0.5)).float().mean()),
        }
