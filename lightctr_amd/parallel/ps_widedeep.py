"""Wide&Deep under the asynchronous parameter server.

The reference's distributed Wide&Deep worker (distributed_algo_abst.h:
105-280) trains its wide LR weights and embeddings through the sparse PS
table and its fully-connected layers through the dense tensor table. Here
the worker pulls the touched sparse rows AND the whole fused MLP slab every
step, computes gradients locally, and pushes both back; the PS owns every
update (the local MLP optimizer is never called).

Fixed-fields rows (exactly `num_fields` entries per row, e.g. Criteo 39)
are required for the concat layout, as in models/wide_deep.py.
"""

from __future__ import annotations

import torch

from ..models.mlp import MLP
from ..ops import fm_ref
from .ps import PSConfig, PSWorker
from .ps_dense import dense_total, mlp_dense_spec


def widedeep_dims(hyper):
    """MLP layer widths of the deep half for a WideDeepHyper."""
    return [hyper.num_fields * hyper.k, *hyper.hidden, 1]


def widedeep_dense_spec(hyper):
    """PSConfig.dense_spec for the deep half of a WideDeepHyper."""
    return mlp_dense_spec(widedeep_dims(hyper))


def widedeep_grads(row_ptr, fids_local, vals, labels, Wl, El, mlp,
                   num_fields):
    """One Wide&Deep forward/backward over pulled parameters.

    fids_local index the pulled rows Wl [U] (wide weights) and El [U, K]
    (embeddings). Returns (per-row loss, gWl [U], gEl [U, K]) with the loss
    averaged over the batch in the gradients; the MLP gradients are left in
    the layers (mlp.flat_grads()). Pure: no parameter is modified.
    CPU: the torch math of WideDeepModel._forward_cpu / train_step.
    GPU: the same kernels as WideDeepModel.train_step."""
    B = row_ptr.numel() - 1
    U, K = El.shape
    scale = 1.0 / B
    if El.is_cuda:
        from ..ops._extension import require_hip_ops, sort_ids

        ops = require_hip_ops()
        dev = El.device
        wide = ops.wide_forward(row_ptr, fids_local, vals, Wl)
        deep_in = ops.embed_gather(row_ptr, fids_local, vals, El, num_fields)
        deep = mlp.forward(deep_in, train=True)
        pred = wide + deep[:, 0]
        loss, dpred = ops.logloss_grad(pred, labels, scale)
        dDeep = mlp.backward(dpred.unsqueeze(1))  # [B, nf*K]
        gw, gv = ops.embed_backward_emit(row_ptr, vals, dDeep.contiguous(),
                                         dpred, num_fields, K)
        sorted_l, perm = sort_ids(fids_local, U)
        gWl = torch.zeros(U, device=dev)
        gEl = torch.zeros(U, K, device=dev)
        bitmap = torch.zeros((U + 63) // 64, dtype=torch.int64, device=dev)
        ops.fm_sorted_apply(sorted_l, perm, gw, gv, gWl, gEl, bitmap)
        return loss, gWl, gEl
    nf = num_fields
    rp = row_ptr.long()
    f = fids_local.long()
    row_idx = torch.repeat_interleave(torch.arange(B), rp[1:] - rp[:-1])
    pos = torch.arange(f.numel()) - rp[:-1][row_idx]
    keep = pos < nf
    wide = torch.zeros(B)
    wide.index_add_(0, row_idx, Wl[f] * vals)
    deep_in = torch.zeros(B, nf * K)
    flat_idx = (row_idx * nf + pos).clamp(max=B * nf - 1)
    deep_in.view(B * nf, K).index_add_(
        0, flat_idx[keep], (El[f] * vals.unsqueeze(1))[keep])
    deep = mlp.forward(deep_in, train=True)
    pred = wide + deep[:, 0]
    loss, dpred = fm_ref.logloss_grad_ref(pred, labels, scale)
    dDeep = mlp.backward(dpred.unsqueeze(1))
    gWl = torch.zeros(U)
    gWl.index_add_(0, f, dpred[row_idx] * vals)
    dE = dDeep.view(B, nf, K)[row_idx, pos.clamp(max=nf - 1)] \
        * vals.unsqueeze(1)
    dE = torch.where(keep.unsqueeze(1), dE, torch.zeros_like(dE))
    gEl = torch.zeros(U, K)
    gEl.index_add_(0, f, dE)
    return loss, gWl, gEl


def ps_train_widedeep(cfg: PSConfig, group, gen_batch, steps: int, hyper,
                      device: str = "cpu", epoch_per_step: int = 1,
                      fin: bool = True, epoch_base: int = 0):
    """Worker-side Wide&Deep training loop against the PS (the sparse
    tables hold W and the embeddings, width cfg.k; cfg.dense_spec must be
    widedeep_dense_spec(hyper)). gen_batch(step) -> CSR batch on `device`.
    Per step: unique fids -> pull -> pull_dense -> load_flat ->
    widedeep_grads -> push -> push_dense. Returns per-step mean losses."""
    assert cfg.k == hyper.k, "sparse table width must be the embedding k"
    dims = widedeep_dims(hyper)
    assert dense_total(cfg.dense_spec) == dense_total(mlp_dense_spec(dims)), \
        "cfg.dense_spec does not match the hyper's MLP"
    worker = PSWorker(cfg, group, device=device)
    # parameter/gradient holder only: its optimizer is never stepped
    mlp = MLP(dims, optimizer=hyper.mlp_optimizer, lr=hyper.mlp_lr,
              dropout=hyper.dropout, seed=hyper.seed, device=device)
    losses = []
    for step in range(steps):
        epoch = epoch_base + step * epoch_per_step
        row_ptr, fids, vals, labels = gen_batch(step)
        uniq, inverse = torch.unique(fids.long(), return_inverse=True)
        Wl, El = worker.pull(uniq, epoch)
        mlp.load_flat(worker.pull_dense(epoch))
        loss, gWl, gEl = widedeep_grads(row_ptr, inverse.to(torch.int32),
                                        vals, labels, Wl, El, mlp,
                                        hyper.num_fields)
        worker.push(uniq, gWl, gEl, epoch)
        worker.push_dense(mlp.flat_grads(), epoch)
        losses.append(float(loss.mean()))
    if fin:
        worker.fin()
    return losses
