"""Field-addressed concat layout shared by Wide&Deep and DeepFM
(layout="field"): the hyper check, the models' common state and the CPU
paths of ops/csrc/embed_bag_kernels.hip in the kernels' operation order.

    deep_in[r, c*K+k] = inv(r,c) sum_{j in row r, fields[j] == c} E[f_j,k] x_j

inv is 1 (pooling="sum") or 1 / (number of entries in the slot) ("mean");
empty slots are +0; an entry whose field is outside [0, nf) is left out.
"""

from __future__ import annotations

import torch

from ..ops._extension import require_hip_ops


def check_bag_hyper(hyper, gpu):
    """layout / pooling of a hyper; on a GPU also that the per-wave staging
    of the field layout fits the device's LDS"""
    if hyper.layout not in ("position", "field"):
        raise ValueError(f"unknown layout {hyper.layout!r}")
    if hyper.pooling not in ("sum", "mean"):
        raise ValueError(f"unknown pooling {hyper.pooling!r}")
    if gpu and hyper.layout == "field":
        ops = require_hip_ops()
        need = ops.embed_bag_lds_bytes(hyper.num_fields, hyper.k)
        have = ops.ffm_max_lds_per_block()
        if need > have:
            raise ValueError(
                f"layout='field' with num_fields={hyper.num_fields}, "
                f"k={hyper.k} needs {need} bytes of LDS per block, the "
                f"device gives {have}")


class BagLayout:
    """What a model with the two concat layouts keeps: whether the concat is
    addressed by field, the pooling code of the bindings, and the rule for
    the `fields` argument of train_step / predict_proba."""

    def _init_bag(self, hyper, device):
        check_bag_hyper(hyper, device.type == "cuda")
        self._field = hyper.layout == "field"
        self._pool = 1 if hyper.pooling == "mean" else 0

    def _fields(self, fields):
        """the fields array the field layout needs; None under "position",
        where the argument is ignored"""
        if not self._field:
            return None
        if fields is None:
            raise ValueError('layout="field" needs the fields array')
        return fields


def bag_slots(row_ptr, fields, nf):
    """entry -> (row index, kept mask, flat slot row*nf + field (0 where not
    kept), slot count as fp32 [B*nf]) of the field layout"""
    B = row_ptr.numel() - 1
    rp = row_ptr.long()
    row_idx = torch.repeat_interleave(torch.arange(B), rp[1:] - rp[:-1])
    c = fields.long()
    keep = (c >= 0) & (c < nf)
    flat = torch.where(keep, row_idx * nf + c, torch.zeros_like(c))
    cnt = torch.zeros(B * nf).index_add_(0, flat[keep],
                                         torch.ones(int(keep.sum())))
    return row_idx, keep, flat, cnt


def bag_inv(cnt, pooling):
    """per-slot multiplier: 1 (sum) or the correctly rounded 1/cnt (mean)"""
    if pooling == "mean":
        return 1.0 / cnt.clamp(min=1.0)
    return torch.ones_like(cnt)


def bag_gather_cpu(E, row_ptr, fields, fids, vals, nf, pooling):
    """deep_in [B, nf*K] of the field layout in the kernel's operation
    order: fp32 sum of the slot's products in entry order from +0, then one
    multiply by inv (kept fp32 here, like the position gather; the kernel
    rounds the result to bf16 for the GEMM)"""
    B, K = row_ptr.numel() - 1, E.shape[1]
    _, keep, flat, cnt = bag_slots(row_ptr, fields, nf)
    vx = E[fids.long()] * vals.unsqueeze(1)
    out = torch.zeros(B * nf, K).index_add_(0, flat[keep], vx[keep])
    out = out * bag_inv(cnt, pooling).unsqueeze(1)
    return out.view(B, nf * K)


def bag_dgather_cpu(dDeep, row_ptr, fields, nf, K, pooling):
    """per-entry D inv [nnz, K]: the deep gradient of the entry's slot times
    the slot's inv, 0 for an entry outside the concat"""
    B = row_ptr.numel() - 1
    _, keep, flat, cnt = bag_slots(row_ptr, fields, nf)
    D = dDeep.reshape(B * nf, K)[flat] * bag_inv(cnt, pooling)[flat] \
        .unsqueeze(1)
    return torch.where(keep.unsqueeze(1), D, torch.zeros_like(D))


def load_checkpoint(path_or_dict, device):
    """a checkpoint given as a path or as the dict already read from it"""
    if isinstance(path_or_dict, dict):
        return path_or_dict
    return torch.load(path_or_dict, map_location=device, weights_only=True)
