"""Pure-PyTorch fp32 reference for the field-weighted FM ops (test oracle +
CPU path), in the per-field-sum form the HIP kernels use
(ops/csrc/fwfm_kernels.hip):

  S[r,a,k] = sum_{j in r, a_j = a} V[f_j,k] x_j
  Rs[a,b]  = R[min(a,b), max(a,b)]
  T[r,a,k] = sum_b Rs[a,b] S[r,b,k]
  pred[r]  = sum_j W[f_j] x_j + 0.5 (sum_a <S_a,T_a> - sum_a R[a,a] Q_a)
  Q[r,a]   = sum_{j in r, a_j = a} sum_k (V[f_j,k] x_j)^2

An entry whose field is outside [0, nf) counts in the wide term only.
"""

from __future__ import annotations

import torch


def _sym(R):
    """Rs: the upper triangle of R mirrored below the diagonal"""
    up = torch.triu(R)
    return up + torch.triu(R, 1).t()


def _field_sums(row_ptr, fields, fids, vals, V, nf):
    """(row_idx, in-range mask, clamped field, vx [nnz,K], S [B,nf,K])"""
    B = row_ptr.numel() - 1
    K = V.shape[1]
    rp = row_ptr.long()
    row_idx = torch.repeat_interleave(torch.arange(B, device=V.device),
                                      rp[1:] - rp[:-1])
    a = fields.long()
    ok = (a >= 0) & (a < nf)
    a = a.clamp(0, nf - 1)
    vx = V[fids.long()] * vals.unsqueeze(1)
    S = torch.zeros(B * nf, K, dtype=V.dtype, device=V.device)
    S.index_add_(0, (row_idx * nf + a)[ok], vx[ok])
    return row_idx, ok, a, vx, S.view(B, nf, K)


def fwfm_forward_ref(row_ptr, fields, fids, vals, W, V, R):
    """V: [F, K], R: [nf, nf]. Returns pred [B]."""
    B = row_ptr.numel() - 1
    nf = R.shape[0]
    row_idx, ok, a, vx, S = _field_sums(row_ptr, fields, fids, vals, V, nf)
    T = torch.einsum("ab,rbk->rak", _sym(R), S)
    lin = torch.zeros(B, dtype=V.dtype, device=V.device)
    lin.index_add_(0, row_idx, W[fids.long()] * vals)
    diag = torch.zeros(B, dtype=V.dtype, device=V.device)
    diag.index_add_(0, row_idx[ok],
                    (R.diagonal()[a] * (vx * vx).sum(dim=1))[ok])
    return lin + 0.5 * ((S * T).sum(dim=(1, 2)) - diag)


def fwfm_backward_emit_ref(row_ptr, fields, fids, vals, V, R, dpred):
    """Per-entry (gw [nnz], gv [nnz, K]) and dR [nf, nf] (zero below the
    diagonal)."""
    B = row_ptr.numel() - 1
    nf = R.shape[0]
    row_idx, ok, a, vx, S = _field_sums(row_ptr, fields, fids, vals, V, nf)
    T = torch.einsum("ab,rbk->rak", _sym(R), S)
    dx = dpred[row_idx] * vals
    gv = dx.unsqueeze(1) * (T[row_idx, a] - R.diagonal()[a].unsqueeze(1) * vx)
    gv = torch.where(ok.unsqueeze(1), gv, torch.zeros_like(gv))
    gram = torch.einsum("r,rak,rbk->ab", dpred, S, S)
    slot = (row_idx * nf + a)[ok]
    Q = torch.zeros(B * nf, dtype=V.dtype, device=V.device)
    Q.index_add_(0, slot, (vx * vx).sum(dim=1)[ok])
    cnt = torch.zeros(B * nf, dtype=V.dtype, device=V.device)
    cnt.index_add_(0, slot, torch.ones_like(Q[slot]))
    # pairs inside a field: 0.5 (<S_a,S_a> - Q_a), and exactly 0 (not the
    # rounding of that difference) where the field holds a single entry
    inner = 0.5 * ((S * S).sum(dim=2) - Q.view(B, nf))
    inner = torch.where(cnt.view(B, nf) > 1, inner, torch.zeros_like(inner))
    dR = torch.triu(gram, 1) + torch.diag(
        torch.einsum("r,ra->a", dpred, inner))
    return dx, gv, dR
