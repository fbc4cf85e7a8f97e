"""Pure-PyTorch reference for AFM's pair attention (CPU path and baseline
arm). x0 [B, nf*K] is the concat row, viewed as e [B, nf, K]; Wa [K, A],
ba [A], qa [A], ua [K]:

  p_ij   = e_i * e_j                 i < j, P = nf (nf - 1) / 2 pairs
  z_ij   = Wa^T p_ij + ba
  s_ij   = qa . relu(z_ij)
  a      = softmax over the P pairs of s
  afm[b] = ua . sum_ij a_ij p_ij

with the backward written out (no autograd), in the dtype of its inputs and
in chunks of rows, so [B, P, K] is never whole. It is what
ops/csrc/afm_kernels.hip computes, and with rounding="bf16" it rounds where
those kernels round and nowhere else: the pair product as the operand of the
score product and of dWa (f, t, dua and dx0 read it unrounded), and dz as the
operand of dp and dWa (dba reads it unrounded). The ReLU mask reads z before
any rounding. The forward hands on lse [B], the log-sum-exp of the scores,
from which the backward recomputes the softmax.
"""

from __future__ import annotations

import torch


def _rounder(rounding):
    if rounding is None:
        return lambda t: t
    if rounding != "bf16":
        raise ValueError(f"unknown rounding {rounding!r}")
    return lambda t: t.bfloat16().to(t.dtype)


def _scores(x, Wa, ba, qa, nf, rd):
    """(e [b, nf, K], i, j, p [b, P, K], h = z + ba [b, P, A], s [b, P])"""
    e = x.view(x.shape[0], nf, x.shape[1] // nf)
    i, j = torch.triu_indices(nf, nf, 1, device=x.device)
    p = e[:, i] * e[:, j]
    h = rd(p) @ Wa + ba
    return e, i, j, p, h, torch.relu(h) @ qa


def afm_forward_ref(x0, Wa, ba, qa, ua, nf, rounding=None, chunk=1024):
    """(afm [B], lse [B])"""
    rd = _rounder(rounding)
    afm, lse = x0.new_empty(x0.shape[0]), x0.new_empty(x0.shape[0])
    for c in range(0, x0.shape[0], chunk):
        _, _, _, p, _, s = _scores(x0[c:c + chunk], Wa, ba, qa, nf, rd)
        lse[c:c + chunk] = torch.logsumexp(s, 1)
        a = torch.exp(s - lse[c:c + chunk, None])
        afm[c:c + chunk] = (a[:, :, None] * p).sum(1) @ ua
    return afm, lse


def afm_backward_ref(x0, lse, afm, Wa, ba, qa, ua, dpred, nf, rounding=None,
                     chunk=1024):
    """(dx0 [B, nf*K], dWa [K, A], dba, dqa, dua)"""
    rd = _rounder(rounding)
    dx0 = torch.zeros_like(x0)
    dWa, dba, dqa, dua = (torch.zeros_like(t) for t in (Wa, ba, qa, ua))
    for c in range(0, x0.shape[0], chunk):
        sl = slice(c, c + chunk)
        e, i, j, p, h, s = _scores(x0[sl], Wa, ba, qa, nf, rd)
        g = dpred[sl, None] * torch.exp(s - lse[sl, None])
        ds = g * (p @ ua - afm[sl, None])
        dz = ds[:, :, None] * qa * (h > 0)
        dzr = rd(dz)
        dba += dz.sum((0, 1))
        dqa += (ds[:, :, None] * torch.relu(h)).sum((0, 1))
        dua += (g[:, :, None] * p).sum((0, 1))
        dWa += torch.einsum("bpk,bpa->ka", rd(p), dzr)
        dp = dzr @ Wa.t() + g[:, :, None] * ua
        de = torch.zeros_like(e)
        de.index_add_(1, i, dp * e[:, j])
        de.index_add_(1, j, dp * e[:, i])
        dx0[sl] = de.flatten(1)
    return dx0, dWa, dba, dqa, dua
