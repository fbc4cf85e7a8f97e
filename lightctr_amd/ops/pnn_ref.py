"""Pure-PyTorch reference for PNN's inner-product layer (CPU path and baseline
arm). x0 [B, nf*K] is the concat row, viewed as e [B, nf, K]:

  g[b, p(i,j)] = e_i . e_j          i < j, p the row-major strict upper
                                    triangle (torch.triu_indices(nf, nf, 1))
  z[b]         = [x0[b], g[b], 0 .. 0]      Dz = nf K + P up to a multiple of 8

and, from the gradient dz [B, Dz] of z, Gs the symmetric matrix of the pair
gradients with a zero diagonal,

  dDeep[b, i K + k] = dz[b, i K + k] + sum_j Gs[b, i, j] e[b, j, k]

in the dtype of the inputs and in chunks of rows, so [B, nf, nf] is never
whole. It is what ops/csrc/pnn_kernels.hip computes, and with rounding="bf16"
it rounds where those kernels round and nowhere else: g on output, and the
pair gradients before the product (the dz of the x0 columns is added
unrounded).
"""

from __future__ import annotations

import torch


def _rounder(rounding):
    if rounding is None:
        return lambda t: t
    if rounding != "bf16":
        raise ValueError(f"unknown rounding {rounding!r}")
    return lambda t: t.bfloat16().to(t.dtype)


def pnn_dims(nf, K):
    """(P, Dz): pairs, and the width of z"""
    P = nf * (nf - 1) // 2
    return P, (nf * K + P + 7) // 8 * 8


def pnn_forward_ref(x0, nf, rounding=None, chunk=1024):
    """z [B, Dz]"""
    rd = _rounder(rounding)
    B, d = x0.shape
    P, Dz = pnn_dims(nf, d // nf)
    i, j = torch.triu_indices(nf, nf, 1, device=x0.device)
    z = x0.new_zeros(B, Dz)
    z[:, :d] = x0
    for c in range(0, B, chunk):
        e = x0[c:c + chunk].view(-1, nf, d // nf)
        z[c:c + chunk, d:d + P] = rd((e @ e.transpose(1, 2))[:, i, j])
    return z


def pnn_backward_ref(z, dz, nf, K, rounding=None, chunk=1024):
    """dDeep [B, nf*K]; z's columns past nf*K and dz's pad are not read"""
    rd = _rounder(rounding)
    d, P = nf * K, pnn_dims(nf, K)[0]
    i, j = torch.triu_indices(nf, nf, 1, device=z.device)
    dDeep = dz[:, :d].clone()
    for c in range(0, z.shape[0], chunk):
        e = z[c:c + chunk, :d].reshape(-1, nf, K)
        Gs = e.new_zeros(e.shape[0], nf, nf)
        Gs[:, i, j] = rd(dz[c:c + chunk, d:d + P])
        Gs = Gs + Gs.transpose(1, 2)
        dDeep[c:c + chunk] += (Gs @ e).flatten(1)
    return dDeep
