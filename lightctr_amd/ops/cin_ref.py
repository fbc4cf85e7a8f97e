"""Pure-PyTorch reference for xDeepFM's Compressed Interaction Network (CPU
path and baseline arm). x0 [B, nf*K] is the concat row, viewed as
X^0 [B, m = nf, D = K]; W is a list of L tensors, W^1 [H, m, m] and
W^l [H, H, m]; u [L, H]:

  X^l[b,h,d] = sum_{i,j} W^l[h,i,j] X^{l-1}[b,i,d] x0[b,j,d]
  cin[b]     = sum_l sum_h u[l,h] sum_d X^l[b,h,d]

with the backward written out (no autograd), in the dtype of its inputs and
chunked over the batch so that Z[b,d,i,j] = X^{l-1}[b,i,d] x0[b,j,d] stays
bounded. X and dX come in the kernels' row form [L, B, K, H]. It is what
ops/csrc/cin_kernels.hip computes, and with rounding="bf16" it rounds where
those kernels round and nowhere else: Z once; X^l and dX^l as saved and as
operands. The sums of cin read X^l before its rounding, du reads the saved
X^l, as the kernels do.

``cin_order`` is the kernels' order of (i, j) along a layer's reduction axis:
j in groups of 8 (m padded to a multiple of 8), i in blocks of 4.
"""

from __future__ import annotations

import torch


def _rounder(rounding):
    if rounding is None:
        return lambda t: t
    if rounding != "bf16":
        raise ValueError(f"unknown rounding {rounding!r}")
    return lambda t: t.bfloat16().to(t.dtype)


def cin_order(nf, h_prev):
    """(idx int64 [h_prev, nf], Kl): the column of W^l[:, i, j] in the
    kernels' [H, Kl] weight matrix; the other columns are padding (zero)."""
    nib = (h_prev + 3) // 4
    i = torch.arange(h_prev)[:, None]
    j = torch.arange(nf)[None, :]
    idx = (((j // 8) * nib + i // 4) * 4 + i % 4) * 8 + j % 8
    return idx, 32 * ((nf + 7) // 8) * nib


def _rows(x0, nf):
    B = x0.shape[0]
    return x0.view(B, nf, x0.shape[1] // nf).transpose(1, 2)  # [B, K, m]


def cin_forward_ref(x0, W, u, nf, rounding=None, chunk=1024):
    """(cin [B], X [L, B, K, H] = X^1 .. X^L)"""
    rd = _rounder(rounding)
    B, L, H = x0.shape[0], len(W), u.shape[1]
    K = x0.shape[1] // nf
    cin = x0.new_zeros(B)
    X = x0.new_zeros(L, B, K, H)
    for s in range(0, B, chunk):
        xr = _rows(x0[s:s + chunk], nf)
        xp = xr
        for l in range(L):
            Z = rd(xp[..., :, None] * xr[..., None, :]).flatten(2)
            xl = Z @ W[l].flatten(1).t()           # [b, K, H]
            cin[s:s + chunk] += xl.sum(1) @ u[l]
            xp = X[l, s:s + chunk] = rd(xl)
    return cin, X


def cin_backward_ref(x0, X, W, u, dpred, nf, rounding=None, chunk=1024):
    """(dx0 [B, nf*K], dX [L, B, K, H], dW list like W, du [L, H])"""
    rd = _rounder(rounding)
    B, L = x0.shape[0], len(W)
    dx0 = torch.zeros_like(x0)
    dX = torch.zeros_like(X)
    dW = [torch.zeros_like(w) for w in W]
    du = torch.zeros_like(u)
    for s in range(0, B, chunk):
        e = s + chunk
        xr, dp = _rows(x0[s:e], nf), dpred[s:e]
        dxr = torch.zeros_like(xr)
        down = torch.zeros_like(X[0, s:e])  # from the layer above to dX^l
        for l in range(L - 1, -1, -1):
            xp = X[l - 1, s:e] if l else xr
            du[l] += dp @ X[l, s:e].sum(1)
            g = dX[l, s:e] = rd(dp[:, None, None] * u[l] + down)
            Z = rd(xp[..., :, None] * xr[..., None, :])
            dW[l] += (g.flatten(0, 1).t() @ Z.flatten(0, 1).flatten(1)
                      ).view_as(W[l])
            dZ = (g @ W[l].flatten(1)).view_as(Z)
            down = (dZ * xr[..., None, :]).sum(-1)
            dxr = dxr + (dZ * xp[..., :, None]).sum(2)
        dx0[s:e] = (dxr + down).transpose(1, 2).reshape(dp.shape[0], -1)
    return dx0, dX, dW, du
