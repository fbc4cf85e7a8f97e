"""Pure-PyTorch reference for AutoInt's attention layers (CPU path and
baseline arm). x0 [B, nf*K] is the concat row, viewed as X^0 [B, nf, K];
W is a list of L matrices, W^1 [K, 4D] and W^l [D, 4D] with the columns
[Q | K | V | R], D = heads * head_dim; u [nf, D]:

  P   = X^{l-1} W^l
  S_h = Q_h K_h^T                      per head, unscaled
  A_h = softmax over keys (S_h)
  X^l = relu(concat_h(A_h V_h) + R)
  ai[b] = sum_{m,c} u[m,c] X^L[b,m,c]

with the backward written out (no autograd), in the dtype of its inputs. It
is what ops/csrc/autoint_kernels.hip computes, and with rounding="bf16" it
rounds where those kernels round and nowhere else: Q, K, V; A as the operand
of A V and of dV = A^T dY (the softmax and dS read it before the rounding);
X^l as saved; dY (the upstream gradient after the ReLU mask), dS, dQ, dK and
dV once each. ai reads X^L before its rounding, du the saved X^L.
"""

from __future__ import annotations

import torch


def _rounder(rounding):
    if rounding is None:
        return lambda t: t
    if rounding != "bf16":
        raise ValueError(f"unknown rounding {rounding!r}")
    return lambda t: t.bfloat16().to(t.dtype)


def _heads(t, heads):  # [B, nf, D] -> [B, heads, nf, hd]
    B, nf, D = t.shape
    return t.view(B, nf, heads, D // heads).transpose(1, 2)


def _attend(xp, w, heads, rd):
    """(Q, K, V as [B, heads, nf, hd], R [B, nf, D], A [B, heads, nf, nf])"""
    D = w.shape[1] // 4
    P = xp @ w
    q, k, v = (_heads(rd(P[..., i * D:(i + 1) * D]), heads) for i in range(3))
    A = torch.softmax(q @ k.transpose(2, 3), dim=-1)
    return q, k, v, P[..., 3 * D:], A


def autoint_forward_ref(x0, W, u, nf, heads, head_dim, rounding=None):
    """(ai [B], X [L, B, nf, D] = X^1 .. X^L)"""
    rd = _rounder(rounding)
    B, D = x0.shape[0], heads * head_dim
    xp, X, top = x0.view(B, nf, x0.shape[1] // nf), [], None
    for w in W:
        _, _, v, R, A = _attend(xp, w, heads, rd)
        top = torch.relu((rd(A) @ v).transpose(1, 2).reshape(B, nf, D) + R)
        xp = rd(top)
        X.append(xp)
    return (top * u).sum((1, 2)), torch.stack(X)


def autoint_backward_ref(x0, X, W, u, dpred, nf, heads, head_dim,
                         rounding=None):
    """(dx0 [B, nf*K], dW list like W, du [nf, D])"""
    rd = _rounder(rounding)
    B, D, L = x0.shape[0], heads * head_dim, len(W)
    du = torch.einsum("b,bmc->mc", dpred, X[L - 1])
    dX = dpred[:, None, None] * u
    dW = [None] * L
    for l in range(L - 1, -1, -1):
        xp = X[l - 1] if l else x0.view(B, nf, x0.shape[1] // nf)
        q, k, v, _, A = _attend(xp, W[l], heads, rd)
        dY = rd(dX * (X[l] > 0))
        dYh = _heads(dY, heads)
        dA = dYh @ v.transpose(2, 3)
        dS = rd(A * (dA - (A * dA).sum(-1, keepdim=True)))
        flat = lambda t: rd(t).transpose(1, 2).reshape(B, nf, D)
        G = torch.cat([flat(dS @ k), flat(dS.transpose(2, 3) @ q),
                       flat(rd(A).transpose(2, 3) @ dYh), dY], dim=-1)
        dW[l] = xp.flatten(0, 1).t() @ G.flatten(0, 1)
        dX = G @ W[l].t()
    return dX.reshape(B, x0.shape[1]), dW, du
