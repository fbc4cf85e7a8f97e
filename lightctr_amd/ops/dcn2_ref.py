"""Pure-PyTorch reference for the DCN-v2 cross term (CPU path and baseline
arm), x0 [B, d], U / V [L, d, r], bc [L, d], u [d]:

  T_l     = x_l V_l
  z_l     = T_l U_l^T + b_l
  x_{l+1} = x0 * z_l + x_l          l = 0 .. L-1
  cross   = x_L . u

layer by layer in the dtype of its inputs, with the backward written out (no
autograd): it is what ops/csrc/dcn2_kernels.hip computes, and with
rounding="bf16" it rounds where those kernels round and nowhere else: T_l;
x_l as saved (X_l) and as operand of x_l V_l; G_l = g_{l+1} * x0 and
S_l = G_l U_l, as saved and as operands. dbc sums G_l before its rounding and
du reads the saved X_L, as the kernels do.
"""

from __future__ import annotations

import torch


def _rounder(rounding):
    if rounding is None:
        return lambda t: t
    if rounding != "bf16":
        raise ValueError(f"unknown rounding {rounding!r}")
    return lambda t: t.bfloat16().to(t.dtype)


def dcn2_cross_forward_ref(x0, U, V, bc, u, rounding=None):
    """(cross [B], X [L, B, d] = x_1 .. x_L, T [L, B, r])"""
    rd = _rounder(rounding)
    x, xb, X, T = x0, x0, [], []
    for l in range(U.shape[0]):
        T.append(rd(xb @ V[l]))
        x = x0 * (T[l] @ U[l].t() + bc[l]) + x
        xb = rd(x)
        X.append(xb)
    return x @ u, torch.stack(X), torch.stack(T)


def dcn2_cross_backward_ref(x0, X, T, U, V, bc, u, dpred, rounding=None):
    """(dx0 [B, d], G [L, B, d], S [L, B, r], dU, dV, dbc, du)"""
    rd = _rounder(rounding)
    L = U.shape[0]
    g = dpred[:, None] * u
    du = dpred @ X[L - 1]
    dx0 = torch.zeros_like(x0)
    G, S = [None] * L, [None] * L
    dU, dV, dbc = torch.empty_like(U), torch.empty_like(V), \
        torch.empty_like(bc)
    for l in range(L - 1, -1, -1):
        Gf = g * x0
        G[l] = rd(Gf)
        dbc[l] = Gf.sum(0)
        dx0 = dx0 + g * (T[l] @ U[l].t() + bc[l])
        S[l] = rd(G[l] @ U[l])
        dU[l] = G[l].t() @ T[l]
        dV[l] = (X[l - 1] if l else x0).t() @ S[l]
        g = g + S[l] @ V[l].t()
    return dx0 + g, torch.stack(G), torch.stack(S), dU, dV, dbc, du
