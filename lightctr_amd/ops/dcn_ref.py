"""Pure-PyTorch fp32 reference for the Deep & Cross cross term (CPU path and
baseline arm), x0 [B, d], Wc / bc [L, d], u [d]:

  x_{l+1} = x0 (x_l . w_l) + b_l + x_l      l = 0 .. L-1
  cross   = x_L . u

dcn_cross_* is the closed form of ops/csrc/dcn_kernels.hip: x_l = sigma_l x0
+ C_l, so the row needs only the L+1 dots P = x0 [Wc; u]^T and a scalar
recurrence, and no x_l is formed. dcn_layers_* is the definition, layer by
layer with its x_l kept for the backward (cross_impl="torch").
"""

from __future__ import annotations

import torch


def dcn_cross_prep_ref(Wc, bc, u):
    """(C [L+1, d], q [L+1]): C_0 = 0, C_{l+1} = C_l + b_l, q_l = C_l . w'_l
    with w' = [Wc; u]"""
    C = torch.cat([torch.zeros_like(bc[:1]), torch.cumsum(bc, 0)])
    return C, (C * torch.cat([Wc, u[None]])).sum(1)


def _sigmas(P, q):
    """sigma [B, L+1]: sigma_0 = 1, sigma_{l+1} = sigma_l + sigma_l p_l + q_l"""
    sig = [torch.ones_like(P[:, 0])]
    for l in range(P.shape[1] - 1):
        sig.append(sig[l] + (sig[l] * P[:, l] + q[l]))
    return torch.stack(sig, 1)


def dcn_cross_forward_ref(x0, Wc, u, q):
    """(cross [B], P [B, L+1])"""
    P = x0 @ torch.cat([Wc, u[None]]).t()
    sig = _sigmas(P, q)
    return sig[:, -1] * P[:, -1] + q[-1], P


def dcn_cross_backward_ref(x0, P, Wc, u, q, C, dpred):
    """(dx0 [B, d], dWc, dbc, du)"""
    L = Wc.shape[0]
    Wp = torch.cat([Wc, u[None]])
    sig = _sigmas(P, q)
    a, e = torch.empty_like(P), torch.empty_like(P)
    a[:, L], e[:, L] = dpred * sig[:, L], dpred
    dsig = dpred * P[:, L]
    for l in range(L - 1, -1, -1):
        a[:, l], e[:, l] = dsig * sig[:, l], dsig
        dsig = dsig * (1 + P[:, l])
    ebar = e.sum(0)
    dWp = a.t() @ x0 + ebar[:, None] * C
    # db_m = sum_{l > m} ebar_l w'_l
    dbc = torch.flip(torch.cumsum(torch.flip(ebar[1:, None] * Wp[1:], [0]),
                                  0), [0])
    return a @ Wp, dWp[:L], dbc, dWp[L]


def dcn_layers_forward(x0, Wc, bc, u):
    """(cross [B], [x_0 .. x_L]) by the definition"""
    xs = [x0]
    for l in range(Wc.shape[0]):
        s = xs[l] @ Wc[l]
        xs.append(x0 * s[:, None] + bc[l] + xs[l])
    return xs[-1] @ u, xs


def dcn_layers_backward(xs, Wc, u, dpred):
    """(dx0 [B, d], dWc, dbc, du) from the x_l of dcn_layers_forward"""
    x0 = xs[0]
    dx = dpred[:, None] * u
    du = dpred @ xs[-1]
    dx0 = torch.zeros_like(x0)
    dWc, dbc = torch.empty_like(Wc), torch.empty_like(Wc)
    for l in range(Wc.shape[0] - 1, -1, -1):
        ds = (dx * x0).sum(1)
        dx0 += dx * (xs[l] @ Wc[l])[:, None]
        dbc[l] = dx.sum(0)
        dWc[l] = ds @ xs[l]
        dx = dx + ds[:, None] * Wc[l]
    return dx0 + dx, dWc, dbc, du
