"""xDeepFM on the CPU: ops/cin_ref.py against the definition in float64 under
autograd, and XDeepFMModel's learning, checkpoint and CLI. ``cin_autograd``
and the case builders are also the reference of test_cin_kernels_gpu.py."""

import os

import pytest
import torch

from lightctr_amd.models.xdeepfm import (XDeepFMHyper, XDeepFMModel,
                                         XDeepFMTrainer)
from lightctr_amd.ops import cin_ref

DATA = os.path.join(os.path.dirname(__file__), "..", "data")


def outs(L):
    return ("cin", "X", "dX", "dDeep", "du") + tuple(
        f"dW{l}" for l in range(L))


def cin_autograd(c, dtype=torch.float64):
    """The definition X^l[b,h,d] = sum_ij W^l[h,i,j] X^{l-1}[b,i,d] x0[b,j,d],
    cin[b] = sum_l sum_h u[l,h] sum_d X^l[b,h,d], layer by layer in `dtype`;
    its gradients by autograd with dpred as the upstream gradient. X and dX
    in row form [L, B, K, H]; dDeep is the incoming one plus dx0."""
    nf, L = c["nf"], len(c["W"])
    x0, u = (c[n].to(dtype).clone().requires_grad_() for n in ("x0", "u"))
    W = [w.to(dtype).clone().requires_grad_() for w in c["W"]]
    B = x0.shape[0]
    xr = x0.view(B, nf, x0.shape[1] // nf)
    xp, X, cin = xr, [], 0.0
    for l in range(L):
        Z = (xp[:, :, None, :] * xr[:, None, :, :]).flatten(1, 2)
        X.append(torch.einsum("hn,bnd->bhd", W[l].flatten(1), Z))
        cin = cin + torch.einsum("h,bhd->b", u[l], X[l])
        xp = X[l]
    gr = torch.autograd.grad(cin, (x0, u, *W, *X), c["dpred"].to(dtype))
    rows = lambda ts: torch.stack([t.detach().transpose(1, 2) for t in ts])
    out = {"cin": cin.detach(), "X": rows(X), "dX": rows(gr[2 + L:]),
           "dDeep": c["dDeep"].to(dtype) + gr[0], "du": gr[1]}
    out.update({f"dW{l}": gr[2 + l] for l in range(L)})
    return out


def float_case(B, nf, K, H, L, seed):
    """randn inputs, W and u scaled as at init; x0 and W hold bf16 values,
    which is what the kernels are given"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t: t.bfloat16().float()
    hp = lambda l: nf if l == 0 else H
    return {"nf": nf, "x0": bf(rn(B, nf * K)),
            "W": [bf(rn(H, hp(l), nf) * (hp(l) * nf) ** -0.5)
                  for l in range(L)],
            "u": rn(L, H) * H ** -0.5, "dpred": rn(B), "dDeep": rn(B, nf * K)}


def ref_outputs(c, rounding=None):
    """ops/cin_ref.py on a case, in the dtype of the case"""
    cin, X = cin_ref.cin_forward_ref(c["x0"], c["W"], c["u"], c["nf"],
                                     rounding, chunk=2)
    dx0, dX, dW, du = cin_ref.cin_backward_ref(
        c["x0"], X, c["W"], c["u"], c["dpred"], c["nf"], rounding, chunk=2)
    out = {"cin": cin, "X": X, "dX": dX, "dDeep": c["dDeep"] + dx0, "du": du}
    out.update({f"dW{l}": w for l, w in enumerate(dW)})
    return out


@pytest.mark.parametrize("nf,K,H,L", [(1, 5, 16, 1), (7, 1, 16, 2),
                                      (9, 4, 32, 4)])
def test_ref_matches_definition(nf, K, H, L):
    c = float_case(5, nf, K, H, L, seed=100 * L + nf)
    c = {k: [w.double() for w in v] if k == "W" else
         v if k == "nf" else v.double() for k, v in c.items()}
    ref, got = cin_autograd(c), ref_outputs(c)
    for name in outs(L):
        torch.testing.assert_close(got[name], ref[name], rtol=1e-10,
                                   atol=1e-10, msg=lambda m: f"{name}: {m}")
    with pytest.raises(ValueError, match="rounding"):
        ref_outputs(c, rounding="fp16")
    idx, cols = cin_ref.cin_order(nf, H)  # distinct columns, pads left over
    assert idx.unique().numel() == nf * H and int(idx.max()) < cols


def _pair_data(n, seed):
    """4 fields of 8 values each; the label is the parity of the first two
    fields' values: nothing for a model that is linear in the one-hots"""
    from lightctr_amd.data import LibffmDataset

    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, 8, (n, 4), generator=g)
    fids = (v + 8 * torch.arange(4)).flatten().int()
    labels = ((v[:, 0] + v[:, 1]) % 2).float()
    return LibffmDataset(torch.arange(0, 4 * n + 1, 4, dtype=torch.int32),
                         torch.arange(4).repeat(n).int(), fids,
                         torch.ones(4 * n), labels)


def test_learns_a_field_pair_signal():
    from lightctr_amd.models.lr import LRHyper, LRTrainer

    ds, test = _pair_data(1024, 1), _pair_data(512, 2)
    h = XDeepFMHyper(num_features=32, num_fields=4, k=4, hidden=(8,),
                     cin_layers=2, cin_maps=16, init_sigma=0.3, mlp_lr=0.01,
                     lr=0.1, l2=0.0)
    tr = XDeepFMTrainer(ds, h, batch_size=64, epochs=12).train(log=None)
    wide = LRTrainer(ds, LRHyper(num_features=32), batch_size=64,
                     epochs=12).train(log=None)
    auc, base = tr.evaluate(test)["auc"], wide.evaluate(test)["auc"]
    assert base < 0.6 and auc > 0.9, (auc, base)
    idx, cols = cin_ref.cin_order(4, 4)  # 16 of layer 1's 32 columns are pads
    pad = torch.ones(cols, dtype=torch.bool)
    pad[idx.flatten()] = False
    wk = tr.model._layer(tr.model.Wk, 0)
    assert pad.sum() == 16 and not wk[:, pad].any() and wk[:, ~pad].all()


def test_checkpoint_layout_and_cli(tmp_path, capsys):
    from lightctr_amd import cli
    from lightctr_amd.data.libffm import load_libffm

    path = os.path.join(DATA, "train_sparse.csv")
    ds = load_libffm(path)
    h = XDeepFMHyper(num_features=ds.num_features, num_fields=ds.num_fields,
                     k=4, cin_layers=2, cin_maps=16, layout="field",
                     pooling="mean")
    m = XDeepFMModel(h)
    b = ds.slice_rows(0, 128)
    before = (m.Wk.clone(), m.u.clone())
    for _ in range(2):
        m.train_step(b.row_ptr, b.fids, b.vals, b.labels, fields=b.fields)
    assert not torch.equal(before[0], m.Wk) and not torch.equal(before[1],
                                                                m.u)
    m.save(tmp_path / "m.pt")
    d = torch.load(tmp_path / "m.pt", weights_only=True)
    nf = ds.num_fields
    assert d["cin_W0"].shape == (16, nf, nf) and d["cin_W1"].shape == (
        16, 16, nf)
    idx, cols = cin_ref.cin_order(nf, 16)  # canonical <-> kernel order
    wk = m._layer(m.Wk, 1)
    assert torch.equal(wk[:, idx[3, 2]], d["cin_W1"][:, 3, 2])
    m2 = XDeepFMModel(h)
    m2.load(str(tmp_path / "m.pt"))
    for n in ("Wk", "m_Wk", "v_Wk", "u", "m_u", "v_u", "W", "E", "nE"):
        assert torch.equal(getattr(m, n), getattr(m2, n)), n
    assert m2.cin_step == m.cin_step == 2
    want = m.predict_proba(b.row_ptr, b.fids, b.vals, fields=b.fields)
    # predict takes depth 2 and 16 maps from the checkpoint, not the flags
    dump = tmp_path / "scores.txt"
    assert cli.main(["predict", "--model", "xdeepfm", "--data", path, "--k",
                     "4", "--features", str(ds.num_features), "--load",
                     str(tmp_path / "m.pt"), "--device", "cpu",
                     "--cin-layers", "3", "--cin-maps", "32", "--dump",
                     str(dump)]) == 0
    scores = torch.tensor([float(s) for s in dump.read_text().split()])
    torch.testing.assert_close(scores[:128], want, rtol=0, atol=2e-6)
    assert cli.main(["train", "--model", "xdeepfm", "--data", path, "--k",
                     "4", "--epochs", "1", "--device", "cpu", "--cin-maps",
                     "16", "--no-watchdog"]) == 0
    assert "auc" in capsys.readouterr().out
    for bad, fig in ((dict(cin_layers=5), "1..4, got 5"),
                     (dict(cin_maps=24), "16..128, got 24"),
                     (dict(num_fields=65), "1..64, got 65"),
                     (dict(num_fields=64, k=32), "1024, got 2048")):
        with pytest.raises(ValueError, match=fig):
            XDeepFMModel(XDeepFMHyper(**{**dict(num_features=8, num_fields=2,
                                                k=4), **bad}))
