"""AutoInt on the CPU: ops/autoint_ref.py against the definition in float64
under autograd, and AutoIntModel's learning, checkpoint and CLI.
``attn_autograd`` and the case builders are also the reference of
test_autoint_kernels_gpu.py. A case's shape is (nf, K, heads, head_dim, L).

The field-pair test keeps xDeepFM's data, epochs, batch, k, hidden,
init_sigma and learning rates; the attention part is 2 layers of 2 heads of
16, the smallest served width, which passes the CPU run as it stands."""

import os

import pytest
import torch

from lightctr_amd.models.autoint import (AutoIntHyper, AutoIntModel,
                                         AutoIntTrainer)
from lightctr_amd.ops import autoint_ref
from test_xdeepfm import _pair_data

DATA = os.path.join(os.path.dirname(__file__), "..", "data")


def outs(L):
    return ("ai", "X", "dDeep", "du") + tuple(f"dW{l}" for l in range(L))


def attn_autograd(c, dtype=torch.float64):
    """P = X^{l-1} W^l = [Q | K | V | R], A_h = softmax(Q_h K_h^T),
    X^l = relu(concat_h(A_h V_h) + R), ai[b] = sum u X^L[b], layer by layer
    in `dtype`; its gradients by autograd with dpred as the upstream
    gradient. X is [L, B, nf, D]; dDeep is the incoming one plus dx0."""
    nf, H, L = c["nf"], c["heads"], len(c["W"])
    x0, u = (c[n].to(dtype).clone().requires_grad_() for n in ("x0", "u"))
    W = [w.to(dtype).clone().requires_grad_() for w in c["W"]]
    B, D = x0.shape[0], u.shape[1]
    xp, X = x0.view(B, nf, x0.shape[1] // nf), []
    for w in W:
        q, k, v, r = ((xp @ w[:, i * D:(i + 1) * D]) for i in range(4))
        hv = lambda t: t.view(B, nf, H, D // H).transpose(1, 2)
        A = torch.softmax(hv(q) @ hv(k).transpose(2, 3), dim=-1)
        xp = torch.relu((A @ hv(v)).transpose(1, 2).reshape(B, nf, D) + r)
        X.append(xp)
    ai = (xp * u).sum((1, 2))
    gr = torch.autograd.grad(ai, (x0, u, *W), c["dpred"].to(dtype))
    out = {"ai": ai.detach(), "X": torch.stack([t.detach() for t in X]),
           "dDeep": c["dDeep"].to(dtype) + gr[0], "du": gr[1]}
    out.update({f"dW{l}": gr[2 + l] for l in range(L)})
    return out


def float_case(B, nf, K, heads, hd, L, seed):
    """randn inputs, W and u scaled as at init; x0 and W hold bf16 values,
    which is what the kernels are given"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t: t.bfloat16().float()
    D = heads * hd
    return {"nf": nf, "heads": heads, "x0": bf(rn(B, nf * K)),
            "W": [bf(rn(din, 4 * D) * din ** -0.5)
                  for din in [K] + [D] * (L - 1)],
            "u": rn(nf, D) * (nf * D) ** -0.5, "dpred": rn(B),
            "dDeep": rn(B, nf * K)}


def ref_outputs(c, rounding=None):
    """ops/autoint_ref.py on a case, in the dtype of the case"""
    a = (c["nf"], c["heads"], c["u"].shape[1] // c["heads"], rounding)
    ai, X = autoint_ref.autoint_forward_ref(c["x0"], c["W"], c["u"], *a)
    dx0, dW, du = autoint_ref.autoint_backward_ref(
        c["x0"], X, c["W"], c["u"], c["dpred"], *a)
    out = {"ai": ai, "X": X, "dDeep": c["dDeep"] + dx0, "du": du}
    out.update({f"dW{l}": w for l, w in enumerate(dW)})
    return out


@pytest.mark.parametrize("nf,K,heads,hd,L", [(1, 5, 1, 16, 1),
                                             (7, 5, 2, 16, 2),
                                             (9, 4, 2, 32, 4)])
def test_ref_matches_definition(nf, K, heads, hd, L):
    c = float_case(5, nf, K, heads, hd, L, seed=100 * L + nf)
    c = {k: [w.double() for w in v] if k == "W" else
         v if k in ("nf", "heads") else v.double() for k, v in c.items()}
    ref, got = attn_autograd(c), ref_outputs(c)
    for name in outs(L):
        torch.testing.assert_close(got[name], ref[name], rtol=1e-10,
                                   atol=1e-10, msg=lambda m: f"{name}: {m}")
    with pytest.raises(ValueError, match="rounding"):
        ref_outputs(c, rounding="fp16")


def test_learns_a_field_pair_signal():
    from lightctr_amd.models.lr import LRHyper, LRTrainer

    ds, test = _pair_data(1024, 1), _pair_data(512, 2)
    h = AutoIntHyper(num_features=32, num_fields=4, k=4, hidden=(8,),
                     attn_layers=2, attn_heads=2, attn_dim=16,
                     init_sigma=0.3, mlp_lr=0.01, lr=0.1, l2=0.0)
    tr = AutoIntTrainer(ds, h, batch_size=64, epochs=12).train(log=None)
    wide = LRTrainer(ds, LRHyper(num_features=32), batch_size=64,
                     epochs=12).train(log=None)
    auc, base = tr.evaluate(test)["auc"], wide.evaluate(test)["auc"]
    assert base < 0.6 and auc > 0.9, (auc, base)


def test_checkpoint_layout_and_cli(tmp_path, capsys):
    from lightctr_amd import cli
    from lightctr_amd.data.libffm import load_libffm

    path = os.path.join(DATA, "train_sparse.csv")
    ds = load_libffm(path)
    h = AutoIntHyper(num_features=ds.num_features, num_fields=ds.num_fields,
                     k=4, attn_layers=2, attn_heads=1, attn_dim=16,
                     layout="field", pooling="mean")
    m = AutoIntModel(h)
    b = ds.slice_rows(0, 128)
    before = (m.Wa.clone(), m.ua.clone())
    for _ in range(2):
        m.train_step(b.row_ptr, b.fids, b.vals, b.labels, fields=b.fields)
    assert not torch.equal(before[0], m.Wa) and not torch.equal(before[1],
                                                                m.ua)
    m.save(tmp_path / "m.pt")
    d = torch.load(tmp_path / "m.pt", weights_only=True)
    assert d["attn_W0"].shape == (4, 64) and d["attn_W1"].shape == (16, 64)
    assert d["attn_u"].shape == (ds.num_fields, 16)
    assert torch.equal(d["attn_W1"], m.layers(m.Wa)[1])
    m2 = AutoIntModel(h)
    m2.load(str(tmp_path / "m.pt"))
    for n in ("Wa", "m_Wa", "v_Wa", "ua", "m_ua", "v_ua", "W", "E", "nE"):
        assert torch.equal(getattr(m, n), getattr(m2, n)), n
    assert m2.attn_step == m.attn_step == 2
    want = m.predict_proba(b.row_ptr, b.fids, b.vals, fields=b.fields)
    # predict takes depth, heads and head width from the checkpoint
    dump = tmp_path / "scores.txt"
    assert cli.main(["predict", "--model", "autoint", "--data", path, "--k",
                     "4", "--features", str(ds.num_features), "--load",
                     str(tmp_path / "m.pt"), "--device", "cpu",
                     "--attn-layers", "3", "--attn-heads", "2", "--dump",
                     str(dump)]) == 0
    scores = torch.tensor([float(s) for s in dump.read_text().split()])
    torch.testing.assert_close(scores[:128], want, rtol=0, atol=2e-6)
    assert cli.main(["train", "--model", "autoint", "--data", path, "--k",
                     "4", "--epochs", "1", "--device", "cpu", "--attn-dim",
                     "16", "--no-watchdog"]) == 0
    assert "auc" in capsys.readouterr().out
    for bad, fig in ((dict(attn_layers=5), "1..4, got 5"),
                     (dict(attn_heads=3), "1, 2 or 4, got 3"),
                     (dict(attn_dim=24), "16 or 32, got 24"),
                     (dict(attn_heads=4, attn_dim=32), "at most 64, got 128"),
                     (dict(num_fields=65), "1..64, got 65"),
                     (dict(num_fields=32, k=64), "1024, got 2048"),
                     (dict(k=128), "at most 64, got 128")):
        with pytest.raises(ValueError, match=fig):
            AutoIntModel(AutoIntHyper(**{**dict(num_features=8, num_fields=2,
                                                k=4), **bad}))
