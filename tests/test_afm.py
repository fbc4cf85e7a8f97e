"""AFM on the CPU: ops/afm_ref.py against the definition in float64 under
autograd, and AFMModel's learning, checkpoint, argument errors and CLI.
``afm_autograd`` and the case builders are also the reference of
test_afm_kernels_gpu.py. A case's shape is (nf, K, A)."""

import os

import pytest
import torch

from lightctr_amd.models.afm import AFMHyper, AFMModel
from lightctr_amd.ops import afm_ref

DATA = os.path.join(os.path.dirname(__file__), "..", "data")
NAMES = ("afm", "dDeep", "dWa", "dba", "dqa", "dua")
PARAMS = ("Wa", "ba", "qa", "ua")


def afm_autograd(c, dtype=torch.float64):
    """p_ij = e_i e_j (i < j), s = qa . relu(Wa^T p + ba), a = softmax over
    the pairs, afm = ua . sum a p in `dtype`; its gradients by autograd with
    dpred as the upstream gradient. dDeep is the incoming one plus dx0."""
    nf = c["nf"]
    x0, Wa, ba, qa, ua = (c[n].to(dtype).clone().requires_grad_()
                          for n in ("x0",) + PARAMS)
    e = x0.view(x0.shape[0], nf, x0.shape[1] // nf)
    i, j = torch.triu_indices(nf, nf, 1)
    p = e[:, i] * e[:, j]
    a = torch.softmax(torch.relu(p @ Wa + ba) @ qa, dim=1)
    afm = (a[:, :, None] * p).sum(1) @ ua
    gr = torch.autograd.grad(afm, (x0, Wa, ba, qa, ua), c["dpred"].to(dtype))
    return {"afm": afm.detach(), "dDeep": c["dDeep"].to(dtype) + gr[0],
            "dWa": gr[1], "dba": gr[2], "dqa": gr[3], "dua": gr[4]}


def float_case(B, nf, K, A, seed):
    """randn inputs, the parameters scaled as at init but ba (randn * 0.1);
    x0 and Wa hold bf16 values, which is what the kernels are given"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t: t.bfloat16().float()
    return {"nf": nf, "x0": bf(rn(B, nf * K)), "Wa": bf(rn(K, A) * K ** -0.5),
            "ba": rn(A) * 0.1, "qa": rn(A) * A ** -0.5,
            "ua": rn(K) * K ** -0.5, "dpred": rn(B), "dDeep": rn(B, nf * K)}


def ref_outputs(c, rounding=None):
    """ops/afm_ref.py on a case, in the dtype of the case"""
    w = tuple(c[n] for n in PARAMS)
    afm, lse = afm_ref.afm_forward_ref(c["x0"], *w, c["nf"], rounding, 2)
    dx0, *gr = afm_ref.afm_backward_ref(c["x0"], lse, afm, *w, c["dpred"],
                                        c["nf"], rounding, 2)
    return dict(zip(NAMES, (afm, c["dDeep"] + dx0, *gr)))


@pytest.mark.parametrize("nf,K,A", [(2, 5, 16), (7, 4, 32)])
def test_ref_matches_definition(nf, K, A):
    c = float_case(5, nf, K, A, seed=10 * nf + K)
    c = {k: v if k == "nf" else v.double() for k, v in c.items()}
    ref, got = afm_autograd(c), ref_outputs(c)
    for name in NAMES:
        torch.testing.assert_close(got[name], ref[name], rtol=1e-10,
                                   atol=1e-10, msg=lambda m: f"{name}: {m}")
    with pytest.raises(ValueError, match="rounding"):
        ref_outputs(c, rounding="fp16")


def test_model_learns_and_round_trips(tmp_path):
    from lightctr_amd.data.synthetic import SyntheticMultiHot

    h = AFMHyper(num_features=256, num_fields=5, k=4, hidden=(8,),
                 attn_factor=16, layout="field", pooling="mean",
                 init_sigma=0.3, mlp_lr=0.01, lr=0.1, mlp_optimizer="adam")
    m = AFMModel(h)
    gen = SyntheticMultiHot(num_features=256, num_fields=5, multi=(1, 3),
                            max_multi=3, seed=2)
    row_ptr, fields, fids, vals, labels = gen.batch(128)
    before = {n: getattr(m, n).clone() for n in PARAMS}
    loss = [float(m.train_step(row_ptr, fids, vals, labels,
                               fields=fields).mean()) for _ in range(3)]
    assert loss[2] < loss[1] < loss[0], loss
    for n in PARAMS:
        assert not torch.equal(before[n], getattr(m, n)), n
    m.save(tmp_path / "m.pt")
    d = torch.load(tmp_path / "m.pt", weights_only=True)
    assert d["afm_W"].shape == (4, 16) and d["afm_v_q"].shape == (16,)
    m2 = AFMModel(h)
    m2.load(str(tmp_path / "m.pt"))
    for n in PARAMS:
        for s in ("", "m_", "v_"):
            assert torch.equal(getattr(m, s + n), getattr(m2, s + n)), s + n
    assert m2.afm_step == m.afm_step == 3
    assert torch.equal(
        m.predict_proba(row_ptr, fids, vals, fields=fields),
        m2.predict_proba(row_ptr, fids, vals, fields=fields))


@pytest.mark.parametrize("bad,fig", [
    (dict(attn_factor=24), "16..64, got 24"),
    (dict(attn_factor=80), "16..64, got 80"),
    (dict(num_fields=1), "2..64, got 1"),
    (dict(num_fields=65), "2..64, got 65"),
    (dict(num_fields=32, k=64), "1024, got 2048"),
    (dict(k=128), "at most 64, got 128")])
def test_constructor_errors(bad, fig):
    with pytest.raises(ValueError, match=fig):
        AFMModel(AFMHyper(**{**dict(num_features=8, num_fields=2, k=4),
                             **bad}))
    with pytest.raises(ValueError, match="afm_impl"):
        AFMModel(AFMHyper(num_features=8, num_fields=2, k=4), afm_impl="x")


def test_cli_round_trip(tmp_path, capsys):
    from lightctr_amd import cli

    path, ckpt = os.path.join(DATA, "train_sparse.csv"), tmp_path / "m.pt"
    assert cli.main(["train", "--model", "afm", "--data", path, "--k", "4",
                     "--epochs", "1", "--device", "cpu", "--attn-factor",
                     "16", "--save", str(ckpt), "--no-watchdog"]) == 0
    assert "auc" in capsys.readouterr().out
    assert torch.load(ckpt, weights_only=True)["afm_W"].shape == (4, 16)
    # predict takes the attention width from the checkpoint
    dump = tmp_path / "scores.txt"
    assert cli.main(["predict", "--model", "afm", "--data", path, "--k", "4",
                     "--load", str(ckpt), "--device", "cpu", "--attn-factor",
                     "48", "--dump", str(dump)]) == 0
    scores = [float(s) for s in dump.read_text().split()]
    assert scores and all(0.0 < s < 1.0 for s in scores)
