"""PNN on the CPU: ops/pnn_ref.py against the float64 definition under autograd
(``pnn_autograd``, with the case builders also test_pnn_kernels_gpu.py's
reference), PNNModel's learning, checkpoint, errors and CLI. Shape: (nf, K)."""

import os

import pytest
import torch

import kernel_oracles as ko
from lightctr_amd.models.pnn import PNNHyper, PNNModel
from lightctr_amd.ops import pnn_ref

DATA = os.path.join(os.path.dirname(__file__), "..", "data")
SHAPES = [(2, 4), (16, 16), (17, 16), (33, 8), (6, 64), (5, 32), (39, 16),
          (64, 16)]


def pair_index(i, j, nf):
    return i * (2 * nf - i - 1) // 2 + (j - i - 1)


def pnn_autograd(x0, dz, nf):
    """(z, dDeep) in float64: g[p(i,j)] = e_i . e_j pair by pair, z = [x0, g,
    0 .. 0], and dDeep the gradient of sum(z * dz) by autograd"""
    x = x0.double().clone().requires_grad_()
    B, d = x.shape
    e = x.view(B, nf, d // nf)
    P, Dz = nf * (nf - 1) // 2, (d + nf * (nf - 1) // 2 + 7) // 8 * 8
    g = [None] * P
    for i in range(nf):
        for j in range(i + 1, nf):
            g[pair_index(i, j, nf)] = (e[:, i] * e[:, j]).sum(1)
    z = torch.cat([x, torch.stack(g, 1), x.new_zeros(B, Dz - d - P)], 1)
    dDeep, = torch.autograd.grad(z, x, dz.double())
    return z.detach(), dDeep


def exact_case(B, nf, K, seed):
    """e and dz from {-1, 0, 1}: every sum is exact in bf16 / fp32"""
    g = torch.Generator().manual_seed(seed)
    draw = lambda *s: torch.randint(-1, 2, s, generator=g).float()
    return draw(B, nf * K), draw(B, pnn_ref.pnn_dims(nf, K)[1])


def float_case(B, nf, K, seed):
    """randn scaled as the embeddings at init, x0 holding bf16 values"""
    g = torch.Generator().manual_seed(seed)
    x0 = (torch.randn(B, nf * K, generator=g) * 0.01).bfloat16().float()
    return x0, torch.randn(B, pnn_ref.pnn_dims(nf, K)[1], generator=g)


def ref_outputs(x0, dz, nf, rounding=None):
    """ops/pnn_ref.py on a case, two rows at a time"""
    z = pnn_ref.pnn_forward_ref(x0, nf, rounding, 2)
    return z, pnn_ref.pnn_backward_ref(z, dz, nf, x0.shape[1] // nf, rounding,
                                       2)


@pytest.mark.parametrize("nf,K", SHAPES)
def test_ref_matches_definition(nf, K):
    """fp32 against float64 on the exact set, where no sum rounds: bit-equal,
    the pad +0; the bf16 rounding points then change nothing either"""
    x0, dz = exact_case(5, nf, K, seed=10 * nf + K)
    z64, dD64 = pnn_autograd(x0, dz, nf)
    assert z64.shape[1] == pnn_ref.pnn_dims(nf, K)[1]
    assert not z64[:, nf * K + nf * (nf - 1) // 2:].signbit().any()
    for rounding in (None, "bf16"):
        z, dDeep = ref_outputs(x0, dz, nf, rounding)
        ko.check_bits("z", z, z64.float())
        ko.check_bits("dDeep", dDeep, dD64.float())
    with pytest.raises(ValueError, match="rounding"):
        ref_outputs(x0, dz, nf, rounding="fp16")


def test_pair_order_is_triu_indices():
    for nf in (2, 5, 39, 64):
        i, j = torch.triu_indices(nf, nf, 1)
        p = [pair_index(a, b, nf) for a, b in zip(i.tolist(), j.tolist())]
        assert p == list(range(nf * (nf - 1) // 2))


@pytest.mark.parametrize("layout", ("position", "field"))
def test_model_learns_and_round_trips(tmp_path, layout):
    from lightctr_amd.data.synthetic import SyntheticMultiHot

    h = PNNHyper(num_features=256, num_fields=5, k=4, hidden=(8,),
                 layout=layout, pooling="mean", init_sigma=0.3, mlp_lr=0.01,
                 lr=0.1, mlp_optimizer="adam")
    m = PNNModel(h)
    assert m.mlp.layers[0].W.shape == (8, 32)  # Dz = 20 + 10, up to 32
    gen = SyntheticMultiHot(num_features=256, num_fields=5, multi=(1, 3),
                            max_multi=3, seed=2)
    row_ptr, fields, fids, vals, labels = gen.batch(128)
    loss = [float(m.train_step(row_ptr, fids, vals, labels,
                               fields=fields).mean()) for _ in range(3)]
    assert loss[2] < loss[1] < loss[0], loss
    m.save(tmp_path / "m.pt")
    assert sorted(torch.load(tmp_path / "m.pt", weights_only=True)) == [
        "E", "W", "hyper", "mlp", "nE", "nW"]  # Wide&Deep's checkpoint
    m2 = PNNModel(h)
    m2.load(str(tmp_path / "m.pt"))
    assert torch.equal(
        m.predict_proba(row_ptr, fids, vals, fields=fields),
        m2.predict_proba(row_ptr, fids, vals, fields=fields))


@pytest.mark.parametrize("bad,fig", [
    (dict(num_fields=1), "2..64, got 1"),
    (dict(num_fields=65), "2..64, got 65"),
    (dict(k=5), "4, 8, 16, 32 or 64, got 5"),
    (dict(num_fields=32, k=64), "1024, got 2048")])
def test_constructor_errors(bad, fig):
    with pytest.raises(ValueError, match=fig):
        PNNModel(PNNHyper(**{**dict(num_features=8, num_fields=2, k=4),
                             **bad}))
    with pytest.raises(ValueError, match="pnn_impl"):
        PNNModel(PNNHyper(num_features=8, num_fields=2, k=4), pnn_impl="x")


def test_cli_round_trip(tmp_path, capsys):
    from lightctr_amd import cli

    path, ckpt = os.path.join(DATA, "train_sparse.csv"), tmp_path / "m.pt"
    assert cli.main(["train", "--model", "pnn", "--data", path, "--k", "4",
                     "--epochs", "1", "--device", "cpu", "--save", str(ckpt),
                     "--no-watchdog"]) == 0
    assert "auc" in capsys.readouterr().out
    d = torch.load(ckpt, weights_only=True)
    nf = d["hyper"]["num_fields"]
    assert d["mlp"]["layer0"]["W"].shape[1] == pnn_ref.pnn_dims(nf, 4)[1]
    dump = tmp_path / "scores.txt"
    assert cli.main(["predict", "--model", "pnn", "--data", path, "--k", "4",
                     "--load", str(ckpt), "--device", "cpu", "--dump",
                     str(dump)]) == 0
    scores = dump.read_text().split()
    assert scores and all(0.0 < float(s) < 1.0 for s in scores)
