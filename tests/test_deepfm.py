"""DeepFM model-level tests on the CPU path: convergence, checkpoint round
trip, reduction to FM when the deep head is zero, and the CLI."""

import pytest
import torch

from lightctr_amd.data import LibffmDataset
from lightctr_amd.data.synthetic import SyntheticCriteo
from lightctr_amd.models.deepfm import (DeepFMHyper, DeepFMModel,
                                        DeepFMTrainer)
from lightctr_amd.models.fm import FMHyper, FMModel


def test_deepfm_cpu_convergence():
    """size and AUC floor of test_widedeep_cpu_convergence"""
    gen = SyntheticCriteo(num_features=1 << 13, seed=37)
    row_ptr, fields, fids, vals, labels = gen.batch(1024)
    ds = LibffmDataset(row_ptr, fields, fids, vals, labels)
    h = DeepFMHyper(num_features=1 << 13, num_fields=39, k=8,
                    hidden=(64, 32))
    tr = DeepFMTrainer(ds, h, device="cpu", batch_size=256, epochs=3)
    m0 = tr.evaluate()
    tr.train(log=None)
    m1 = tr.evaluate()
    assert m1["logloss"] < m0["logloss"]
    assert m1["auc"] > 0.55


def _state(m):
    out = {k: v.clone() for k, v in m.state_dict().items()
           if torch.is_tensor(v)}
    for name, la in m.mlp.state_dict().items():
        for k, v in la.items():
            out[f"{name}.{k}"] = v.clone()
    return out


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
def test_deepfm_checkpoint_roundtrip(tmp_path, opt):
    """checkpoint -> perturb -> load -> the next step is identical,
    optimizer state and MLP included"""
    F = 1 << 10
    gen = SyntheticCriteo(num_features=F, seed=5)
    h = DeepFMHyper(num_features=F, num_fields=39, k=4, hidden=(16,),
                    optimizer=opt, lr=0.1)
    a = DeepFMModel(h, device="cpu")
    batches = [gen.batch(64) for _ in range(3)]
    for rp, _, fi, v, lb in batches[:2]:
        a.train_step(rp, fi, v, lb)
    path = str(tmp_path / "deepfm.pt")
    a.save(path)
    rp, _, fi, v, lb = batches[2]
    loss_a = a.train_step(rp, fi, v, lb)

    b = DeepFMModel(h, device="cpu")
    for rp2, _, fi2, v2, lb2 in batches[:1]:   # perturb every tensor
        b.train_step(rp2, fi2, v2, lb2)
    b.W.add_(1.0)
    b.mlp.layers[0].W.add_(1.0)
    b.load(path)
    loss_b = b.train_step(rp, fi, v, lb)
    assert torch.equal(loss_a, loss_b)
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    if opt == "ftrl":
        assert "zW" in sa and "zE" in sa
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_deepfm_zero_head_equals_fm():
    """last MLP layer zero: the score is the FM score of the same W / V"""
    F, K = 1 << 10, 8
    gen = SyntheticCriteo(num_features=F, seed=11)
    rp, _, fi, v, _ = gen.batch(128)
    g = torch.Generator().manual_seed(2)
    dfm = DeepFMModel(DeepFMHyper(num_features=F, num_fields=39, k=K,
                                  hidden=(16,), init_sigma=0.1),
                      device="cpu")
    dfm.W.copy_(torch.randn(F, generator=g) * 0.1)
    dfm.mlp.layers[-1].W.zero_()
    dfm.mlp.layers[-1].b.zero_()
    fm = FMModel(FMHyper(num_features=F, k=K), device="cpu")
    fm.W.copy_(dfm.W)
    fm.V.copy_(dfm.E)
    p = dfm.predict_proba(rp, fi, v)
    q = fm.predict_proba(rp, fi, v)
    assert torch.allclose(p, q, atol=1e-6, rtol=0), (p - q).abs().max()
    assert float((p - 0.5).abs().max()) > 1e-3  # not a trivial batch


def test_deepfm_cli_roundtrip(tmp_path):
    """train --save -> predict --load --dump for --model deepfm"""
    from lightctr_amd.cli import main

    model_path = str(tmp_path / "deepfm.pt")
    dump_path = str(tmp_path / "deepfm.scores")
    rc = main(["train", "--model", "deepfm", "--data", "synthetic", "--rows",
               "256", "--features", "4096", "--k", "8", "--epochs", "1",
               "--batch", "128", "--device", "cpu", "--save", model_path])
    assert rc == 0
    rc = main(["predict", "--model", "deepfm", "--data", "synthetic",
               "--rows", "128", "--features", "4096", "--k", "8", "--device",
               "cpu", "--load", model_path, "--dump", dump_path])
    assert rc == 0
    with open(dump_path) as f:
        scores = [float(s) for s in f.read().split()]
    # probabilities, written with six decimals
    assert len(scores) == 128 and all(0.0 <= s <= 1.0 for s in scores)


def test_deepfm_empty_batch_cpu():
    m = DeepFMModel(DeepFMHyper(num_features=64, num_fields=3, k=4,
                                hidden=(8,)), device="cpu")
    rp = torch.zeros(1, dtype=torch.int32)
    fi = torch.zeros(0, dtype=torch.int32)
    v = torch.zeros(0)
    assert m.predict_proba(rp, fi, v).shape == (0,)
    assert m.train_step(rp, fi, v, torch.zeros(0)).shape == (0,)
