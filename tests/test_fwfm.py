"""Field-weighted FM on the CPU: ops/fwfm_ref.py (per-field sums) against
the entry-pair form in float64 and against autograd, the R == 1 => FM
identity, checkpoints, the construction-time LDS rule, the bundled data and
the CLI. ``pair_ref`` is also the reference of test_fwfm_kernels_gpu.py."""

import os

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel, FMTrainer
from lightctr_amd.models.fwfm import FwFMHyper, FwFMModel, FwFMTrainer
from lightctr_amd.ops import fwfm_ref

F64 = torch.float64
DATA = os.path.join(os.path.dirname(__file__), "..", "data")


def pair_ref(row_ptr, fields, fids, vals, W, V, R, dpred):
    """float64 over the entry pairs i != j of every row, deliberately not
    the per-field sums. Per output a [3, ...] stack: the value, the sum of
    the absolute values of its terms, and the number of terms."""
    B, nf, K = row_ptr.numel() - 1, R.shape[0], V.shape[1]
    W, V, R, vals, dpred = (t.double() for t in (W, V, R, vals, dpred))
    nnz = fids.numel()
    out = {"pred": torch.zeros(3, B, dtype=F64),
           "gw": torch.zeros(3, nnz, dtype=F64),
           "gv": torch.zeros(3, nnz, K, dtype=F64),
           "dR": torch.zeros(3, nf * nf, dtype=F64)}
    for r in range(B):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        n = hi - lo
        if n == 0:
            continue
        a, f, x, d = fields[lo:hi].long(), fids[lo:hi].long(), vals[lo:hi], \
            dpred[r]
        ok = (a >= 0) & (a < nf)
        a = a.clamp(0, nf - 1)
        cell = torch.minimum(a[:, None], a[None, :]) * nf + \
            torch.maximum(a[:, None], a[None, :])
        live = (ok[:, None] & ok[None, :] & ~torch.eye(n, dtype=torch.bool))
        wt = R.view(-1)[cell] * live             # [n, n], 0 on i == j
        vx = V[f] * x[:, None]
        up = live & torch.ones(n, n).triu(1).bool()   # i < j
        prod = vx[:, None, :] * vx[None, :, :]        # [n, n, K]
        lin, pt = W[f] * x, (wt * up)[:, :, None] * prod
        out["pred"][:, r] = torch.stack([
            lin.sum() + pt.sum() + 0.0, lin.abs().sum() + pt.abs().sum(),
            n + up.sum() * K])
        dx = d * x
        out["gw"][:, lo:hi] = torch.stack([dx, dx.abs(), torch.ones(n)])
        g = torch.einsum("ij,ik->jk", wt, vx) + 0.0
        gv = torch.where(ok[:, None], dx[:, None] * g, torch.zeros(1, dtype=F64))
        out["gv"][:, lo:hi] = torch.stack([
            gv, dx.abs()[:, None] * torch.einsum("ij,ik->jk", wt.abs(),
                                                 vx.abs()),
            live.sum(0)[:, None].expand(n, K).double()])
        for i, t in enumerate((d * prod.sum(-1), (d * prod).abs().sum(-1),
                               torch.full((n, n), float(K), dtype=F64))):
            out["dR"][i].index_add_(0, cell[up], t[up])
    out["dR"] = out["dR"].view(3, nf, nf)
    return out


def random_batch(B, nf, K, F=512, seed=0, lo=1, hi=12):
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(lo, hi + 1, (B,), generator=g)
    row_ptr = torch.zeros(B + 1, dtype=torch.int32)
    row_ptr[1:] = n.cumsum(0)
    nnz = int(n.sum())
    return {"row_ptr": row_ptr,
            "fields": torch.randint(0, nf, (nnz,), generator=g,
                                    dtype=torch.int32),
            "fids": torch.randint(0, F, (nnz,), generator=g,
                                  dtype=torch.int32),
            "vals": torch.rand(nnz, generator=g) + 0.5,
            "W": torch.randn(F, generator=g), "V": torch.randn(F, K, generator=g),
            "R": torch.randn(nf, nf, generator=g),
            "dpred": torch.randn(B, generator=g),
            "labels": torch.randint(0, 2, (B,), generator=g).float()}


def csr(c):
    return c["row_ptr"], c["fields"], c["fids"], c["vals"]


@pytest.mark.parametrize("nf,K", [(1, 4), (5, 8), (39, 16)])
def test_ref_matches_pairs_and_autograd(nf, K):
    c = random_batch(7, nf, K, seed=nf)
    c["fields"][0], c["fields"][-1] = nf, -1      # wide term only
    d = {k: (v.double() if v.is_floating_point() else v)
         for k, v in c.items()}
    V, R = d["V"].requires_grad_(), d["R"].requires_grad_()
    ref = pair_ref(*csr(c), c["W"], c["V"], c["R"], c["dpred"])
    pred = fwfm_ref.fwfm_forward_ref(*csr(d), d["W"], V, R)
    torch.testing.assert_close(pred.detach(), ref["pred"][0], rtol=1e-12,
                               atol=1e-12)
    gw, gv, dR = fwfm_ref.fwfm_backward_emit_ref(*csr(d), V.detach(),
                                                 R.detach(), d["dpred"])
    (pred * d["dpred"]).sum().backward()
    gV = torch.zeros_like(V).index_add_(0, d["fids"].long(), gv)
    for got, want in ((gV, V.grad), (dR, R.grad), (dR, ref["dR"][0]),
                      (gv, ref["gv"][0]), (gw, ref["gw"][0])):
        torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    assert not dR.tril(-1).any()


def test_r_one_is_fm_and_checkpoint_roundtrip(tmp_path):
    c = random_batch(16, 5, 8, seed=3)
    m = FwFMModel(FwFMHyper(num_features=512, num_fields=5, k=8, r_lr=0.0))
    fm = FMModel(FMHyper(num_features=512, k=8))
    for _ in range(2):
        m.train_step(*csr(c), c["labels"])
    assert torch.equal(m.R, torch.ones(5, 5))     # r_lr = 0: R stays 1
    fm.W.copy_(m.W), fm.V.copy_(m.V)
    torch.testing.assert_close(m.predict_proba(*csr(c)),
                               fm.predict_proba(c["row_ptr"], c["fids"],
                                                c["vals"]))
    m = FwFMModel(FwFMHyper(num_features=512, num_fields=5, k=8,
                            optimizer="ftrl"))
    m.train_step(*csr(c), c["labels"])
    assert m.nR.triu().any() and (m.R != 1).any()  # R trains, but not
    assert torch.equal(m.R.tril(-1), torch.ones(5, 5).tril(-1))  # below
    m.save(tmp_path / "m.pt")
    m2 = FwFMModel(FwFMHyper(num_features=512, num_fields=5, k=8,
                             optimizer="ftrl"))
    m2.load(str(tmp_path / "m.pt"))
    for name in ("W", "V", "R", "nW", "nV", "nR", "zW", "zV"):
        assert torch.equal(getattr(m, name), getattr(m2, name)), name


def test_lds_rule_refuses_on_gpu_only():
    h = FwFMHyper(num_features=64, num_fields=64, k=64)
    FwFMModel(h, device="cpu")                     # the CPU path has no limit
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="bytes of LDS"):
            FwFMModel(h, device="cuda:0")


def test_bundled_data_auc_and_cli(tmp_path, capsys):
    from lightctr_amd.cli import main
    from lightctr_amd.data.libffm import load_libffm

    tr = load_libffm(os.path.join(DATA, "train_sparse.csv"))
    te = load_libffm(os.path.join(DATA, "test_sparse.csv"))
    F = max(tr.num_features, te.num_features)
    kw = dict(num_features=F, k=8, lr=0.3)
    a_fm = FMTrainer(tr, FMHyper(**kw), batch_size=128,
                     epochs=8).train(log=None).evaluate(te)["auc"]
    a_fw = FwFMTrainer(tr, FwFMHyper(num_fields=tr.num_fields, **kw),
                       batch_size=128, epochs=8).train(log=None) \
        .evaluate(te)["auc"]
    print(f"AUC fm {a_fm:.4f} fwfm {a_fw:.4f}")
    assert a_fw >= a_fm - 0.01, (a_fw, a_fm)
    common = ["--model", "fwfm", "--k", "8", "--device", "cpu", "--batch",
              "128", "--no-watchdog"]
    path = str(tmp_path / "fw.pt")
    assert main(["train", "--data", os.path.join(DATA, "train_sparse.csv"),
                 "--epochs", "2", "--save", path] + common) == 0
    assert main(["predict", "--data", os.path.join(DATA, "test_sparse.csv"),
                 "--load", path] + common) == 0
    assert '"auc"' in capsys.readouterr().out
