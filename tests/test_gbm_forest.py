"""CompiledForest (CPU path), GBDT+LR stacking and the dense serving CLI.

Margin oracle: the unchanged GBMModel.predict_margin, compared with
torch.equal (the compiled walk sums leaf values in the same tree order).
Leaf oracle: gbm_forest_util.leaf_oracle, a copy of GBMModel._route.
"""

import json
import os
import subprocess
import sys

import pytest
import torch

from gbm_forest_util import (leaf_oracle, make_model, make_X,
                             put_edge_values, random_tree, stacking_data,
                             tree_with_nodes)
from lightctr_amd.models import GBDTLRHyper, GBDTLRModel
from lightctr_amd.models.gbm import GBMHyper, GBMModel
from lightctr_amd.predict import BatchPredictor, CompiledForest
from lightctr_amd.utils.metrics import auc_score

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _forest(seed, N, D, n_trees, depth, K=1, special=False, n_bins=255):
    g = torch.Generator().manual_seed(seed)
    X = make_X(g, N, D, special=special)
    trees = [random_tree(g, D, depth) for _ in range(n_trees)]
    m = make_model(trees, X if N else torch.randn(8, D, generator=g), K=K,
                   n_bins=n_bins, max_depth=depth)
    if special and N:
        X = put_edge_values(g, X, m.bin_edges)
    return m, X


def _check_all(m, X):
    cf = m.compile()
    assert torch.equal(cf.predict_margin(X), m.predict_margin(X))
    assert torch.equal(cf.predict_proba(X), m.predict_proba(X))
    leaf = cf.predict_leaf(X)
    assert leaf.dtype == torch.int32
    assert torch.equal(leaf, leaf_oracle(m, X))
    return cf


@pytest.mark.parametrize("K", [1, 3])
def test_margin_proba_leaf_equal(K):
    m, X = _forest(0, 301, 5, 4 * K, 4, K=K)
    cf = _check_all(m, X)
    assert cf.n_trees == 4 * K and cf.n_classes == K
    assert cf.max_depth <= 4
    assert cf.n_leaves == sum(int((t.feature < 0).sum())
                              for rt in m.trees for t in rt)
    assert cf.predict_margin(X).shape == (301, K)


def test_transform_csr():
    m, X = _forest(1, 200, 6, 7, 4)
    cf = m.compile()
    T, N, off = cf.n_trees, X.shape[0], 1000
    f = cf.transform(X, fid_offset=off)
    assert f.row_ptr.dtype == torch.int32 and f.fids.dtype == torch.int32
    assert torch.equal(f.row_ptr,
                       torch.arange(0, N * T + 1, T, dtype=torch.int32))
    assert torch.equal(f.vals, torch.ones(N * T))
    assert torch.equal(f.fields, torch.arange(T, dtype=torch.int32).repeat(N))
    fids = f.fids.view(N, T)
    assert int(fids.min()) >= off and int(fids.max()) < off + cf.n_leaves
    leaf = leaf_oracle(m, X)
    seen = {}
    for t in range(T):
        # one fid per distinct leaf of the tree, and the other way round
        pairs = set(zip(leaf[:, t].tolist(), fids[:, t].tolist()))
        assert len({p[0] for p in pairs}) == len(pairs)
        assert len({p[1] for p in pairs}) == len(pairs)
        for _, fid in pairs:
            assert seen.setdefault(fid, t) == t  # trees are disjoint
        n_leaf_t = int((m.trees[t][0].feature < 0).sum())
        lo = off + int(cf.leaf_base[t])
        assert all(lo <= fid < lo + n_leaf_t for _, fid in pairs)
    assert torch.equal(cf.transform(X).fids + off, f.fids)


@pytest.mark.parametrize("n_bins", [255, 16])
def test_special_inputs(n_bins):
    """10% NaN, +-inf, exact edge values, tied / constant / all-NaN
    columns; thresholds past the last edge (always n_bins=16)."""
    m, X = _forest(2, 400, 6, 6, 5, special=True, n_bins=n_bins)
    assert torch.isnan(X[:, -1]).all() and torch.isinf(X).any()
    _check_all(m, X)
    # every exact edge value of every column, as a probe row set
    E = m.bin_edges
    P = E.t().contiguous().clone()
    _check_all(m, P)


def test_degenerate_shapes():
    g = torch.Generator().manual_seed(3)
    # empty forest
    X = make_X(g, 10, 4)
    m = make_model([], X)
    cf = m.compile()
    assert cf.n_trees == 0 and cf.n_leaves == 0 and cf.max_depth == 0
    assert torch.equal(cf.predict_margin(X), torch.zeros(10, 1))
    assert torch.equal(cf.predict_proba(X), m.predict_proba(X))
    assert cf.predict_leaf(X).shape == (10, 0)
    f = cf.transform(X)
    assert f.fids.numel() == 0 and f.row_ptr.shape == (11,)
    assert not f.row_ptr.any()
    # N == 0
    m, _ = _forest(4, 50, 4, 3, 3)
    cf = m.compile()
    X0 = torch.zeros(0, 4)
    assert cf.predict_margin(X0).shape == (0, 1)
    assert cf.predict_leaf(X0).shape == (0, 3)
    f = cf.transform(X0)
    assert f.fids.numel() == 0 and torch.equal(
        f.row_ptr, torch.zeros(1, dtype=torch.int32))
    # root-only trees
    trees = [tree_with_nodes(g, 4, 1, 0) for _ in range(3)]
    m = make_model(trees, X)
    cf = _check_all(m, X)
    assert cf.max_depth == 0 and cf.n_leaves == 3
    assert not cf.predict_leaf(X).any()
    # D == 1
    m, X1 = _forest(5, 77, 1, 5, 4)
    _check_all(m, X1)


def _one_tree_model():
    g = torch.Generator().manual_seed(6)
    X = make_X(g, 20, 3)
    return make_model([tree_with_nodes(g, 3, 7, 3)], X), X


def test_validation_errors():
    m, X = _one_tree_model()
    m.compile()  # the untouched tree is fine
    t = m.trees[0][0]
    internal = int((t.feature >= 0).nonzero()[0])

    def broken(field, value, at=internal):
        m2, _ = _one_tree_model()
        getattr(m2.trees[0][0], field)[at] = value
        return m2

    with pytest.raises(ValueError):  # child index <= parent
        broken("left", internal).compile()
    with pytest.raises(ValueError):
        broken("right", 0).compile()
    with pytest.raises(ValueError):  # child out of range
        broken("right", 7).compile()
    with pytest.raises(ValueError):  # feature >= D
        broken("feature", 3).compile()
    with pytest.raises(ValueError):  # leaf marker other than -1
        broken("feature", -2).compile()
    leaf = int((t.feature < 0).nonzero()[0])
    with pytest.raises(ValueError):  # NaN leaf value
        broken("value", float("nan"), at=leaf).compile()
    with pytest.raises(ValueError):
        broken("value", float("inf"), at=leaf).compile()
    m2, _ = _one_tree_model()
    m2.bin_edges[:] = float("nan")
    m2.trees[0][0].threshold[internal] = 0
    with pytest.raises(ValueError):  # split on a NaN bin edge
        m2.compile()
    cf = m.compile()
    with pytest.raises(ValueError):  # wrong D
        cf.predict_margin(torch.zeros(4, 2))
    with pytest.raises(ValueError):  # fp64 X
        cf.predict_margin(X.double())
    with pytest.raises(ValueError):
        cf.predict_leaf(X.double())
    with pytest.raises(ValueError):
        cf.transform(torch.zeros(4, 5))


def test_noncontiguous_X():
    m, X = _forest(7, 100, 5, 4, 4)
    big = torch.randn(100, 9)
    big[:, 2:7] = X
    view = big[:, 2:7]
    assert not view.is_contiguous()
    assert torch.equal(m.compile().predict_margin(view), m.predict_margin(X))


@pytest.mark.parametrize("n_classes", [2, 3])
def test_fit_save_load_roundtrip(tmp_path, n_classes):
    g = torch.Generator().manual_seed(8)
    X = torch.randn(500, 6, generator=g)
    X[torch.rand(500, 6, generator=g) < 0.05] = float("nan")
    s = torch.nan_to_num(X[:, 0]) + torch.nan_to_num(X[:, 1] * X[:, 2])
    y = (s > 0).float() if n_classes == 2 else \
        torch.bucketize(s, torch.tensor([-0.5, 0.5])).float()
    m = GBMModel(GBMHyper(n_rounds=5, max_depth=3, n_classes=n_classes),
                 device="cpu").fit(X, y)
    path = str(tmp_path / "gbm.pt")
    m.save(path)
    cf = CompiledForest.load(path, "cpu")
    K = 1 if n_classes == 2 else n_classes
    assert cf.n_trees == 5 * K and cf.n_classes == K
    assert torch.equal(cf.predict_margin(X), m.predict_margin(X))
    assert torch.equal(cf.predict_proba(X), m.predict_proba(X))
    assert torch.equal(cf.predict_leaf(X), leaf_oracle(m, X))


def _stack_hyper():
    return GBDTLRHyper(gbm=GBMHyper(n_rounds=10, max_depth=4, colsample=1.0,
                                    n_classes=2),
                       lr_optimizer="adagrad", epochs=5, batch=256)


def test_gbdt_lr_stacking_auc(tmp_path):
    """Held-out AUC of the stack >= AUC of its own GBM stage - 0.01 (the
    margin covers LR summation-order noise, not a regression). Measured
    on CPU: GBM 0.7948, stacked 0.8027 in the issue's prototype; this
    implementation's values are recorded in docs/TESTING.md."""
    Xtr, ytr = stacking_data(2000, 0)
    Xte, yte = stacking_data(1000, 1)
    model = GBDTLRModel(_stack_hyper(), device="cpu").fit(Xtr, ytr)
    p = model.predict_proba(Xte)
    assert p.shape == (1000,) and torch.isfinite(p).all()
    auc_stack = auc_score(p, yte)
    auc_gbm = auc_score(model.gbm.predict_proba(Xte), yte)
    print(f"gbdt_lr held-out AUC: gbm={auc_gbm:.4f} stacked={auc_stack:.4f}")
    assert auc_stack >= auc_gbm - 0.01
    # save / load round trip gives equal predictions
    path = str(tmp_path / "stack.pt")
    model.save(path)
    again = GBDTLRModel(GBDTLRHyper(), device="cpu").load(path)
    assert torch.equal(again.predict_proba(Xte), p)
    # batching changes the LR reference's summation shape, not the model:
    # sigmoid outputs agree to fp32 rounding of a 10-term sum
    assert torch.allclose(BatchPredictor(again, batch_size=300)
                          .predict_dense(Xte), p, rtol=0, atol=1e-6)


def test_gbdt_lr_rejects_multiclass():
    with pytest.raises(ValueError):
        GBDTLRModel(GBDTLRHyper(gbm=GBMHyper(n_classes=3)), device="cpu")


def test_cli_dense_serving(tmp_path, capsys):
    from lightctr_amd.cli import main

    data = os.path.join(ROOT, "data", "train_dense.csv")
    for model in ("gbdt_lr", "gbm"):
        path = str(tmp_path / f"{model}.pt")
        dump = str(tmp_path / f"{model}.scores")
        rc = main(["train", "--model", model, "--data", data, "--rows",
                   "120", "--epochs", "1", "--batch", "64", "--device",
                   "cpu", "--save", path])
        assert rc == 0, model
        assert "final" in json.loads(
            capsys.readouterr().out.strip().splitlines()[-1])
        rc = main(["predict", "--model", model, "--data", data, "--rows",
                   "120", "--device", "cpu", "--load", path, "--dump", dump,
                   "--batch", "50"])
        assert rc == 0, model
        rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert "accuracy" in rep
        if model == "gbdt_lr":
            assert 0.0 <= rep["auc"] <= 1.0 and "logloss" in rep
        with open(dump) as f:
            assert len(f.readlines()) == 120, model


def test_bench_forest_cpu_smoke():
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "tools", "bench_forest.py"),
         "--rows", "2000", "--cols", "8", "--trees", "5", "--depth", "4",
         "--rounds", "2", "--cpu"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["bit_identical"] and rep["compiled_rows_per_s"] > 0
