"""gbm_forest_kernel on the GPU against the CPU GBMModel (margins with
torch.equal — the kernel sums leaf values in tree order in one thread per
row) and the CPU leaf oracle."""

import pytest
import torch

from gbm_forest_util import (forest_sizes, leaf_oracle, make_model, make_X,
                             put_edge_values, random_tree, stacking_data,
                             tree_with_nodes)
from lightctr_amd.models import (GBDTLRHyper, GBDTLRModel, LRHyper, LRModel)
from lightctr_amd.models.gbm import GBMHyper
from lightctr_amd.predict import CompiledForest
from lightctr_amd.utils.metrics import auc_score

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from lightctr_amd.ops._extension import require_hip_ops

    return require_hip_ops()


def _check_gpu(m, X, Xg=None):
    """Compile the CPU model for the GPU and compare margins, proba, leaf
    ids and leaf features with the CPU oracles."""
    cf = m.compile(device=DEV)
    Xg = X.to(DEV) if Xg is None else Xg
    got = cf.predict_margin(Xg)
    assert got.device.type == "cuda" and got.dtype == torch.float32
    assert torch.equal(got.cpu(), m.predict_margin(X))
    leaf = cf.predict_leaf(Xg)
    assert leaf.dtype == torch.int32
    assert torch.equal(leaf.cpu(), leaf_oracle(m, X))
    ref = m.compile(device="cpu").transform(X, fid_offset=17)
    f = cf.transform(Xg, fid_offset=17)
    for a, b in zip(f, ref):
        assert torch.equal(a.cpu(), b)
    return cf


def _model(seed, D, n_trees, depth, K=1, n_bins=255, Nfit=300):
    g = torch.Generator().manual_seed(seed)
    trees = [random_tree(g, D, depth) for _ in range(n_trees)]
    return make_model(trees, make_X(g, Nfit, D), K=K, n_bins=n_bins,
                      max_depth=depth), g


@pytest.fixture(scope="module")
def small_model():
    return _model(0, 5, 7, 4)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_counts(small_model, N):
    m, _ = small_model
    X = make_X(torch.Generator().manual_seed(N), N, 5)
    _check_gpu(m, X)


@pytest.mark.parametrize("D", [1, 39, 130])
def test_feature_counts_multiclass(D):
    m, g = _model(D, D, 15, 4, K=3)  # 5 rounds x 3 classes
    X = make_X(g, 777, D)
    cf = _check_gpu(m, X)
    assert cf.n_classes == 3
    # margins are bit-equal (checked above); softmax itself runs on two
    # devices, so a few fp32 ulps
    assert torch.allclose(cf.predict_proba(X.to(DEV)).cpu(),
                          m.predict_proba(X), rtol=1e-5, atol=1e-7)


def test_many_classes_fall_back_to_global_accumulators():
    K = _ops().gbm_forest_max_register_classes() + 2
    m, g = _model(11, 6, 2 * K, 3, K=K)
    _check_gpu(m, make_X(g, 515, 6))


@pytest.mark.parametrize("extra", ["C", "C+1", "2C+1"])
def test_chunk_boundaries(extra):
    C = _ops().gbm_forest_chunk_capacity()
    total = {"C": C, "C+1": C + 1, "2C+1": 2 * C + 1}[extra]
    g = torch.Generator().manual_seed(total)
    D = 9
    trees = [tree_with_nodes(g, D, n, 6) for n in forest_sizes(total)]
    m = make_model(trees, make_X(g, 300, D), max_depth=6)
    cf = _check_gpu(m, make_X(g, 600, D))
    assert int(cf.nodes.shape[0]) == total
    ch = cf.chunks.cpu()
    assert int(ch.shape[0]) == {"C": 1, "C+1": 2, "2C+1": 3}[extra]
    assert bool(ch[:, 3].all())  # every chunk fits the LDS buffer
    assert int(ch[:, 1].sum()) == len(trees)


def test_oversized_tree_between_small_trees():
    """small, > C nodes (walked from global memory), small: order of the
    sum is kept across the switch."""
    C = _ops().gbm_forest_chunk_capacity()
    g = torch.Generator().manual_seed(5)
    D = 12
    trees = [random_tree(g, D, 4), tree_with_nodes(g, D, C + 101, 14),
             random_tree(g, D, 4)]
    m = make_model(trees, make_X(g, 300, D), max_depth=14)
    cf = _check_gpu(m, make_X(g, 1500, D))
    assert cf.chunks.cpu()[:, 3].tolist() == [1, 0, 1]
    assert 4 < cf.max_depth <= 14


@pytest.mark.parametrize("n_bins", [255, 16])
def test_special_inputs(n_bins):
    g = torch.Generator().manual_seed(21)
    D = 6
    X = make_X(g, 700, D, special=True)
    trees = [random_tree(g, D, 5) for _ in range(6)]
    m = make_model(trees, X, n_bins=n_bins, max_depth=5)
    X = put_edge_values(g, X, m.bin_edges)
    assert torch.isnan(X[:, -1]).all() and torch.isinf(X).any()
    _check_gpu(m, X)
    _check_gpu(m, m.bin_edges.t().contiguous().clone())


def test_degenerate_shapes(small_model):
    m, g = small_model
    X = make_X(g, 10, 5)
    empty = make_model([], X).compile(device=DEV)
    assert torch.equal(empty.predict_margin(X.to(DEV)).cpu(),
                       torch.zeros(10, 1))
    assert empty.predict_leaf(X.to(DEV)).shape == (10, 0)
    assert empty.transform(X.to(DEV)).fids.numel() == 0
    cf = m.compile(device=DEV)
    X0 = torch.zeros(0, 5, device=DEV)
    assert cf.predict_margin(X0).shape == (0, 1)
    assert cf.predict_leaf(X0).shape == (0, 7)
    assert cf.transform(X0).row_ptr.cpu().tolist() == [0]
    roots = make_model([tree_with_nodes(g, 5, 1, 0) for _ in range(3)], X)
    assert _check_gpu(roots, X).max_depth == 0


def test_noncontiguous_and_offset_views(small_model):
    m, g = small_model
    X = make_X(g, 300, 5)
    big = torch.randn(300, 9, generator=g)
    big[:, 2:7] = X
    sliced = big.to(DEV)[:, 2:7]
    assert not sliced.is_contiguous()
    _check_gpu(m, X, sliced)
    # contiguous view that starts one element into a larger buffer: the
    # base is only 4-byte aligned
    buf = torch.zeros(300 * 5 + 1, device=DEV)
    buf[1:] = X.to(DEV).reshape(-1)
    view = buf[1:].view(300, 5)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    _check_gpu(m, X, view)


def test_second_grid_trip():
    """The grid is clamped; one row past the first trip's coverage runs
    the grid-stride loop a second time in block 0."""
    N = _ops().gbm_forest_rows_per_grid() + 1
    m, g = _model(31, 2, 2, 3)
    X = torch.randn(N, 2, generator=g)
    cf = m.compile(device=DEV)
    Xg = X.to(DEV)
    assert torch.equal(cf.predict_margin(Xg).cpu(), m.predict_margin(X))
    leaf = cf.predict_leaf(Xg).cpu()
    tail = slice(N - 2000, N)
    assert torch.equal(leaf[tail], leaf_oracle(m, X[tail]))


def test_repeatable(small_model):
    m, g = small_model
    Xg = make_X(g, 5000, 5, special=True).to(DEV)
    cf = m.compile(device=DEV)
    a, b = cf.predict_margin(Xg), cf.predict_margin(Xg)
    assert torch.equal(a, b)
    assert torch.equal(cf.transform(Xg).fids, cf.transform(Xg).fids)


def test_transform_feeds_lr(small_model):
    m, g = small_model
    X = make_X(g, 400, 5)
    cpu, gpu = m.compile(device="cpu"), m.compile(device=DEV)
    lr_c = LRModel(LRHyper(num_features=cpu.n_leaves), device="cpu")
    lr_c.W.copy_(torch.randn(cpu.n_leaves, generator=g))
    lr_g = LRModel(LRHyper(num_features=gpu.n_leaves), device=DEV)
    lr_g.W.copy_(lr_c.W)
    fc, fg = cpu.transform(X), gpu.transform(X.to(DEV))
    pc = lr_c.predict_proba(fc.row_ptr, fc.fids, fc.vals)
    pg = lr_g.predict_proba(fg.row_ptr, fg.fids, fg.vals)
    assert torch.allclose(pg.cpu(), pc, rtol=0, atol=1e-6)


def test_fitted_model_load_on_gpu(tmp_path):
    from lightctr_amd.models.gbm import GBMModel

    g = torch.Generator().manual_seed(8)
    X = torch.randn(500, 6, generator=g)
    y = (X[:, 0] + X[:, 1] * X[:, 2] > 0).float()
    m = GBMModel(GBMHyper(n_rounds=5, max_depth=3), device="cpu").fit(X, y)
    path = str(tmp_path / "gbm.pt")
    m.save(path)
    cf = CompiledForest.load(path, DEV)
    assert torch.equal(cf.predict_margin(X.to(DEV)).cpu(),
                       m.predict_margin(X))


def test_gbdt_lr_on_gpu():
    """Same recipe and AUC condition as the CPU test, on cuda:0, against
    the model's own GBM stage."""
    Xtr, ytr = stacking_data(2000, 0)
    Xte, yte = stacking_data(1000, 1)
    hyper = GBDTLRHyper(gbm=GBMHyper(n_rounds=10, max_depth=4, colsample=1.0,
                                     n_classes=2),
                        lr_optimizer="adagrad", epochs=5, batch=256)
    model = GBDTLRModel(hyper, device=DEV).fit(Xtr.to(DEV), ytr.to(DEV))
    p = model.predict_proba(Xte.to(DEV)).cpu()
    assert p.shape == (1000,) and torch.isfinite(p).all()
    auc_stack = auc_score(p, yte)
    auc_gbm = auc_score(model.gbm.predict_proba(Xte.to(DEV)).cpu(), yte)
    print(f"gbdt_lr GPU held-out AUC: gbm={auc_gbm:.4f} "
          f"stacked={auc_stack:.4f}")
    assert auc_stack >= auc_gbm - 0.01
