"""GPU tests of forest_candidates_kernel (ops/csrc/knn_kernels.hip) and of
ForestIndex on ``cuda:0``.

Exact set (``forest_oracles`` exact-input rule): ``candidates`` must be
equal to the CPU path, which ``test_forest.py`` holds to the contract's
oracle, and ``search`` ids equal and distances bit-equal. One axis is varied
at a time around the base case. Float set: structural conditions, the sum
rule of ``knn_oracles`` for the distances and at most 2 of 64 id rows that
differ from the CPU path on the same arrays (a margin's sign or two queue
bounds within fp32 summation error of each other). No test hands a
malformed forest to the kernel."""

import pytest
import torch

import forest_oracles as fo
import knn_oracles as ko
from kernel_oracles import check_bits
from lightctr_amd.ops._extension import require_hip_ops
from lightctr_amd.predict import ForestIndex
from lightctr_amd.predict.rp_forest import FOREST_MAX_SEARCH, FOREST_QUEUE

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METRICS = ("l2", "ip")


@pytest.fixture(scope="module")
def ops():
    return require_hip_ops()


def check(name, got, ref):
    assert torch.equal(got[0].cpu(), ref[0]), f"{name}: ids differ"
    check_bits(name, got[1], ref[1])


def indexes(f, metric="l2"):
    """(CPU index, GPU index) over the same arrays"""
    return (ForestIndex(f.X, *f.arrays(), metric=metric),
            ForestIndex(f.X.to(DEV), *f.arrays(DEV), metric=metric))


# ---------------------------------------------------------------------------
# exact set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", fo.EXACT_CASES)
def test_exact_case(ops, name):
    f, Q, sk = fo.case(name)
    cx, gx = indexes(f)
    ref = cx.candidates(Q, sk)
    got = gx.candidates(Q.to(DEV), sk)
    assert got.is_cuda and got.dtype == torch.int32
    assert got.shape == ref.shape == (Q.shape[0], f.width(sk))
    assert torch.equal(got.cpu(), ref), f"{name}: candidates differ"
    raw = ops.forest_candidates(*f.arrays(DEV), Q.to(DEV), sk, f.width(sk))
    assert torch.equal(raw, got)
    for metric in METRICS:
        cx, gx = indexes(f, metric)
        check(f"{name}/{metric}", gx.search(Q.to(DEV), 10, search_k=sk),
              cx.search(Q, 10, search_k=sk))


def test_planted_answers(ops):
    """the queue bound during descent and the zero-margin tie, as ids"""
    f, Q, sk = fo.case("chain_far")
    got = indexes(f)[1].candidates(Q.to(DEV), sk)[0].tolist()
    assert got[:fo.QUEUE] == list(range(1199, 175, -1))
    assert set(got[fo.QUEUE:]) == {-1}
    f, Q, sk = fo.case("chain_near")
    assert indexes(f)[1].candidates(Q.to(DEV), sk)[0].tolist() == \
        list(range(1200))
    f, Q, sk = fo.case("zero_margin_root")
    got = indexes(f)[1].candidates(Q.to(DEV), sk)[0].tolist()
    assert got[:f.total] == fo.walk(f, Q[0], sk)[0]
    assert got[:f.total] != fo.walk(f, Q[0], sk, tie_low=False)[0]


def test_wider_row_is_padded(ops):
    f, Q, sk = fo.case("base")
    R = f.width(sk)
    got = ops.forest_candidates(*f.arrays(DEV), Q.to(DEV), sk, R + 70)
    assert torch.equal(got[:, :R].cpu(), fo.case_candidates("base"))
    assert bool((got[:, R:] == -1).all())


def test_poisoned_outputs_and_run_to_run(ops):
    """the padding is written by the kernel; two runs are bit-equal"""
    runs = []
    for name in ("base", "search_k=total+1", "chain_far"):
        f, Q, sk = fo.case(name)
        arrays, Qd, R = f.arrays(DEV), Q.to(DEV), f.width(sk)
        pair = []
        for _ in range(2):
            block = torch.full((Q.shape[0], R), -7, dtype=torch.int32,
                               device=DEV)
            torch.cuda.synchronize()
            del block
            pair.append(ops.forest_candidates(*arrays, Qd, sk, R))
        assert torch.equal(pair[0], pair[1])
        assert torch.equal(pair[0].cpu(), fo.case_candidates(name))
        runs.append(pair)
    assert bool((runs[1][0] == -1).any())


def test_empty_table_and_no_queries(ops):
    ix = ForestIndex.build(torch.zeros(0, 4, device=DEV), n_trees=2)
    Q = ko.ints((3, 4), 1).to(DEV)
    assert bool((ix.candidates(Q, 5) == -1).all())
    ids, dist = ix.search(Q, 4)
    assert bool((ids == -1).all()) and bool((dist == ko.INF).all())
    f, Q, sk = fo.case("base")
    got = ops.forest_candidates(*f.arrays(DEV), Q[:0].to(DEV), sk, 50)
    assert got.shape == (0, 50) and got.is_cuda


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------
def test_bindings_raise(ops):
    f, Q, sk = fo.case("base")
    a = dict(zip(fo.Forest.FIELDS, f.arrays(DEV)))
    Qd, R = Q.to(DEV), f.width(sk)
    assert ops.forest_queue() == FOREST_QUEUE == fo.QUEUE
    assert ops.forest_max_search() == FOREST_MAX_SEARCH == fo.MAX_SEARCH

    def bad(Q=Qd, search_k=sk, width=R, **repl):
        arrays = [repl.get(k, a[k]) for k in fo.Forest.FIELDS]
        with pytest.raises(RuntimeError):
            ops.forest_candidates(*arrays, Q, search_k, width)

    ops.forest_candidates(*a.values(), Qd, sk, R)  # the good call
    bad(planes=a["planes"].double())  # dtypes
    bad(bias=a["bias"].double())
    bad(child=a["child"].long())
    bad(roots=a["roots"].long())
    bad(leaf_off=a["leaf_off"].long())
    bad(leaf_items=a["leaf_items"].long())
    bad(Q=Qd.double())
    for k in fo.Forest.FIELDS:  # CPU tensors
        bad(**{k: a[k].cpu()})
    bad(Q=Q)
    bad(search_k=0)
    bad(search_k=FOREST_MAX_SEARCH + 1, width=FOREST_MAX_SEARCH + R)
    bad(width=sk - 1)
    bad(Q=Qd[:, :8].contiguous())  # Q width mismatch
    bad(Q=Qd[:, ::2])  # not contiguous
    bad(bias=a["bias"][:-1].contiguous())  # shapes
    bad(child=a["child"].reshape(-1))
    bad(roots=a["roots"][:0])
    bad(leaf_off=a["leaf_off"][:0])
    with pytest.raises(RuntimeError):  # dim > 1024
        ops.forest_candidates(
            torch.zeros(1, 1025, device=DEV), torch.zeros(1, device=DEV),
            torch.tensor([[-1, -2]], dtype=torch.int32, device=DEV),
            a["roots"][:1] * 0, torch.tensor([0, 1, 2], dtype=torch.int32,
                                             device=DEV),
            torch.tensor([0, 1], dtype=torch.int32, device=DEV),
            torch.zeros(1, 1025, device=DEV), 1, 1)


# ---------------------------------------------------------------------------
# float set
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def float_set():
    X, Q = ko.flat_case(600, 32, 64, seed=101, exact=False)
    gx = ForestIndex.build(X.to(DEV), n_trees=4, leaf_size=8, seed=3)
    assert gx.planes.is_cuda and gx.leaf_items.is_cuda
    cx = ForestIndex(X, *(getattr(gx, n).cpu() for n in fo.Forest.FIELDS))
    return X, Q, gx, cx


def test_float_build_invariants_on_device(float_set):
    X, Q, gx, cx = float_set
    assert cx.max_leaf == gx.max_leaf <= 8  # the constructor accepted it
    per_tree = torch.zeros(600, dtype=torch.long)
    per_tree.index_add_(0, cx.leaf_items.long(),
                        torch.ones(cx.total, dtype=torch.long))
    assert bool((per_tree == 4).all())  # every row once per tree


@pytest.mark.parametrize("search_k", [1, 40, 300])
def test_float_candidates_structure(float_set, search_k):
    X, Q, gx, cx = float_set
    cand = gx.candidates(Q.to(DEV), search_k).cpu()
    assert cand.shape == (64, search_k + gx.max_leaf - 1)
    assert int(cand.min()) >= -1 and int(cand.max()) < 600
    pad = cand < 0
    assert bool((pad[:, 1:] >= pad[:, :-1]).all())  # -1 entries only trail
    count = (~pad).sum(1)
    assert bool((count >= search_k).all())  # 2400 items: never runs dry
    assert bool((count < search_k + gx.max_leaf).all())
    ids, dist = gx.search(Q.to(DEV), 10, search_k=search_k)
    ref = gx.flat.search(Q.to(DEV), 10, cand=gx.candidates(Q.to(DEV),
                                                           search_k))
    assert torch.equal(ids, ref[0])
    check_bits("search", dist, ref[1].cpu())
    # distances of the returned ids: the float sum rule
    d64, mag = ko.dist64(Q, X, "l2")
    ids, dist = ids.cpu().long(), dist.cpu().double()
    real = ids >= 0
    err = (dist - torch.gather(d64, 1, ids.clamp(min=0))).abs()
    bound = 32 * ko.U23 * torch.gather(mag, 1, ids.clamp(min=0))
    assert bool((err <= bound)[real].all())
    assert bool((dist[~real] == ko.INF).all())
    # against the CPU path on the same arrays
    differ = int((cand != cx.candidates(Q, search_k)).any(1).sum())
    print(f"ROWS forest search_k={search_k} differ {differ}/64")
    assert differ <= 2
    assert torch.equal(cx.candidates(Q, search_k),
                       cx.candidates(Q, search_k))


@pytest.mark.parametrize("metric", METRICS)
def test_float_search_everything_is_exact_search(float_set, metric):
    X, Q, gx, _ = float_set
    ix = ForestIndex(gx.X, *(getattr(gx, n) for n in fo.Forest.FIELDS),
                     metric=metric)
    ids, dist = ix.search(Q.to(DEV), 10, search_k=ix.total)
    d64, mag = ko.dist64(Q, X, metric)
    ko.check_float_result(f"forest_all_{metric}", ids, dist, d64, mag, 32,
                          10)


def test_embed_model_forest_on_device():
    from lightctr_amd.models.embedding import EmbedHyper, EmbedModel

    vocab = [f"w{i}" for i in range(200)]
    m = EmbedModel(vocab, [3] * 200, EmbedHyper(dim=32), device=DEV)
    m.E = ko.normals((200, 32), 91).to(DEV)
    words = vocab[:7]
    m.build_index(kind="flat")
    flat = m.neighbors(words, 5)
    ix = m.build_index(kind="forest", n_trees=4, leaf_size=8, seed=2)
    assert isinstance(ix, ForestIndex) and ix.planes.is_cuda
    got = m.neighbors(words, 5, search_k=ix.total)
    assert [[n for n, _ in r] for r in got] == \
        [[n for n, _ in r] for r in flat]
    assert all(len(r) == 5 for r in m.neighbors(words, 5))
