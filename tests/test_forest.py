"""CPU tests of ForestIndex (lightctr_amd/predict/rp_forest.py): the CPU
path against the contract's oracle (``forest_oracles``) on the exact set
that ``test_forest_gpu.py`` holds the kernel to, the constructor's
structure checks, the two builders, persistence, the wiring and the recall
condition of docs/TESTING.md."""

import json
import pathlib
import subprocess
import sys

import pytest
import torch

import forest_oracles as fo
import knn_oracles as ko
from lightctr_amd.predict import ANNIndex, FlatIndex, ForestIndex
from lightctr_amd.predict.rp_forest import FOREST_MAX_SEARCH, FOREST_QUEUE

REPO = pathlib.Path(__file__).resolve().parent.parent
METRICS = ("l2", "ip")


def index_of(f, metric="l2"):
    return ForestIndex(f.X, *f.arrays(), metric=metric)


def assert_same(got, ref):
    assert ko.same(got, ref)


def test_limits_mirror_the_oracle():
    assert (FOREST_QUEUE, FOREST_MAX_SEARCH) == (fo.QUEUE, fo.MAX_SEARCH)


# ---------------------------------------------------------------------------
# CPU path == oracle on the exact set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", fo.EXACT_CASES)
def test_candidates_equal_the_oracle(name):
    f, Q, sk = fo.case(name)
    ix = index_of(f)
    assert ix.max_leaf == f.max_leaf
    got = ix.candidates(Q, sk)
    assert got.dtype == torch.int32 and got.shape == (Q.shape[0],
                                                      f.width(sk))
    assert torch.equal(got, fo.case_candidates(name))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("name", fo.EXACT_CASES)
def test_search_equals_the_oracle(name, metric):
    f, Q, sk = fo.case(name)
    ref = ko.flat_ref(f.X, Q, metric, 10, cand=fo.case_candidates(name))
    assert_same(index_of(f, metric).search(Q, 10, search_k=sk), ref)


def test_oracle_on_the_chain():
    """the planted answers of the queue-bound cases, and that an unbounded
    queue is told from the bounded one"""
    f, Q, sk = fo.case("chain_far")
    ids, _, longest = fo.walk(f, Q[0], sk)
    assert ids == list(range(1199, 175, -1)) and longest == fo.QUEUE
    assert fo.walk(f, Q[0], sk, queue=None)[0] == list(range(1199, -1, -1))
    f, Q, sk = fo.case("chain_near")
    assert fo.walk(f, Q[0], sk)[0] == list(range(1200))
    f, Q, _ = fo.case("many_roots=4000")
    # 1030 roots: six are dropped at the seeding, and a full queue goes on
    # dropping leaves, so the walk runs dry before search_k
    ids, _, longest = fo.walk(f, Q[0], fo.MAX_SEARCH)
    assert longest == fo.QUEUE and len(ids) < 64 * fo.QUEUE
    assert len(fo.walk(f, Q[0], fo.MAX_SEARCH, queue=None)[0]) >= \
        fo.MAX_SEARCH


def test_oracle_zero_margin_root_pops_the_lower_code_first():
    """the query lies on the root plane of tree 0: both children are pushed
    with bound 0 (+0 and -0) and the walk must take the lower code first;
    the case tells the wrong tie rule from the right one"""
    f, Q, sk = fo.case("zero_margin_root")
    assert fo.walk(f, Q[0], sk)[0] != fo.walk(f, Q[0], sk, tie_low=False)[0]
    assert sorted(fo.walk(f, Q[0], sk)[0]) == sorted(
        f.leaf_items.tolist())


def test_default_search_k_and_flat_equivalence():
    f, Q, _ = fo.case("base")
    for metric in METRICS:
        ix = index_of(f, metric)
        assert_same(ix.search(Q, 3), ix.search(Q, 3, search_k=3 * 4 * 2))
        # search_k >= total: every row is a candidate
        assert_same(ix.search(Q, 10, search_k=f.total),
                    FlatIndex(f.X, metric).search(Q, 10))


def test_empty_table():
    X = torch.zeros(0, 4)
    ix = ForestIndex.build(X, n_trees=2)
    assert ix.N == 0 and bool((ix.roots < 0).all()) and ix.max_leaf == 0
    Q = ko.ints((3, 4), 1)
    assert bool((ix.candidates(Q, 5) == -1).all())
    ids, dist = ix.search(Q, 4)
    assert bool((ids == -1).all()) and bool((dist == ko.INF).all())


# ---------------------------------------------------------------------------
# constructor and argument checks
# ---------------------------------------------------------------------------
def broken(f, **repl):
    a = dict(zip(fo.Forest.FIELDS, (t.clone() for t in f.arrays())))
    a.update(repl)
    return [a[k] for k in fo.Forest.FIELDS]


def test_constructor_value_errors():
    f, Q, _ = fo.case("base")
    a = dict(zip(fo.Forest.FIELDS, f.arrays()))
    n_inner, n_leaves = f.planes.shape[0], f.leaf_off.numel() - 1
    index_of(f)  # the unbroken forest is accepted

    def bad(X=f.X, **repl):
        with pytest.raises(ValueError):
            ForestIndex(X, *broken(f, **repl))

    # dtypes
    bad(planes=a["planes"].double())
    bad(bias=a["bias"].double())
    bad(child=a["child"].long())
    bad(roots=a["roots"].long())
    bad(leaf_off=a["leaf_off"].long())
    bad(leaf_items=a["leaf_items"].long())
    bad(X=f.X.double())
    # shapes
    bad(planes=a["planes"][:, :8].contiguous())
    bad(planes=a["planes"][:-1].contiguous())
    bad(bias=a["bias"][:-1].contiguous())
    bad(child=a["child"].reshape(-1))
    bad(child=a["child"][:-1].contiguous())
    bad(roots=a["roots"].reshape(2, 2))
    bad(leaf_off=a["leaf_off"][:0])
    # T >= 1
    bad(roots=a["roots"][:0])
    # dim in [1, KNN_MAX_DIM]
    with pytest.raises(ValueError):
        ForestIndex(torch.zeros(3, 1025), torch.zeros(0, 1025),
                    torch.zeros(0), torch.zeros(0, 2, dtype=torch.int32),
                    torch.tensor([-1], dtype=torch.int32),
                    torch.tensor([0, 3], dtype=torch.int32),
                    torch.arange(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        ForestIndex(torch.zeros(3, 0), torch.zeros(0, 0),
                    torch.zeros(0), torch.zeros(0, 2, dtype=torch.int32),
                    torch.tensor([-1], dtype=torch.int32),
                    torch.tensor([0, 3], dtype=torch.int32),
                    torch.arange(3, dtype=torch.int32))
    # finite planes and biases
    p = a["planes"].clone()
    p[1, 2] = float("nan")
    bad(planes=p)
    b = a["bias"].clone()
    b[0] = float("inf")
    bad(bias=b)
    # topological child codes: child[i] <= i
    inner = (a["child"][:, 0] >= 0).nonzero()[0].item()
    for c in (inner, 0 if inner else inner):
        ch = a["child"].clone()
        ch[inner, 0] = c
        bad(child=ch)
    ch = a["child"].clone()
    ch[3, 1] = 2
    bad(child=ch)
    # codes in range
    ch = a["child"].clone()
    ch[0, 0] = n_inner
    bad(child=ch)
    ch = a["child"].clone()
    ch[0, 1] = -1 - n_leaves
    bad(child=ch)
    r = a["roots"].clone()
    r[1] = -1 - n_leaves
    bad(roots=r)
    r[1] = n_inner
    bad(roots=r)
    # a node with two parents
    r = a["roots"].clone()
    r[1] = r[0]
    bad(roots=r)
    # leaf_off from 0 to total, non-decreasing
    lo = a["leaf_off"].clone()
    lo[0] = 1
    bad(leaf_off=lo)
    lo = a["leaf_off"].clone()
    lo[-1] += 1
    bad(leaf_off=lo)
    lo = a["leaf_off"].clone()
    lo[2] = lo[1] - 1
    bad(leaf_off=lo)
    # items in [0, N)
    it = a["leaf_items"].clone()
    it[5] = f.X.shape[0]
    bad(leaf_items=it)
    it[5] = -1
    bad(leaf_items=it)
    with pytest.raises(ValueError):
        ForestIndex(f.X, *f.arrays(), metric="cosine")


def test_search_argument_errors():
    f, Q, _ = fo.case("base")
    ix = index_of(f)
    for sk in (0, -1, FOREST_MAX_SEARCH + 1, 2.5):
        with pytest.raises(ValueError):
            ix.candidates(Q, sk)
    with pytest.raises(ValueError):
        ix.candidates(Q[:, :5], 10)
    with pytest.raises(ValueError):
        ix.candidates(Q.double(), 10)
    Qb = Q.clone()
    Qb[0, 0] = float("nan")
    with pytest.raises(ValueError):
        ix.candidates(Qb, 10)
    with pytest.raises(ValueError):
        ix.search(Q, 0)
    with pytest.raises(ValueError):
        ix.search(Q, 257)
    assert ix.candidates(Q[:0], 10).shape == (0, f.width(10))
    assert ix.candidates(Q, FOREST_MAX_SEARCH).shape[1] == \
        f.width(FOREST_MAX_SEARCH)


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def tree_rows(ix):
    """per tree, the sorted rows of its leaves (walks the child table)"""
    child, off = ix.child.tolist(), ix.leaf_off.tolist()
    items = ix.leaf_items.tolist()
    out = []
    for root in ix.roots.tolist():
        rows, stack = [], [root]
        while stack:
            c = stack.pop()
            if c < 0:
                rows.extend(items[off[-1 - c]:off[-c]])
            else:
                stack.extend(child[c])
        out.append(sorted(rows))
    return out


def ann_leaves(node, out):
    if node.items is not None:
        out.append(node.items.tolist())
    else:
        ann_leaves(node.left, out)
        ann_leaves(node.right, out)
    return out


def test_from_ann_round_trip():
    X = ko.normals((300, 12), 5)
    ann = ANNIndex(X, n_trees=3, leaf_size=10, seed=2)
    ix = ForestIndex.from_ann(ann)
    assert ix.n_trees == 3 and ix.X is X
    assert tree_rows(ix) == [list(range(300))] * 3
    # pre-order: leaves come in left-to-right order, tree after tree
    want = [leaf for t in ann.trees for leaf in ann_leaves(t, [])]
    off = ix.leaf_off.tolist()
    got = [ix.leaf_items[a:b].tolist() for a, b in zip(off, off[1:])]
    assert got == want
    # the same planes: a walk from the root follows ANNIndex's sides
    node, code = ann.trees[0], int(ix.roots[0])
    q = X[7]
    while node.items is None:
        assert torch.equal(ix.planes[code], node.w)
        m = float(node.w @ q + node.b)
        node = node.left if m > 0 else node.right
        code = int(ix.child[code, 0 if m > 0 else 1])
    assert ix.leaf_items[off[-1 - code]:off[-code]].tolist() == \
        node.items.tolist()
    assert 7 in node.items.tolist()
    # a single-leaf ANN tree
    small = ForestIndex.from_ann(ANNIndex(X[:5], n_trees=2, leaf_size=8))
    assert small.roots.tolist() == [-1, -2] and small.n_inner == 0


@pytest.mark.parametrize("N,leaf", [(1000, 16), (257, 1), (40, 64)])
def test_build_invariants(N, leaf):
    X = ko.normals((N, 8), N)
    ix = ForestIndex.build(X, n_trees=3, leaf_size=leaf, seed=4)
    assert ix.n_trees == 3
    assert tree_rows(ix) == [list(range(N))] * 3
    assert ix.max_leaf <= leaf  # distinct float rows always split
    own = torch.arange(ix.n_inner)[:, None]
    assert bool(((ix.child < 0) | (ix.child > own)).all())
    jx = ForestIndex.build(X, n_trees=3, leaf_size=leaf, seed=4)
    for name in fo.Forest.FIELDS:
        assert torch.equal(getattr(ix, name), getattr(jx, name)), name
    kx = ForestIndex.build(X, n_trees=3, leaf_size=leaf, seed=5)
    assert N <= leaf or not torch.equal(kx.planes, ix.planes)
    # ids ascend inside a leaf (the regrouping sort is stable)
    off = ix.leaf_off.tolist()
    for a, b in zip(off, off[1:]):
        seg = ix.leaf_items[a:b].tolist()
        assert seg == sorted(seg)


def test_build_unsplittable_nodes_become_leaves():
    X = ko.normals((200, 6), 8)
    X[50:90] = X[50]  # 40 equal rows
    ix = ForestIndex.build(X, n_trees=2, leaf_size=8, seed=0)
    assert tree_rows(ix) == [list(range(200))] * 2
    off = ix.leaf_off.tolist()
    for a, b in zip(off, off[1:]):
        seg = ix.leaf_items[a:b]
        if b - a > 8:  # longer than leaf_size only where no plane splits
            assert bool((X[seg.long()] == X[seg[0]]).all())
    assert ix.max_leaf >= 40
    every = torch.ones(150, 4)
    one = ForestIndex.build(every, n_trees=2, leaf_size=8)
    assert one.n_inner == 0 and one.max_leaf == 150


def test_save_load_round_trip(tmp_path):
    f, Q, sk = fo.case("base")
    ix = index_of(f, "ip")
    p = str(tmp_path / "forest.pt")
    ix.save(p)
    jx = ForestIndex.load(p)
    assert jx.metric == "ip" and jx.max_leaf == ix.max_leaf
    for name in fo.Forest.FIELDS:
        assert torch.equal(getattr(ix, name), getattr(jx, name)), name
    assert_same(jx.search(Q, 10, search_k=sk), ix.search(Q, 10, search_k=sk))
    ix.save(p, keep_vectors=False)
    with pytest.raises(ValueError):
        ForestIndex.load(p)
    kx = ForestIndex.load(p, vectors=f.X)
    assert torch.equal(kx.candidates(Q, sk), ix.candidates(Q, sk))


# ---------------------------------------------------------------------------
# EmbedModel, CLI, bench tool
# ---------------------------------------------------------------------------
def test_embed_model_forest_index():
    from test_knn import toy_embed_model

    m = toy_embed_model()
    words = list(m.vocab)
    m.build_index(kind="flat")
    flat = m.neighbors(words, 3)
    ix = m.build_index(kind="forest", n_trees=2, leaf_size=2, seed=1)
    assert isinstance(ix, ForestIndex) and ix.metric == "ip"
    # search_k covers every row: the flat answer (the candidate path sums
    # in another order; unit vectors, 16 terms)
    for a, b in zip(m.neighbors(words, 3, search_k=2 * len(words)), flat):
        assert [n for n, _ in a] == [n for n, _ in b]
        for (_, sa), (_, sb) in zip(a, b):
            assert abs(sa - sb) <= 2 * 16 * ko.U23
    assert all(len(r) <= 3 for r in m.neighbors(words, 3))
    with pytest.raises(ValueError):
        m.build_index(kind="tree")


def run_cli(*argv):
    r = subprocess.run([sys.executable, "-m", "lightctr_amd.cli", *argv],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()


def test_cli_neighbors_forest(tmp_path):
    p = str(tmp_path / "emb.pt")
    run_cli("train", "--model", "embed", "--epochs", "1", "--rows", "200",
            "--device", "cpu", "--no-watchdog", "--save", p)
    args = ("neighbors", "--load", p, "--words", "a0,b1", "--topk", "5",
            "--device", "cpu")
    flat = json.loads(run_cli(*args)[-1])
    out = json.loads(run_cli(*args, "--index", "forest", "--trees", "2",
                             "--leaf-size", "2", "--search-k", "64")[-1])
    assert out["index"] == "forest"
    for w, hits in flat["neighbors"].items():  # search_k covers all rows
        got = out["neighbors"][w]
        assert [n for n, _ in got] == [n for n, _ in hits]
        assert all(abs(a - b) <= 2e-6 for (_, a), (_, b) in zip(got, hits))


def test_bench_rp_forest_cpu_smoke():
    r = subprocess.run([sys.executable,
                        str(REPO / "tools" / "bench_rp_forest.py"),
                        "--device", "cpu", "--small"], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.strip().splitlines()]
    search = [x for x in rows if x["path"] == "forest"]
    assert {x["nq"] for x in search} == {1, 64}
    assert all(x["outputs_match"] for x in search)
    assert all(0.0 <= x["recall"] <= 1.0 for x in search)
    assert any(x["path"] == "build" for x in rows)


# ---------------------------------------------------------------------------
# recall on clustered float data (seeded, CPU only)
# ---------------------------------------------------------------------------
def test_recall_on_clustered_data():
    X, Q = fo.clustered()
    ix = ForestIndex.build(X, n_trees=8, leaf_size=16, seed=0)
    truth, _ = FlatIndex(X).search(Q, 10)
    r = fo.recall(ix.search(Q, 10, search_k=640)[0], truth)
    print(f"RECALL forest search_k=640 {r:.4f}")
    assert r >= 0.9
    # the CPU path is deterministic
    assert torch.equal(ix.candidates(Q, 640), ix.candidates(Q, 640))
    # the re-rank of everything is the exact search
    big = min(ix.total, FOREST_MAX_SEARCH)
    assert_same(ix.search(Q[:4], 10, search_k=big),
                FlatIndex(X).search(Q[:4], 10))
