"""Oracle, exact-input forests and shared cases of the random-projection
forest tests (``test_forest.py`` on the CPU, ``test_forest_gpu.py`` on the
GPU).

Plain helper module, imported like ``knn_oracles.py``. Everything here runs
on the CPU and is written from the search contract in
``lightctr_amd/predict/rp_forest.py``, not from the project's code paths:

* the walk works per query on a plain sorted list (no ``heapq``) with an
  explicit (bound, code) comparison, and drops the last entry when the list
  outgrows the queue bound;
* margins are float64 dot products plus the bias.

Exact-input rule (extends ``knn_oracles``): X, Q and planes are integers in
{-3..3} and biases are multiples of 0.5, so every product (at most 9) and
partial sum is a multiple of 0.5 below 2^23 and exact in fp32 in any order
while ``dim * 9 < 2^23``. The float64 margin is then what any correct fp32
evaluation gives, and the walk must be equal on every device. (The chain
forest holds coordinates up to 1300 in dim 2; its margins are multiples of
0.5 below 2^12 and as exact.)

Forests of the exact set are generated here, never by ``ForestIndex.build``:
recursive splits on random integer planes, the bias set from the member
margins so that both sides are non-empty and, for half of the nodes, some
member margins are exactly 0 (they go to ``child[i, 1]``).
"""

from __future__ import annotations

import functools

import numpy as np
import torch

import knn_oracles as ko

QUEUE = 1024
MAX_SEARCH = 65536
INF = float("inf")

BASE_SEARCH_K = 40  # around N = 257, dim 16, T = 4, leaf 8, nq = 3


def assert_exact(dim):
    assert dim * 9 < 2 ** 23, "exact-input rule violated"


# ---------------------------------------------------------------------------
# exact-input forests
# ---------------------------------------------------------------------------
class Forest:
    """The arrays of the flattened layout plus X (all CPU tensors)."""

    FIELDS = ("planes", "bias", "child", "roots", "leaf_off", "leaf_items")

    def __init__(self, X, planes, bias, child, roots, leaves):
        dim = X.shape[1]
        self.X = X
        self.planes = (torch.tensor(np.array(planes), dtype=torch.float32)
                       if planes else torch.zeros(0, dim))
        self.bias = torch.tensor(bias, dtype=torch.float32)
        self.child = torch.tensor(child, dtype=torch.int32).reshape(-1, 2)
        self.roots = torch.tensor(roots, dtype=torch.int32)
        off = np.cumsum([0] + [len(l) for l in leaves])
        self.leaf_off = torch.tensor(off, dtype=torch.int32)
        self.leaf_items = torch.tensor(
            [i for l in leaves for i in l], dtype=torch.int32)
        self.max_leaf = max(len(l) for l in leaves)
        self.total = int(off[-1])

    def arrays(self, device="cpu"):
        return [getattr(self, f).to(device) for f in self.FIELDS]

    def width(self, search_k):
        return search_k + max(self.max_leaf, 1) - 1


def grow(X, T, leaf, seed, single_leaf_trees=0, zero_root=False):
    """T trees over all rows of X split recursively on random integer
    planes, numbered in pre-order (parent before children), then
    ``single_leaf_trees`` trees that are one leaf of all rows. With
    ``zero_root`` the root bias of tree 0 is minus a member margin, so that
    member as a query has margin exactly 0 there."""
    rng = np.random.default_rng(seed)
    Xn = X.numpy().astype(np.int64)
    planes, bias, child, roots, leaves = [], [], [], [], []

    def build(items, force_zero):
        if len(items) > leaf:
            for _ in range(8):  # a plane that separates the members
                w = rng.integers(-3, 4, Xn.shape[1])
                mg = Xn[items] @ w
                vals = np.unique(mg)
                if len(vals) > 1:
                    break
            if len(vals) > 1:
                v = int(vals[rng.integers(0, len(vals) - 1)])  # not the max
                # b = -v: members at v have margin 0 (right side);
                # b = -(v + 0.5): no member on the plane
                b = -float(v) if force_zero or rng.integers(0, 2) else \
                    -(v + 0.5)
                i = len(planes)
                planes.append(w.astype(np.float32))
                bias.append(b)
                child.append([0, 0])
                left = mg + b > 0
                child[i][0] = build(items[left], False)
                child[i][1] = build(items[~left], False)
                return i
        leaves.append(items.tolist())  # small, or unsplittable
        return -len(leaves)

    for t in range(T):
        roots.append(build(np.arange(len(Xn)), zero_root and t == 0))
    for _ in range(single_leaf_trees):
        leaves.append(list(range(len(Xn))))
        roots.append(-len(leaves))
    return Forest(X, planes, bias, child, roots, leaves)


def chain():
    """1200 points (i, 0); node j has plane (1, 0), bias -(j + 0.5), the
    next node on the left and leaf {j} on the right."""
    N = 1200
    X = torch.zeros(N, 2)
    X[:, 0] = torch.arange(N).float()
    n_inner = N - 1
    planes = [np.array([1.0, 0.0], dtype=np.float32)] * n_inner
    bias = [-(j + 0.5) for j in range(n_inner)]
    child = [[j + 1, -1 - j] for j in range(n_inner)]
    child[-1][0] = -1 - (N - 1)
    return Forest(X, planes, bias, child, [0], [[j] for j in range(N)])


def many_roots(T=1030):
    """T trees of one split each over 64 rows: more roots than the queue
    holds."""
    X = ko.ints((64, 8), 300)
    rng = np.random.default_rng(301)
    Xn = X.numpy().astype(np.int64)
    planes, bias, child, roots, leaves = [], [], [], [], []
    while len(roots) < T:
        w = rng.integers(-3, 4, 8)
        mg = Xn @ w
        vals = np.unique(mg)
        if len(vals) < 2:
            continue
        b = -(int(vals[len(vals) // 2 - 1]) + 0.5)
        left = mg + b > 0
        i = len(planes)
        planes.append(w.astype(np.float32))
        bias.append(b)
        leaves.append(np.nonzero(left)[0].tolist())
        leaves.append(np.nonzero(~left)[0].tolist())
        child.append([-len(leaves) + 1, -len(leaves)])
        roots.append(i)
    return Forest(X, planes, bias, child, roots, leaves)


# ---------------------------------------------------------------------------
# the contract's walk
# ---------------------------------------------------------------------------
def _before(a, b, tie_low=True):
    """entry a = (bound, code) comes before b in queue order"""
    if a[0] > b[0]:
        return True
    if a[0] < b[0]:
        return False
    return a[1] < b[1] if tie_low else a[1] > b[1]


def walk(f, q, search_k, queue=QUEUE, tie_low=True):
    """(ids written, running totals after each leaf, longest queue) of one
    query; ``queue=None`` is the wrong, unbounded walk and ``tie_low=False``
    the wrong tie rule."""
    planes = f.planes.double().numpy()
    bias = f.bias.double().numpy()
    child = f.child.tolist()
    off = f.leaf_off.tolist()
    items = f.leaf_items.tolist()
    q = q.double().numpy()
    entries = []

    def push(e):
        lo, hi = 0, len(entries)
        while lo < hi:  # first position whose entry does not come before e
            mid = (lo + hi) // 2
            if _before(entries[mid], e, tie_low):
                lo = mid + 1
            else:
                hi = mid
        entries.insert(lo, e)
        if queue is not None and len(entries) > queue:
            entries.pop()

    for c in f.roots.tolist():
        push((INF, c))
    out, totals, longest = [], [], len(entries)
    while entries and len(out) < search_k:
        b, code = entries.pop(0)
        if code < 0:
            l = -1 - code
            out.extend(items[off[l]:off[l + 1]])
            totals.append(len(out))
            continue
        m = float(planes[code] @ q + bias[code])
        near, far = child[code] if m > 0 else child[code][::-1]
        push((min(b, abs(m)), near))
        push((min(b, -abs(m)), far))
        longest = max(longest, len(entries))
    return out, totals, longest


def candidates(f, Q, search_k, queue=QUEUE):
    """int32 [nq, R] of the contract."""
    out = torch.full((Q.shape[0], f.width(search_k)), -1, dtype=torch.int32)
    for i in range(Q.shape[0]):
        ids, _, _ = walk(f, Q[i], search_k, queue)
        out[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return out


def search(f, Q, k, search_k, metric):
    """(ids, dist) of the contract: the float64 re-rank of the oracle's
    candidates (duplicates once, -1 skipped)."""
    return ko.flat_ref(f.X, Q, metric, k, cand=candidates(f, Q, search_k))


# ---------------------------------------------------------------------------
# the exact set: (forest, Q, search_k) by name, built once
# ---------------------------------------------------------------------------
def _grown(N=257, dim=16, T=4, leaf=8, nq=3, seed=0, **kw):
    assert_exact(dim)
    X = ko.ints((N, dim), 1000 + seed)
    return grow(X, T, leaf, 2000 + seed, **kw), ko.ints((nq, dim),
                                                         3000 + seed)


def _case(name):
    kind, _, arg = name.partition("=")
    sk = BASE_SEARCH_K
    if kind == "base":
        f, Q = _grown()
    elif kind in ("dim", "nq", "T"):
        f, Q = _grown(seed=int(arg) + 7, **{kind: int(arg)})
    elif kind == "search_k":
        f, Q = _grown()
        if arg == "leaf_total":  # query 0 stops with nothing left over
            sk = walk(f, Q[0], f.total)[1][2]
        else:
            sk = {"1": 1, "40": 40, "total": f.total,
                  "total+1": f.total + 1}[arg]
    elif kind == "single_leaf_tree":
        f, Q = _grown(seed=11, single_leaf_trees=1)
        assert int(f.roots[-1]) < 0
        sk = 300
    elif kind == "only_single_leaves":
        f, Q = _grown(N=5, T=3, seed=12)
        assert f.planes.shape[0] == 0 and bool((f.roots < 0).all())
    elif kind == "leaf_len_1":
        f, Q = _grown(leaf=1, seed=13)
        assert int((f.leaf_off[1:] - f.leaf_off[:-1]).min()) == 1
    elif kind == "long_leaf":
        X = ko.ints((257, 16), 1014)
        X[40:70] = X[40]  # 30 equal rows cannot be split
        f, Q = grow(X, 4, 8, 2014), ko.ints((3, 16), 3014)
        assert f.max_leaf >= 30
    elif kind == "zero_margin_root":
        f, Q = _grown(seed=15, zero_root=True)
        mg = f.X.double() @ f.planes[0].double() + float(f.bias[0])
        Q[0] = f.X[int((mg == 0).nonzero()[0])]  # a member on the plane
        assert float(Q[0].double() @ f.planes[0].double()
                     + float(f.bias[0])) == 0.0
        sk = f.total
    elif kind == "chain_far":
        f, Q, sk = chain(), torch.tensor([[1300.0, 0.0]]), 1200
    elif kind == "chain_near":
        f, Q, sk = chain(), torch.tensor([[-5.0, 0.0]]), 1200
    elif kind == "many_roots":
        f, Q, sk = many_roots(), ko.ints((2, 8), 302), int(arg)
    else:
        raise KeyError(name)
    return f, Q, int(sk)


@functools.lru_cache(maxsize=None)
def case(name):
    """(forest, Q, search_k); shared, do not modify."""
    return _case(name)


@functools.lru_cache(maxsize=None)
def case_candidates(name):
    """the oracle's candidate lists of a case; shared, do not modify."""
    f, Q, sk = case(name)
    return candidates(f, Q, sk)


EXACT_CASES = (
    ["base"]
    + [f"dim={d}" for d in (1, 3, 63, 64, 65, 128, 1024)]
    + [f"nq={n}" for n in (1, 4, 5, 64, 65)]
    + [f"T={t}" for t in (1, 2, 8)]
    + [f"search_k={s}" for s in ("1", "leaf_total", "40", "total",
                                 "total+1")]
    + ["single_leaf_tree", "only_single_leaves", "leaf_len_1", "long_leaf",
       "zero_margin_root", "chain_far", "chain_near", "many_roots=4000",
       "many_roots=65536"])


# ---------------------------------------------------------------------------
# float data
# ---------------------------------------------------------------------------
def clustered(N=4096, dim=32, n_clusters=32, nq=64, seed=0):
    """(X, Q): Gaussian clusters of spread 3 with unit noise; the queries
    are data rows plus noise of 0.1."""
    g = torch.Generator().manual_seed(seed)
    centres = 3.0 * torch.randn(n_clusters, dim, generator=g)
    X = centres[torch.randint(0, n_clusters, (N,), generator=g)] + \
        torch.randn(N, dim, generator=g)
    rows = torch.randperm(N, generator=g)[:nq]
    Q = X[rows] + 0.1 * torch.randn(nq, dim, generator=g)
    return X.contiguous(), Q.contiguous()


def recall(ids, truth):
    """mean fraction of the true ids among the returned ones"""
    hit = 0
    for a, b in zip(ids.tolist(), truth.tolist()):
        hit += len(set(a) & set(b))
    return hit / truth.numel()
