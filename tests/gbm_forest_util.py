"""Shared builders for the compiled-forest tests (CPU and GPU files):
synthetic Tree objects in GBMModel._emit order, a GBMModel that holds
them, and the leaf oracle (a copy of GBMModel._route that returns the
node instead of its value)."""

import torch

from lightctr_amd.models.gbm import NAN_BIN, GBMHyper, GBMModel, Tree


def _pack(feature, thr, nanl, left, right, value):
    return Tree(torch.tensor(feature, dtype=torch.int32),
                torch.tensor(thr, dtype=torch.int32),
                torch.tensor(nanl, dtype=torch.bool),
                torch.tensor(left, dtype=torch.int32),
                torch.tensor(right, dtype=torch.int32),
                torch.tensor(value, dtype=torch.float32))


def tree_with_nodes(g, D, n_nodes, max_depth):
    """Random tree with exactly n_nodes (odd) nodes, no deeper than
    max_depth: split a random open leaf until the count is reached."""
    assert n_nodes % 2 == 1
    feature, thr, nanl, left, right = [-1], [0], [False], [-1], [-1]
    depth = [0]
    open_leaves = [0] if max_depth > 0 else []
    while len(feature) < n_nodes:
        assert open_leaves, "max_depth too small for n_nodes"
        j = int(torch.randint(0, len(open_leaves), (1,), generator=g))
        i = open_leaves.pop(j)
        feature[i] = int(torch.randint(0, D, (1,), generator=g))
        thr[i] = int(torch.randint(0, 255, (1,), generator=g))
        nanl[i] = bool(torch.rand(1, generator=g) < 0.5)
        for side in (left, right):
            side[i] = len(feature)
            feature.append(-1)
            thr.append(0)
            nanl.append(False)
            left.append(-1)
            right.append(-1)
            depth.append(depth[i] + 1)
            if depth[-1] < max_depth:
                open_leaves.append(len(feature) - 1)
    value = torch.randn(len(feature), generator=g)
    value[torch.tensor(feature) >= 0] = 0.0
    return _pack(feature, thr, nanl, left, right, value.tolist())


def random_tree(g, D, max_depth, p_leaf=0.25):
    """Random shape to max_depth with early leaves."""
    feature, thr, nanl, left, right, value = [], [], [], [], [], []

    def emit():
        feature.append(-1)
        thr.append(0)
        nanl.append(False)
        left.append(-1)
        right.append(-1)
        value.append(0.0)
        return len(feature) - 1

    todo = [(emit(), 0)]
    while todo:
        i, d = todo.pop(0)
        early = d > 0 and bool(torch.rand(1, generator=g) < p_leaf)
        if d == max_depth or early:
            value[i] = float(torch.randn(1, generator=g))
            continue
        feature[i] = int(torch.randint(0, D, (1,), generator=g))
        thr[i] = int(torch.randint(0, 255, (1,), generator=g))
        nanl[i] = bool(torch.rand(1, generator=g) < 0.5)
        left[i], right[i] = emit(), emit()
        todo += [(left[i], d + 1), (right[i], d + 1)]
    return _pack(feature, thr, nanl, left, right, value)


def forest_sizes(total, cap=127):
    """Odd tree sizes <= cap that sum to exactly `total`."""
    k = -(-total // cap)
    if k % 2 != total % 2:
        k += 1
    sizes = [1] * k
    rem = total - k
    for i in range(k):
        add = min(cap - 1, rem)
        sizes[i] += add
        rem -= add
    assert rem == 0 and sum(sizes) == total
    return sizes


def make_model(trees, X, K=1, n_bins=255, max_depth=6):
    """CPU GBMModel holding `trees` (flat, [round][class] order) with
    bin edges fitted on X."""
    assert len(trees) % K == 0
    m = GBMModel(GBMHyper(n_bins=n_bins, n_classes=2 if K == 1 else K,
                          max_depth=max_depth), device="cpu")
    m._fit_bins(X)
    m.trees = [trees[i:i + K] for i in range(0, len(trees), K)]
    return m


def make_X(g, N, D, special=False):
    X = torch.randn(N, D, generator=g)
    if special and N > 0:
        X[torch.rand(N, D, generator=g) < 0.10] = float("nan")
        X[:, 0] = X[:, 0].round()  # heavy ties -> repeated edges
        if D >= 3:
            X[:, D - 2] = 1.5  # constant column
            X[:, D - 1] = float("nan")  # all-NaN column
    return X


def put_edge_values(g, X, edges, frac=0.1):
    """Overwrite a fraction of cells with exact bin-edge values and 2%
    each with +inf / -inf. Done after the bins are fitted: quantiles of a
    column that holds infinities interpolate to NaN edges."""
    N, D = X.shape
    pick = torch.randint(0, edges.shape[1], (N, D), generator=g)
    ev = edges.cpu().gather(1, pick.t()).t()
    mask = torch.rand(N, D, generator=g) < frac
    # the constant and the all-NaN column stay as they are
    frozen = (torch.isnan(X).all(0) | (X == X[0]).all(0)).unsqueeze(0)
    mask &= ~frozen
    X = torch.where(mask, ev, X)
    for v in (float("inf"), float("-inf")):
        X = torch.where((torch.rand(N, D, generator=g) < 0.02) & ~frozen,
                        torch.full_like(X, v), X)
    return X


def leaf_oracle(model, X):
    """GBMModel._route's loop, returning the node: [N, T] int32."""
    bins = model._binize(X)
    N = bins.shape[0]
    cols = []
    for rt in model.trees:
        for tree in rt:
            node = torch.zeros(N, dtype=torch.long)
            feat = tree.feature.long()
            lft, rgt = tree.left.long(), tree.right.long()
            for _ in range(model.h.max_depth + 1):
                is_leaf = feat[node] < 0
                f = feat[node].clamp(min=0)
                b = bins[torch.arange(N), f].int()
                go_left = torch.where(b == NAN_BIN, tree.nan_left[node],
                                      b <= tree.threshold[node])
                nxt = torch.where(go_left, lft[node], rgt[node])
                node = torch.where(is_leaf, node, nxt)
            cols.append(node.to(torch.int32))
    if not cols:
        return torch.zeros(N, 0, dtype=torch.int32)
    return torch.stack(cols, dim=1)


def stacking_data(n, seed):
    """8 columns, label (x0*x1>0) xor (x2>0.5), 10% labels flipped, 10%
    NaN cells."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 8, generator=g)
    y = ((X[:, 0] * X[:, 1] > 0) ^ (X[:, 2] > 0.5))
    flip = torch.rand(n, generator=g) < 0.10
    y = (y ^ flip).float()
    X[torch.rand(n, 8, generator=g) < 0.10] = float("nan")
    return X, y
