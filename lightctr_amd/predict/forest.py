"""Compiled-forest GBM inference: margins, leaf ids and leaf features.

GBMModel stores each split as a bin id ("go left if bin <= thr") over
per-feature quantile edges. For a non-NaN fp32 value v,
``bucketize(v, edges) <= thr`` is exactly ``v <= edges[thr]``, and
``thr >= len(edges)`` is always-left (threshold +inf); NaN follows
``nan_left``. So a trained forest compiles once to float thresholds and
inference needs no binning pass: one HIP kernel
(ops/csrc/gbm_kernels.hip, gbm_forest_kernel) reads X directly, walks
every tree for a row in one thread and sums leaf values in tree order, so
margins are bit-identical to GBMModel.predict_margin.

Beyond margins it returns the leaf each row lands in, which is what the
reference README's GBDT+LR recipe needs (each leaf is a 0/1 feature for a
downstream LR): ``transform`` emits the CSR that LRModel / FMModel /
FFMModel consume.

The CPU path is the same float-threshold walk in vectorised torch.
"""

from __future__ import annotations

from collections import namedtuple

import torch

from ..ops._extension import require_hip_ops

# nodes per LDS chunk of the kernel (GBF_CAP in gbm_kernels.hip; the
# extension exports it and the GPU path checks the two agree)
CHUNK_CAPACITY = 3072

LeafFeatures = namedtuple("LeafFeatures", ["row_ptr", "fids", "vals",
                                           "fields"])

_MARGIN, _LEAF, _FID = 0, 1, 2
_NAN_LEFT_BIT = -(1 << 31)


def _compile_tree(tree, edges: torch.Tensor, D: int, t: int):
    """One Tree -> ([n,4] int32 records, n_leaves, depth). Raises
    ValueError on anything that would make the walk unsafe."""
    feat = tree.feature.detach().cpu().to(torch.int64)
    n = feat.numel()
    if n == 0:
        raise ValueError(f"tree {t}: no nodes")
    thr = tree.threshold.detach().cpu().to(torch.int64)
    nanl = tree.nan_left.detach().cpu().to(torch.bool)
    left = tree.left.detach().cpu().to(torch.int64)
    right = tree.right.detach().cpu().to(torch.int64)
    value = tree.value.detach().cpu().to(torch.float32)
    for name, a in (("threshold", thr), ("nan_left", nanl), ("left", left),
                    ("right", right), ("value", value)):
        if a.numel() != n:
            raise ValueError(f"tree {t}: {name} has {a.numel()} entries, "
                             f"feature has {n}")
    leaf = feat < 0
    internal = ~leaf
    if bool((feat[leaf] != -1).any()):
        raise ValueError(f"tree {t}: leaves must have feature == -1")
    if bool((feat[internal] >= D).any()):
        raise ValueError(f"tree {t}: split feature out of range [0, {D})")
    if not bool(torch.isfinite(value[leaf]).all()):
        raise ValueError(f"tree {t}: non-finite leaf value")
    ids = torch.arange(n)
    for name, ch in (("left", left), ("right", right)):
        c = ch[internal]
        if bool((c >= n).any()):
            raise ValueError(f"tree {t}: {name} child index out of range")
        # children after their parent (the order GBMModel._emit produces)
        # rules out cycles, so the walk is finite
        if bool((c <= ids[internal]).any()):
            raise ValueError(f"tree {t}: {name} child index must be greater "
                             f"than its parent's")
    if bool((thr[internal] < 0).any()):
        raise ValueError(f"tree {t}: negative split bin")

    E = edges.shape[1] if edges.dim() == 2 else 0
    thr_f = torch.full((n,), float("inf"), dtype=torch.float32)
    finite = internal & (thr < E)
    if bool(finite.any()):
        thr_f[finite] = edges[feat[finite], thr[finite]]
        # quantile edges of a column holding infinities can be NaN; such
        # edges are unsorted and the bin test means nothing
        if bool(torch.isnan(thr_f).any()):
            raise ValueError(f"tree {t}: split on a NaN bin edge")
    x = torch.where(leaf, value, thr_f).view(torch.int32)
    ordinal = torch.cumsum(leaf.to(torch.int64), 0) - 1
    z = torch.where(leaf, ordinal, left)
    w = torch.where(leaf, torch.zeros_like(right), right)
    w = torch.where(internal & nanl, w + _NAN_LEFT_BIT, w)
    rec = torch.stack([x, feat.to(torch.int32), z.to(torch.int32),
                       w.to(torch.int32)], dim=1)

    # measured depth: parents precede children, one forward sweep
    depth = [0] * n
    fl, ll, rl = feat.tolist(), left.tolist(), right.tolist()
    for i in range(n):
        if fl[i] >= 0:
            d = depth[i] + 1
            if depth[ll[i]] < d:
                depth[ll[i]] = d
            if depth[rl[i]] < d:
                depth[rl[i]] = d
    return rec, int(leaf.sum()), max(depth)


def _chunk_table(tree_off: list[int], capacity: int) -> torch.Tensor:
    """Greedy chunks of consecutive whole trees with at most ``capacity``
    nodes: rows of {first tree, n trees, first node, fits flag}. A tree
    larger than the capacity is a chunk of its own with flag 0."""
    rows = []
    T = len(tree_off) - 1
    t = 0
    while t < T:
        size = tree_off[t + 1] - tree_off[t]
        if size > capacity:
            rows.append([t, 1, tree_off[t], 0])
            t += 1
            continue
        e = t + 1
        while e < T and tree_off[e + 1] - tree_off[t] <= capacity:
            e += 1
        rows.append([t, e - t, tree_off[t], 1])
        t = e
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)


class CompiledForest:
    """A GBM forest packed for inference. Build with ``from_model`` or
    ``load``; the source model is not referenced afterwards."""

    def __init__(self, trees, bin_edges, n_features: int, n_classes: int,
                 device=None):
        self.device = torch.device(device if device is not None else "cpu")
        self.n_features = int(n_features)
        self.n_classes = 1 if n_classes <= 2 else int(n_classes)
        K = self.n_classes
        flat = [t for round_trees in trees for t in round_trees]
        for round_trees in trees:
            if len(round_trees) != K:
                raise ValueError(f"every round needs {K} trees, got "
                                 f"{len(round_trees)}")
        if self.n_features < 1:
            raise ValueError("n_features must be >= 1")
        edges = (torch.zeros(self.n_features, 0) if bin_edges is None
                 else bin_edges.detach().cpu().to(torch.float32))
        if flat and (edges.dim() != 2 or edges.shape[0] != self.n_features):
            raise ValueError("bin_edges must be [n_features, n_bins - 1]")

        recs, tree_off, leaf_base, depth = [], [0], [], 0
        n_leaves = 0
        for t, tree in enumerate(flat):
            rec, nl, d = _compile_tree(tree, edges, self.n_features, t)
            recs.append(rec)
            tree_off.append(tree_off[-1] + rec.shape[0])
            leaf_base.append(n_leaves)
            n_leaves += nl
            depth = max(depth, d)
        if tree_off[-1] >= (1 << 31) - 1 or n_leaves >= (1 << 31) - 1:
            raise ValueError("forest too large for int32 indices")
        self.n_trees = len(flat)
        self.n_leaves = n_leaves
        self.max_depth = depth
        dev = self.device
        self.nodes = (torch.cat(recs) if recs else
                      torch.zeros(0, 4, dtype=torch.int32)).contiguous().to(dev)
        self.tree_off = torch.tensor(tree_off, dtype=torch.int32).to(dev)
        self.tree_class = (torch.arange(self.n_trees, dtype=torch.int32)
                           % K).to(dev)
        self.leaf_base = torch.tensor(leaf_base, dtype=torch.int32).to(dev)
        self.chunks = _chunk_table(tree_off, CHUNK_CAPACITY).to(dev)
        self._gpu = dev.type == "cuda"
        if self._gpu:
            ops = require_hip_ops()  # fail loudly if extension missing
            if ops.gbm_forest_chunk_capacity() != CHUNK_CAPACITY:
                raise RuntimeError("forest kernel chunk capacity disagrees "
                                   "with predict/forest.py")
        else:
            # CPU walk tables (global child indices)
            n = self.nodes
            off = torch.repeat_interleave(
                self.tree_off[:-1].long(),
                (self.tree_off[1:] - self.tree_off[:-1]).long())
            self._feat = n[:, 1].long()
            self._x = n[:, 0].contiguous().view(torch.float32)
            self._nanl = n[:, 3] < 0
            self._left = n[:, 2].long() + off
            self._right = (n[:, 3] & 0x7FFFFFFF).long() + off
            self._ordinal = n[:, 2].long()

    # ---- constructors ----
    @classmethod
    def from_model(cls, gbm, device=None) -> "CompiledForest":
        if gbm.bin_edges is None:
            if gbm.trees:
                raise ValueError("model has trees but no bin_edges")
            raise ValueError("model is not fitted (no bin_edges)")
        return cls(gbm.trees, gbm.bin_edges, gbm.bin_edges.shape[0],
                   gbm.h.n_classes,
                   device=gbm.device if device is None else device)

    @classmethod
    def load(cls, path: str, device="cpu") -> "CompiledForest":
        """Reads a file written by GBMModel.save."""
        from ..models.gbm import Tree

        d = torch.load(path, map_location="cpu", weights_only=False)
        trees = [[Tree(**td) for td in rt] for rt in d["trees"]]
        return cls(trees, d["bin_edges"], d["bin_edges"].shape[0],
                   d["hyper"]["n_classes"], device=device)

    # ---- inference ----
    def _check(self, X: torch.Tensor) -> torch.Tensor:
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            raise ValueError("X must be a 2-D tensor")
        if X.dtype != torch.float32:
            raise ValueError(f"X must be float32, got {X.dtype}")
        if X.shape[1] != self.n_features:
            raise ValueError(f"X has {X.shape[1]} columns, forest expects "
                             f"{self.n_features}")
        return X.to(self.device).contiguous()

    def _run_gpu(self, X, mode: int, fid_offset: int = 0):
        return require_hip_ops().gbm_forest(
            X, self.nodes, self.tree_off, self.tree_class, self.leaf_base,
            self.chunks, mode, self.n_features, self.n_classes,
            self.max_depth, fid_offset)

    def _walk_cpu(self, X) -> torch.Tensor:
        """Global leaf-node index per (row, tree), [N, T] int64."""
        N = X.shape[0]
        node = self.tree_off[:-1].long().unsqueeze(0).repeat(N, 1)
        rows = torch.arange(N).unsqueeze(1)
        for _ in range(self.max_depth):
            f = self._feat[node]
            is_leaf = f < 0
            v = X[rows, f.clamp(min=0)]
            go_left = torch.where(torch.isnan(v), self._nanl[node],
                                  v <= self._x[node])
            nxt = torch.where(go_left, self._left[node], self._right[node])
            node = torch.where(is_leaf, node, nxt)
        return node

    def predict_margin(self, X: torch.Tensor) -> torch.Tensor:
        X = self._check(X)
        N, K = X.shape[0], self.n_classes
        if N == 0 or self.n_trees == 0:
            return torch.zeros(N, K, device=self.device)
        if self._gpu:
            return self._run_gpu(X, _MARGIN)
        vals = self._x[self._walk_cpu(X)]  # [N, T]
        out = torch.zeros(N, K)
        for t in range(self.n_trees):  # tree order == GBMModel's sum order
            out[:, t % K] += vals[:, t]
        return out

    def predict_proba(self, X: torch.Tensor) -> torch.Tensor:
        m = self.predict_margin(X)
        if m.shape[1] == 1:
            return torch.sigmoid(m[:, 0])
        return torch.softmax(m, dim=1)

    def predict_leaf(self, X: torch.Tensor) -> torch.Tensor:
        """[N, T] int32 tree-local node id of the leaf each row lands in."""
        X = self._check(X)
        N, T = X.shape[0], self.n_trees
        if N == 0 or T == 0:
            return torch.zeros(N, T, dtype=torch.int32, device=self.device)
        if self._gpu:
            return self._run_gpu(X, _LEAF)
        return (self._walk_cpu(X)
                - self.tree_off[:-1].long().unsqueeze(0)).to(torch.int32)

    def transform(self, X: torch.Tensor, fid_offset: int = 0) -> LeafFeatures:
        """Leaf-membership features as CSR: row r holds one feature per
        tree, ``fid_offset + leaf_base[t] + ordinal of the leaf in t``,
        value 1, field = tree index."""
        X = self._check(X)
        N, T = X.shape[0], self.n_trees
        if fid_offset < 0 or fid_offset + self.n_leaves >= (1 << 31):
            raise ValueError("fid_offset out of int32 range")
        dev = self.device
        if N == 0 or T == 0:
            fids = torch.zeros(N * T, dtype=torch.int32, device=dev)
        elif self._gpu:
            fids = self._run_gpu(X, _FID, int(fid_offset)).view(-1)
        else:
            fids = (self._ordinal[self._walk_cpu(X)]
                    + self.leaf_base.long().unsqueeze(0)
                    + int(fid_offset)).to(torch.int32).view(-1)
        row_ptr = torch.arange(0, N * T + 1, max(T, 1), dtype=torch.int32,
                               device=dev) if T > 0 else \
            torch.zeros(N + 1, dtype=torch.int32, device=dev)
        fields = torch.arange(T, dtype=torch.int32, device=dev).repeat(N)
        vals = torch.ones(N * T, device=dev)
        return LeafFeatures(row_ptr, fids, vals, fields)
