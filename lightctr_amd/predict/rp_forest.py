"""Batched random-projection forest search (ForestIndex): the candidate
generator in front of ``FlatIndex.search(Q, k, cand=...)``.

The flattened forest. All arrays live on the index's device:

* ``planes`` float32 [n_inner, dim], ``bias`` float32 [n_inner]: the
  splitting hyperplane of every inner node;
* ``child`` int32 [n_inner, 2], ``roots`` int32 [T]: node codes. A code is
  an inner-node index ``i >= 0`` or ``-1 - l`` for leaf ``l``; indices are
  global over the whole forest. ``child[i, 0]`` is the side ``margin > 0``
  ("left" in ``ANNIndex._build``), ``child[i, 1]`` the other side, which
  includes ``margin == 0``. A tree that is a single leaf has a negative
  root code;
* ``leaf_off`` int32 [n_leaves + 1], ``leaf_items`` int32 [total]: leaf l
  holds ``leaf_items[leaf_off[l]:leaf_off[l + 1]]``, row ids in [0, N).

The constructor checks the structure once (ValueError): dtypes and shapes,
``T >= 1``, ``1 <= dim <= KNN_MAX_DIM``, finite planes and biases, every
inner child code ``c >= 0`` of node i obeys ``c > i`` (a topological layout:
no cycles, every walk ends), leaf codes in range, no code listed twice
among the roots and children (the forest is a set of trees), ``leaf_off``
non-decreasing from 0 to ``total``, items in [0, N).

Search contract, the same on CPU and GPU. ``candidates(Q, search_k)``
returns int32 [nq, R], ``R = search_k + max(max_leaf, 1) - 1``, for
``1 <= search_k <= FOREST_MAX_SEARCH``. Per query, independently:

* a priority queue holds (bound, code) entries; larger bound first, floats
  compared by ``<`` (-0 and +0 tie), ties to the lower code as a signed
  int. Codes are unique, so the order is;
* it starts with every root at bound +inf, pushed in tree order;
* while it is non-empty and fewer than ``search_k`` ids are written, the
  first entry is popped. A leaf appends all its items in stored order. An
  inner node i with bound b computes ``m = sum_j planes[i, j] * q[j]``
  (fp32, any order) ``+ bias[i]`` (added last); the near child
  (``child[i, 0]`` if ``m > 0`` else ``child[i, 1]``) is pushed with
  ``min(b, |m|)`` and the far child with ``min(b, -|m|)``;
* the queue holds at most ``FOREST_QUEUE`` entries: a push into a full
  queue discards whichever of the FOREST_QUEUE + 1 entries is last in
  queue order (possibly the pushed one);
* slots after the last written id are -1.

The walk uses compares, min, abs and the margin only, so where every margin
is exact in fp32 the list is bit-identical on every device.

``search(Q, k, search_k=None)`` is ``flat.search(Q, k, cand=candidates(Q,
search_k))`` with ``flat = FlatIndex(X, metric)``, so the result obeys the
whole result contract of predict/knn.py. ``metric`` affects the re-rank
only: the planes are Euclidean, which ranks like ``ip`` on unit vectors.

The CPU path is plain torch/Python and is the oracle of the GPU tests. On a
CUDA tensor ``candidates`` calls forest_candidates_kernel
(ops/csrc/knn_kernels.hip) through the extension; there is no eager
fallback.
"""

from __future__ import annotations

import heapq

import torch

from ..ops._extension import require_hip_ops
from .knn import KNN_MAX_DIM, FlatIndex, _METRICS, _check_k, _check_q, _finite

# limits of the kernel (knn_kernels.hip exports them; the GPU path checks
# that the two agree)
FOREST_QUEUE = 1024
FOREST_MAX_SEARCH = 65536

_MARGIN_ALL = 1 << 22  # planes elements up to which a query takes one mv
_INF = float("inf")


def _gpu_ops():
    ops = require_hip_ops()
    if (ops.forest_queue(), ops.forest_max_search(), ops.knn_max_dim()) != \
            (FOREST_QUEUE, FOREST_MAX_SEARCH, KNN_MAX_DIM):
        raise RuntimeError("forest kernel limits disagree with "
                           "predict/rp_forest.py")
    return ops


def _check_array(t, name, dtype, ndim):
    if not isinstance(t, torch.Tensor) or t.dim() != ndim:
        raise ValueError(f"{name} must be a {ndim}-D tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")


class ForestIndex:
    """Random-projection forest over ``X`` [N, dim] float32 in the
    flattened layout of the module docstring; ``search`` re-ranks the
    forest's candidates exactly."""

    def __init__(self, X: torch.Tensor, planes: torch.Tensor,
                 bias: torch.Tensor, child: torch.Tensor,
                 roots: torch.Tensor, leaf_off: torch.Tensor,
                 leaf_items: torch.Tensor, metric: str = "l2"):
        self.flat = FlatIndex(X, metric)
        self.X, self.metric = self.flat.X, metric
        self.device, self._gpu = self.flat.device, self.flat._gpu
        self.N, self.dim = self.flat.N, self.flat.dim
        if not 1 <= self.dim <= KNN_MAX_DIM:
            raise ValueError(f"dim must be in [1, {KNN_MAX_DIM}], "
                             f"got {self.dim}")
        _check_array(planes, "planes", torch.float32, 2)
        _check_array(bias, "bias", torch.float32, 1)
        _check_array(child, "child", torch.int32, 2)
        _check_array(roots, "roots", torch.int32, 1)
        _check_array(leaf_off, "leaf_off", torch.int32, 1)
        _check_array(leaf_items, "leaf_items", torch.int32, 1)
        n_inner = planes.shape[0]
        if planes.shape[1] != self.dim:
            raise ValueError(f"planes must be [n_inner, {self.dim}]")
        if bias.shape[0] != n_inner or tuple(child.shape) != (n_inner, 2):
            raise ValueError("bias must be [n_inner], child [n_inner, 2]")
        if roots.numel() < 1:
            raise ValueError("the forest needs at least one tree")
        if leaf_off.numel() < 1:
            raise ValueError("leaf_off must be [n_leaves + 1]")
        n_leaves, total = leaf_off.numel() - 1, leaf_items.numel()
        if max(n_inner, n_leaves + 1, roots.numel(), total) >= 1 << 31:
            raise ValueError("forest arrays must stay below 2^31 entries")
        planes, bias, child, roots, leaf_off, leaf_items = (
            t.to(self.device).contiguous()
            for t in (planes, bias, child, roots, leaf_off, leaf_items))
        _finite(planes, "planes")
        _finite(bias, "bias")
        codes = torch.cat([roots, child.reshape(-1)]).long()
        if bool(((codes >= n_inner) | (codes < -n_leaves)).any()):
            raise ValueError("a node code is out of range")
        own = torch.arange(n_inner, device=self.device)[:, None]
        ch = child.long()
        if bool(((ch >= 0) & (ch <= own)).any()):
            raise ValueError("an inner child code must be above its "
                             "parent's index (topological layout)")
        if torch.unique(codes).numel() != codes.numel():
            raise ValueError("a node code is listed twice: not a forest")
        lo = leaf_off.long()
        if int(lo[0]) != 0 or int(lo[-1]) != total or \
                bool((lo[1:] < lo[:-1]).any()):
            raise ValueError("leaf_off must be non-decreasing from 0 to "
                             "the number of items")
        if total and (int(leaf_items.min()) < 0
                      or int(leaf_items.max()) >= self.N):
            raise ValueError("leaf items must be in [0, N)")
        if self._gpu:
            _gpu_ops()
        self.planes, self.bias, self.child, self.roots = (planes, bias,
                                                          child, roots)
        self.leaf_off, self.leaf_items = leaf_off, leaf_items
        self.n_inner, self.n_leaves, self.total = n_inner, n_leaves, total
        self.n_trees = roots.numel()
        self.max_leaf = int((lo[1:] - lo[:-1]).max()) if n_leaves else 0
        self._host = None

    # ---- search ----
    def width(self, search_k: int) -> int:
        """Columns of ``candidates(Q, search_k)``."""
        return search_k + max(self.max_leaf, 1) - 1

    def candidates(self, Q: torch.Tensor, search_k: int) -> torch.Tensor:
        if not isinstance(search_k, int) or \
                not 1 <= search_k <= FOREST_MAX_SEARCH:
            raise ValueError(f"search_k must be an int in [1, "
                             f"{FOREST_MAX_SEARCH}], got {search_k!r}")
        Q = _check_q(Q, self.dim, self.device)
        R = self.width(search_k)
        if self._gpu:
            return require_hip_ops().forest_candidates(
                self.planes, self.bias, self.child, self.roots,
                self.leaf_off, self.leaf_items, Q, search_k, R)
        return self._candidates_cpu(Q, search_k, R)

    def search(self, Q: torch.Tensor, k: int, search_k: int = None):
        """(ids, dist) of predict/knn.py's contract over the candidates;
        ``search_k`` defaults to ANNIndex's ``k * n_trees * 2``."""
        _check_k(k)
        if search_k is None:
            search_k = k * self.n_trees * 2
        return self.flat.search(Q, k, cand=self.candidates(Q, search_k))

    def _candidates_cpu(self, Q, search_k, R):
        if self._host is None:
            self._host = (self.roots.tolist(), self.child.tolist(),
                          self.leaf_off.tolist())
        roots, child, off = self._host
        nq = Q.shape[0]
        out = torch.full((nq, R), -1, dtype=torch.int32)
        whole = 0 < self.planes.numel() <= _MARGIN_ALL
        for qi in range(nq):
            q = Q[qi]
            margins = (self.planes @ q + self.bias).tolist() if whole \
                else None
            heap = []  # (-bound, code): the first entry is the smallest

            def push(entry):
                if len(heap) < FOREST_QUEUE:
                    heapq.heappush(heap, entry)
                    return
                last = max(heap)
                if entry < last:
                    heap[heap.index(last)] = entry
                    heapq.heapify(heap)

            for c in roots:
                push((-_INF, c))
            n = 0
            while heap and n < search_k:
                nb, code = heapq.heappop(heap)
                if code < 0:
                    a, b = off[-1 - code], off[-code]
                    out[qi, n:n + b - a] = self.leaf_items[a:b]
                    n += b - a
                    continue
                m = margins[code] if whole else float(
                    self.planes[code] @ q + self.bias[code])
                near, far = child[code] if m > 0 else child[code][::-1]
                push((-min(-nb, abs(m)), near))
                push((-min(-nb, -abs(m)), far))
        return out

    # ---- construction ----
    @classmethod
    def from_ann(cls, ann, metric: str = "l2", device=None) -> "ForestIndex":
        """Flattens the trees of an ``ANNIndex`` in pre-order (a parent is
        numbered before its children, so the layout is topological)."""
        X = ann.X if device is None else ann.X.to(device)
        planes, bias, child, roots, leaves = [], [], [], [], []
        for tree in ann.trees:
            stack = [(tree, -1, 0)]
            while stack:
                node, parent, side = stack.pop()
                if node.items is not None:
                    code = -1 - len(leaves)
                    leaves.append(node.items.to(torch.int32).cpu())
                else:
                    code = len(planes)
                    planes.append(node.w.float().cpu())
                    bias.append(float(node.b))
                    child.append([0, 0])
                    stack.append((node.right, code, 1))
                    stack.append((node.left, code, 0))
                if parent < 0:
                    roots.append(code)
                else:
                    child[parent][side] = code
        dim = X.shape[1]
        sizes = torch.tensor([0] + [t.numel() for t in leaves])
        return cls(
            X,
            torch.stack(planes) if planes else torch.zeros(0, dim),
            torch.tensor(bias, dtype=torch.float32),
            torch.tensor(child, dtype=torch.int32).reshape(-1, 2),
            torch.tensor(roots, dtype=torch.int32),
            torch.cumsum(sizes, 0).to(torch.int32),
            torch.cat(leaves) if leaves else torch.zeros(
                0, dtype=torch.int32),
            metric=metric)

    @classmethod
    def build(cls, X: torch.Tensor, n_trees: int = 8, leaf_size: int = 16,
              seed: int = 0, metric: str = "l2",
              device=None) -> "ForestIndex":
        """Level-synchronous builder in torch ops on X's device: per level
        every node above ``leaf_size`` rows is split at once by the 2-means
        hyperplane of ``ANNIndex._build`` (two distinct random member
        seeds, 4 Lloyd iterations with segment sums, ``w = c0 - c1``
        normalised or a random direction where that vanishes,
        ``b = -w.(c0 + c1)/2``, side ``margin > 0``). A node whose split
        leaves a side empty becomes a leaf, whatever its size. Inner nodes
        are numbered level by level, so the layout is topological.

        All random draws come from a CPU generator. The same seed gives
        the same forest on the CPU; on the GPU the segment sums
        (``index_add_``) may be added in another order from run to run, so
        only the invariants are promised there: every row once per tree,
        leaves within ``leaf_size`` unless unsplittable, topological
        codes."""
        if not isinstance(X, torch.Tensor) or X.dim() != 2 \
                or X.dtype != torch.float32:
            raise ValueError("X must be a float32 [N, dim] tensor")
        if n_trees < 1 or leaf_size < 1:
            raise ValueError("n_trees and leaf_size must be >= 1")
        if device is not None:
            X = X.to(device)
        X = X.contiguous()
        _finite(X, "X")
        dev, (N, dim) = X.device, X.shape
        g = torch.Generator().manual_seed(seed)
        planes, bias, roots = [], [], []
        links = []  # (parent inner index, side, code) of every non-root
        leaf_rows, leaf_len = [], []
        n_inner = n_leaves = 0
        for _ in range(n_trees):
            rows = torch.arange(N, device=dev)
            lens = torch.tensor([N], device=dev)
            parent = torch.tensor([-1], device=dev)
            pside = torch.tensor([0], device=dev)
            while lens.numel():
                A = lens.numel()
                node = torch.repeat_interleave(
                    torch.arange(A, device=dev), lens)
                split = torch.zeros(A, dtype=torch.bool, device=dev)
                side = None
                big = lens > leaf_size
                if bool(big.any()):
                    bi = big.nonzero().squeeze(1)
                    w, b = cls._split_planes(X, rows, lens, node, bi, g)
                    # margins of every active row against its node's plane
                    # (rows of small nodes get a zero plane: side False)
                    W = torch.zeros(A, dim, device=dev)
                    B = torch.zeros(A, device=dev)
                    W[bi], B[bi] = w, b
                    side = (X[rows] * W[node]).sum(1) + B[node] > 0
                    n_left = torch.zeros(A, dtype=torch.long, device=dev)
                    n_left.index_add_(0, node, side.long())
                    split = big & (n_left > 0) & (n_left < lens)
                is_leaf = ~split
                code = torch.empty(A, dtype=torch.long, device=dev)
                n_s, n_l = int(split.sum()), int(is_leaf.sum())
                code[split] = n_inner + torch.arange(n_s, device=dev)
                code[is_leaf] = -1 - (n_leaves + torch.arange(n_l,
                                                              device=dev))
                is_root = parent < 0
                roots.append(code[is_root])
                links.append(torch.stack([parent[~is_root],
                                          pside[~is_root],
                                          code[~is_root]], 1))
                row_leaf = is_leaf[node]
                leaf_rows.append(rows[row_leaf])
                leaf_len.append(lens[is_leaf])
                n_leaves += n_l
                if not n_s:
                    break
                planes.append(W[split])
                bias.append(B[split])
                # regroup the rows of split nodes by (node, side), left
                # first; the sort is stable, so ids stay ascending
                keep = ~row_leaf
                key = node[keep] * 2 + (~side[keep]).long()
                order = torch.sort(key, stable=True)[1]
                rows = rows[keep][order]
                nl = n_left[split]
                lens = torch.stack([nl, lens[split] - nl], 1).reshape(-1)
                parent = code[split].repeat_interleave(2)
                pside = torch.tensor([0, 1], device=dev).repeat(n_s)
                n_inner += n_s
        child = torch.zeros(n_inner, 2, dtype=torch.int32, device=dev)
        links = torch.cat(links)
        child[links[:, 0], links[:, 1]] = links[:, 2].to(torch.int32)
        off = torch.zeros(n_leaves + 1, dtype=torch.long, device=dev)
        off[1:] = torch.cumsum(torch.cat(leaf_len), 0)
        return cls(
            X,
            torch.cat(planes) if planes else torch.zeros(0, dim, device=dev),
            torch.cat(bias) if bias else torch.zeros(0, device=dev),
            child, torch.cat(roots).to(torch.int32), off.to(torch.int32),
            torch.cat(leaf_rows).to(torch.int32), metric=metric)

    @staticmethod
    def _split_planes(X, rows, lens, node, bi, g):
        """(w [B, dim], b [B]) of the B nodes ``bi`` of one level; ``rows``
        are grouped by node, ``node`` names each row's node."""
        dev, dim = X.device, X.shape[1]
        A, nb = lens.numel(), bi.numel()
        start = torch.cumsum(lens, 0) - lens
        ln = lens[bi]
        # two distinct members: the second is drawn from the other len - 1
        u = torch.rand(2, nb, generator=g, dtype=torch.float64).to(dev)
        r0 = (u[0] * ln).long().clamp(max=ln - 1)
        r1 = (u[1] * (ln - 1)).long().clamp(max=ln - 2)
        r1 = r1 + (r1 >= r0).long()
        c = torch.stack([X[rows[start[bi] + r0]], X[rows[start[bi] + r1]]])
        slot = torch.full((A,), -1, dtype=torch.long, device=dev)
        slot[bi] = torch.arange(nb, device=dev)
        sel = slot[node] >= 0
        P, pn = X[rows[sel]], slot[node][sel]  # rows of the big nodes
        for _ in range(4):
            d0 = (P - c[0][pn]).square().sum(1)
            d1 = (P - c[1][pn]).square().sum(1)
            idx = pn * 2 + (d1 < d0).long()
            sums = torch.zeros(nb * 2, dim, device=dev).index_add_(0, idx, P)
            cnt = torch.zeros(nb * 2, device=dev).index_add_(
                0, idx, torch.ones_like(d0))
            mean = (sums / cnt.clamp(min=1)[:, None]).view(nb, 2, dim)
            has = (cnt > 0).view(nb, 2, 1)
            c = torch.where(has, mean, c.permute(1, 0, 2)).permute(1, 0, 2)
        w = c[0] - c[1]
        nrm = w.norm(dim=1)
        flat = nrm < 1e-12
        if bool(flat.any()):  # degenerate: a random hyperplane
            r = torch.randn(int(flat.sum()), dim, generator=g).to(dev)
            w[flat], nrm[flat] = r, r.norm(dim=1)
        w = w / nrm[:, None]
        b = -(w * (c[0] + c[1])).sum(1) / 2
        return w, b

    # ---- persistence ----
    def save(self, path: str, keep_vectors: bool = True):
        torch.save({
            "planes": self.planes.cpu(), "bias": self.bias.cpu(),
            "child": self.child.cpu(), "roots": self.roots.cpu(),
            "leaf_off": self.leaf_off.cpu(),
            "leaf_items": self.leaf_items.cpu(), "metric": self.metric,
            "vectors": self.X.cpu().contiguous() if keep_vectors else None,
        }, path)

    @classmethod
    def load(cls, path: str, device="cpu",
             vectors: torch.Tensor = None) -> "ForestIndex":
        """``vectors`` supplies X for a file saved without them."""
        d = torch.load(path, map_location="cpu", weights_only=False)
        X = d["vectors"] if vectors is None else vectors
        if X is None:
            raise ValueError("the file holds no vectors; pass vectors=")
        return cls(X.to(device), d["planes"], d["bias"], d["child"],
                   d["roots"], d["leaf_off"], d["leaf_items"],
                   metric=d["metric"])
