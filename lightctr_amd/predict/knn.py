"""Batched nearest-neighbour search: exact (FlatIndex) and PQ-coded
(PQIndex) top-k over a device-resident table.

Result contract, the same on CPU and GPU. ``search(Q, k)`` returns
``ids int32 [nq, k]`` and ``dist float32 [nq, k]``:

* ``metric="l2"``: dist is the squared L2 distance (no square root);
  ``metric="ip"``: dist is ``0 - <q, x>``. Smaller is better in both.
* row q holds the k smallest pairs in ascending lexicographic (dist, id)
  order; the float comparison is ``<`` (so -0.0 and +0.0 tie) and a tie
  goes to the lower id. The result is unique.
* with fewer than k rows the trailing slots are id -1, dist +inf.
* ``1 <= k <= KNN_MAX_K``; non-finite vectors, centroids or queries raise
  ValueError.
* an ADC distance is ``lut[q, 0, code[n, 0]] + lut[q, 1, code[n, 1]] + ...``
  added in fp32 in ascending sub-vector order from 0.0f, so it is
  bit-identical on every device for the same LUT. Flat distances and LUT
  entries are sums over the vector dimension in any order.

The CPU path is plain torch and is the oracle of the GPU tests. On a CUDA
tensor the classes call ops/csrc/knn_kernels.hip through the extension;
there is no eager fallback.
"""

from __future__ import annotations

import torch

from ..ops._extension import require_hip_ops

# limits of the kernels (knn_kernels.hip exports them; the GPU path checks
# that the two agree)
KNN_MAX_K = 256
KNN_MAX_SUB = 64
KNN_MAX_DIM = 1024

_METRICS = {"l2": 0, "ip": 1}
_CHUNK = 1 << 22  # elements of one CPU distance block


def _finite(t: torch.Tensor, name: str):
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} holds non-finite values")


def _check_k(k: int):
    if not isinstance(k, int) or not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k must be an int in [1, {KNN_MAX_K}], got {k!r}")


def _check_q(Q, dim: int, device) -> torch.Tensor:
    if not isinstance(Q, torch.Tensor) or Q.dim() != 2 or Q.shape[1] != dim:
        raise ValueError(f"Q must be a [nq, {dim}] tensor")
    if Q.dtype != torch.float32:
        raise ValueError(f"Q must be float32, got {Q.dtype}")
    Q = Q.to(device).contiguous()
    _finite(Q, "Q")
    return Q


def _gpu_ops():
    ops = require_hip_ops()
    if (ops.knn_max_k(), ops.knn_max_sub(), ops.knn_max_dim()) != \
            (KNN_MAX_K, KNN_MAX_SUB, KNN_MAX_DIM):
        raise RuntimeError("knn kernel limits disagree with predict/knn.py")
    return ops


def select_topk(d: torch.Tensor, k: int, skip: torch.Tensor | None = None,
                ids: torch.Tensor | None = None):
    """The contract's selection over a [nq, M] distance matrix whose
    columns are in ascending id order: stable sort, first k, padded.
    ``skip`` marks columns that do not take part, ``ids`` [nq, M] names
    the columns (default: the column index)."""
    nq, M = d.shape
    sd, si = torch.sort(d, dim=1, stable=True)
    if skip is not None:
        # second stable pass: skipped columns last, the rest keep their
        # (dist, id) order, even next to a real +inf distance
        sk = torch.gather(skip, 1, si)
        _, sj = torch.sort(sk.to(torch.uint8), dim=1, stable=True)
        sd, si, sk = (torch.gather(a, 1, sj) for a in (sd, si, sk))
    out_i = si if ids is None else torch.gather(ids.long(), 1, si)
    if skip is not None:
        out_i = torch.where(sk, torch.full_like(out_i, -1), out_i)
        sd = torch.where(sk, torch.full_like(sd, float("inf")), sd)
    out_i, sd = out_i[:, :k], sd[:, :k]
    if M < k:
        out_i = torch.cat([out_i, out_i.new_full((nq, k - M), -1)], 1)
        sd = torch.cat([sd, sd.new_full((nq, k - M), float("inf"))], 1)
    return out_i.to(torch.int32).contiguous(), sd.contiguous()


def flat_distances(Q: torch.Tensor, X: torch.Tensor, metric: str):
    """[nq, N] fp32 distances of the contract (torch; any device)."""
    if metric == "ip":
        return 0.0 - Q @ X.t()
    return (Q[:, None, :] - X[None, :, :]).square().sum(dim=2)


class FlatIndex:
    """Exact search over ``X`` [N, dim] float32 (kept as given, so a
    strided view is searched in place)."""

    def __init__(self, X: torch.Tensor, metric: str = "l2", device=None):
        if metric not in _METRICS:
            raise ValueError(f"metric must be 'l2' or 'ip', got {metric!r}")
        if not isinstance(X, torch.Tensor) or X.dim() != 2:
            raise ValueError("X must be a 2-D tensor")
        if X.dtype != torch.float32:
            raise ValueError(f"X must be float32, got {X.dtype}")
        if X.shape[0] >= 1 << 31:
            raise ValueError("N must be below 2^31")
        if device is not None:
            X = X.to(device)
        self.device = X.device
        self._gpu = self.device.type == "cuda"
        if self._gpu:
            _gpu_ops()
            if not 1 <= X.shape[1] <= KNN_MAX_DIM:
                raise ValueError(f"dim must be in [1, {KNN_MAX_DIM}] on the "
                                 f"GPU, got {X.shape[1]}")
            if X.shape[0] > 1 and X.shape[1] > 1 and X.stride(1) != 1:
                X = X.contiguous()
        _finite(X, "X")
        self.X = X
        self.metric = metric
        self.N, self.dim = X.shape

    def search(self, Q: torch.Tensor, k: int, cand: torch.Tensor = None):
        _check_k(k)
        Q = _check_q(Q, self.dim, self.device)
        if cand is not None:
            if cand.dim() != 2 or cand.shape[0] != Q.shape[0]:
                raise ValueError("cand must be [nq, R]")
            cand = cand.to(self.device).to(torch.int32).contiguous()
            if cand.numel() and (int(cand.min()) < -1
                                 or int(cand.max()) >= self.N):
                raise ValueError("cand ids must be -1 or in [0, N)")
        if self._gpu:
            ids, dist = require_hip_ops().flat_topk(
                self.X, Q, _METRICS[self.metric], k, cand)
            return ids, dist
        if cand is None:
            return self._search_cpu(Q, k)
        return self._search_cand_cpu(Q, k, cand)

    def _search_cpu(self, Q, k):
        nq = Q.shape[0]
        step = max(1, _CHUNK // max(1, self.N * self.dim))
        out = [select_topk(flat_distances(Q[i:i + step], self.X,
                                          self.metric), k)
               for i in range(0, nq, step)]
        if not out:
            return (torch.zeros(0, k, dtype=torch.int32),
                    torch.zeros(0, k))
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    def _search_cand_cpu(self, Q, k, cand):
        nq, R = cand.shape
        if R == 0 or self.N == 0:
            return select_topk(torch.zeros(nq, 0), k)
        # ascending ids per row, so the stable sort breaks ties by id
        c, _ = torch.sort(cand.long(), dim=1)
        skip = c < 0
        skip[:, 1:] |= c[:, 1:] == c[:, :-1]  # duplicates count once
        rows = self.X[c.clamp(min=0)]  # [nq, R, dim]
        if self.metric == "ip":
            d = 0.0 - (rows * Q[:, None, :]).sum(dim=2)
        else:
            d = (Q[:, None, :] - rows).square().sum(dim=2)
        return select_topk(d, k, skip=skip, ids=c)


def pq_lut(Q: torch.Tensor, centroids: torch.Tensor, metric: str):
    """[nq, n_sub, ncb] fp32 table of per-sub-vector distances (torch)."""
    n_sub, ncb, d_sub = centroids.shape
    Qs = Q.view(Q.shape[0], n_sub, d_sub)
    if metric == "ip":
        return 0.0 - torch.einsum("qsd,scd->qsc", Qs, centroids)
    return (Qs[:, :, None, :] - centroids[None]).square().sum(dim=3)


def adc_distances(lut: torch.Tensor, codes: torch.Tensor):
    """[nq, N] ADC distances: fp32 adds in ascending sub-vector order
    from 0.0 (torch; the rule the kernel follows)."""
    nq, n_sub, _ = lut.shape
    acc = torch.zeros(nq, codes.shape[0], dtype=torch.float32,
                      device=lut.device)
    for s in range(n_sub):
        acc = acc + lut[:, s, :][:, codes[:, s].long()]
    return acc


class PQIndex:
    """Search over product-quantiser codes (asymmetric distance: the query
    stays exact, the rows are their centroids). ``pq`` is a fitted
    ``utils.compress.ProductQuantizer``; ``codes`` uint8 [N, n_sub] is what
    its ``encode`` returns and is kept as given. ``vectors`` (optional,
    [N, dim]) enables the exact re-rank."""

    def __init__(self, pq, codes: torch.Tensor, metric: str = "l2",
                 vectors: torch.Tensor = None):
        if metric not in _METRICS:
            raise ValueError(f"metric must be 'l2' or 'ip', got {metric!r}")
        cent = pq.centroids
        if cent is None:
            raise ValueError("the quantizer is not fitted")
        if cent.dim() != 3 or cent.dtype != torch.float32:
            raise ValueError("centroids must be float32 "
                             "[n_sub, ncb, d_sub]")
        n_sub, ncb, d_sub = cent.shape
        if not 1 <= n_sub <= KNN_MAX_SUB:
            raise ValueError(f"n_sub must be in [1, {KNN_MAX_SUB}], "
                             f"got {n_sub}")
        if not 1 <= ncb <= 256:
            raise ValueError(f"codebook size must be in [1, 256], got {ncb}")
        if not isinstance(codes, torch.Tensor) or codes.dim() != 2 \
                or codes.dtype != torch.uint8 or codes.shape[1] != n_sub:
            raise ValueError(f"codes must be uint8 [N, {n_sub}]")
        if codes.shape[0] >= 1 << 31:
            raise ValueError("N must be below 2^31")
        self.device = codes.device
        self._gpu = self.device.type == "cuda"
        if self._gpu:
            _gpu_ops()
            if codes.shape[0] > 1 and n_sub > 1 and codes.stride(1) != 1:
                codes = codes.contiguous()
        _finite(cent, "centroids")
        # a code past the (possibly shrunk) codebook would index outside
        # the distance table
        if codes.numel() and int(codes.max()) >= ncb:
            raise ValueError(f"codes hold values >= the codebook size {ncb}")
        self.centroids = cent.to(self.device).contiguous()
        self.codes = codes
        self.metric = metric
        self.n_sub, self.ncb, self.d_sub = n_sub, ncb, d_sub
        self.dim = n_sub * d_sub
        self.N = codes.shape[0]
        self.flat = None
        if vectors is not None:
            if vectors.shape != (self.N, self.dim):
                raise ValueError(f"vectors must be [{self.N}, {self.dim}]")
            self.flat = FlatIndex(vectors, metric, device=self.device)

    @classmethod
    def build(cls, X: torch.Tensor, n_sub: int, n_centroids: int = 256,
              iters: int = 10, seed: int = 0, keep_vectors: bool = True,
              metric: str = "l2", device=None) -> "PQIndex":
        from ..utils.compress import ProductQuantizer

        if device is not None:
            X = X.to(device)
        X = X.contiguous()
        _finite(X, "X")
        pq = ProductQuantizer(X.shape[1], n_sub=n_sub,
                              n_centroids=n_centroids, iters=iters, seed=seed)
        pq.fit(X)
        return cls(pq, pq.encode(X), metric=metric,
                   vectors=X if keep_vectors else None)

    def lut(self, Q: torch.Tensor) -> torch.Tensor:
        Q = _check_q(Q, self.dim, self.device)
        if self._gpu:
            return require_hip_ops().pq_lut(Q, self.centroids,
                                            _METRICS[self.metric])
        return pq_lut(Q, self.centroids, self.metric)

    def _adc(self, Q, k):
        lut = self.lut(Q)
        if self._gpu:
            ids, dist = require_hip_ops().pq_adc_topk(lut, self.codes,
                                                      self.ncb, k)
            return ids, dist
        nq = Q.shape[0]
        step = max(1, _CHUNK // max(1, self.N))
        out = [select_topk(adc_distances(lut[i:i + step], self.codes), k)
               for i in range(0, nq, step)]
        if not out:
            return (torch.zeros(0, k, dtype=torch.int32),
                    torch.zeros(0, k))
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    def search(self, Q: torch.Tensor, k: int, rerank: int = 0):
        """ADC top-k; with ``rerank = R >= k`` the ADC top-R are re-ranked
        by their exact distance (needs stored vectors). ``R >= N`` is the
        exact search."""
        _check_k(k)
        if not rerank:
            return self._adc(Q, k)
        if self.flat is None:
            raise ValueError("rerank needs an index built with vectors")
        if rerank < k:
            raise ValueError(f"rerank must be 0 or >= k, got {rerank}")
        if rerank >= self.N:
            return self.flat.search(Q, k)
        if rerank > KNN_MAX_K:
            raise ValueError(f"rerank must be <= {KNN_MAX_K} or >= N")
        cand, _ = self._adc(Q, int(rerank))
        return self.flat.search(Q, k, cand=cand)

    def save(self, path: str):
        torch.save({
            "codes": self.codes.cpu().contiguous(),
            "centroids": self.centroids.cpu(),
            "metric": self.metric,
            "vectors": (None if self.flat is None
                        else self.flat.X.cpu().contiguous()),
        }, path)

    @classmethod
    def load(cls, path: str, device="cpu") -> "PQIndex":
        from ..utils.compress import ProductQuantizer

        d = torch.load(path, map_location="cpu", weights_only=False)
        cent = d["centroids"]
        pq = ProductQuantizer(cent.shape[0] * cent.shape[2],
                              n_sub=cent.shape[0], n_centroids=cent.shape[1])
        pq.centroids = cent.to(device)
        vec = d["vectors"]
        return cls(pq, d["codes"].to(device), metric=d["metric"],
                   vectors=None if vec is None else vec.to(device))
