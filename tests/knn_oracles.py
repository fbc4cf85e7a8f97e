"""float64 definitions, shared inputs, wrong references and bounds for the
nearest-neighbour search tests (``test_knn.py`` on the CPU,
``test_knn_gpu.py`` on the GPU).

Plain helper module, imported like ``kernel_oracles.py``. Everything here
runs on the CPU and is written from the result contract in
``lightctr_amd/predict/knn.py``, not from the project's code paths:

* distances: float64 sums over the vector dimension;
* selection: the k smallest (dist, id) pairs, found with a lexicographic
  key sort (``np.lexsort``), not with the stable torch sort the CPU path
  uses;
* ADC: an explicit loop over sub-vectors of ``np.float32`` additions
  starting from 0.0f.

Exact-input rule: X, Q and centroids are integers in {-3..3}, so every
product, difference square (at most 36) and partial sum is an integer below
2^24 and exact in fp32 in any order while ``dim * 36 < 2^24``
(``assert_exact``). The float64 result cast to fp32 is then what any
correct fp32 evaluation gives, bit for bit.

Float rule (docs/TESTING.md, sums): a distance of n terms obeys
``|out - ref64| <= n 2^-23 sum|term|`` with the terms as the kernel forms
them: ``(q-x)^2`` or ``q*x``. For l2 the subtraction q-x is one more
rounding of relative size u = 2^-24 that the square doubles, so first order
is ``(2u + u + (n-1) u) sum|term| = (n+2) u sum|term|``, within the rule's
``2 n u`` from n = 2 on. A one-term l2 sum can be 3u off under any correct
fp32 evaluation, above the rule's 2u, so the float set uses n >= 2 for l2
and one-term l2 sums (dim = 1, d_sub = 1) are held on the exact set, where
they must be bit-equal.
"""

from __future__ import annotations

import numpy as np
import torch

U23 = 2.0 ** -23
INF = float("inf")

# mirror of knn_kernels.hip's slicing rule (the GPU tests assert that it
# equals the exported knn_slice_rows on every shape they use)
MIN_SLICE = 1024
ROUND = 1024
TARGET_BLOCKS = 1024


def slice_rows(n, nq):
    want = (TARGET_BLOCKS + max(nq, 1) - 1) // max(nq, 1)
    rows = (max(n, 1) + want - 1) // want
    rows = (rows + ROUND - 1) // ROUND * ROUND
    return max(rows, MIN_SLICE)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def ints(shape, seed, lo=-3, hi=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def normals(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def assert_exact(dim):
    assert dim * 36 < 2 ** 24, "exact-input rule violated"


def flat_case(N, dim, nq, seed=0, exact=True):
    """(X, Q). With dim small and values in {-3..3} ties are plentiful."""
    if exact:
        assert_exact(dim)
        return ints((N, dim), seed), ints((nq, dim), seed + 1)
    return normals((N, dim), seed), normals((nq, dim), seed + 1)


def adc_case(N, n_sub, ncb, nq, seed=0, tied=False):
    """(lut, codes): an arbitrary float LUT fed straight to the ADC scan.
    ``tied`` draws the LUT from {0, 0.5, 1} so that equal sums abound."""
    g = torch.Generator().manual_seed(seed)
    if tied:
        lut = torch.randint(0, 3, (nq, n_sub, ncb), generator=g).float() / 2
    else:
        lut = torch.randn(nq, n_sub, ncb, generator=g)
    codes = torch.randint(0, ncb, (N, n_sub), generator=g).to(torch.uint8)
    return lut, codes


def pq_case(N, n_sub, d_sub, ncb, nq, seed=0, exact=True):
    """(centroids [n_sub, ncb, d_sub], codes, Q)."""
    dim = n_sub * d_sub
    g = torch.Generator().manual_seed(seed + 7)
    codes = torch.randint(0, ncb, (N, n_sub), generator=g).to(torch.uint8)
    if exact:
        assert_exact(dim)
        return ints((n_sub, ncb, d_sub), seed), codes, ints((nq, dim),
                                                            seed + 1)
    return (normals((n_sub, ncb, d_sub), seed), codes,
            normals((nq, dim), seed + 1))


def flat_base(metric="l2"):
    """(X, Q, metric, k): the case the GPU shape sweeps vary one axis of."""
    X, Q = flat_case(257, 16, 3, seed=0)
    return X, Q, metric, 10


def flat_sliced(metric="l2", nq=3):
    """Two slices + 1 row. Query 0's unique best row is the last row of the
    first slice; query 1's is the last row of X; ties cross the slices."""
    N = 2 * MIN_SLICE + 1
    assert slice_rows(N, nq) == MIN_SLICE
    X, Q = flat_case(N, 8, nq, seed=5)
    Q[0] = torch.tensor([3., -3, 3, -3, 3, -3, 3, -3])
    Q[1] = torch.tensor([-3., -3, 3, 3, -3, -3, 3, 3])
    for q, row in ((0, MIN_SLICE - 1), (1, N - 1)):
        X[(X == Q[q]).all(1)] = 0.0  # no accidental copies
        X[row] = Q[q]
    return X, Q, metric, 10


def cand_base(metric="l2"):
    """(X, Q, metric, k, cand): lists with -1 and duplicates; each query's
    best listed row is listed twice."""
    X, Q = flat_case(300, 8, 3, seed=9)
    g = torch.Generator().manual_seed(10)
    cand = torch.randint(0, 300, (3, 40), generator=g).to(torch.int32)
    cand[:, 3::7] = -1
    d, _ = dist64(Q, X, metric)
    for q in range(3):
        listed = cand[q][cand[q] >= 0].long()
        cand[q, 5] = cand[q, 0] = listed[d[q][listed].argmin()]
    return X, Q, metric, 10, cand


def adc_base(tied=False):
    """(lut, codes, k): an arbitrary float LUT for the raw ADC scan."""
    lut, codes = adc_case(1025, 5, 16, 3, seed=2, tied=tied)
    codes[-1] = lut[0].argmin(dim=1).to(torch.uint8)  # query 0: last row
    return lut, codes, 10


class FakePQ:
    """What PQIndex reads of a ProductQuantizer."""

    def __init__(self, centroids):
        self.centroids = centroids


# ---------------------------------------------------------------------------
# float64 definitions
# ---------------------------------------------------------------------------
def dist64(Q, X, metric):
    """([nq, N] float64 distance, [nq, N] float64 sum|term|)."""
    Q, X = Q.double(), X.double()
    if metric == "ip":
        t = Q[:, None, :] * X[None, :, :]
        return 0.0 - t.sum(2), t.abs().sum(2)
    t = (Q[:, None, :] - X[None, :, :]) ** 2
    return t.sum(2), t.sum(2)


def lut64(Q, centroids, metric):
    """([nq, n_sub, ncb] float64 table, sum|term|)."""
    n_sub, ncb, d_sub = centroids.shape
    Qs = Q.double().view(Q.shape[0], n_sub, 1, d_sub)
    C = centroids.double()[None]
    if metric == "ip":
        t = Qs * C
        return 0.0 - t.sum(3), t.abs().sum(3)
    t = (Qs - C) ** 2
    return t.sum(3), t.sum(3)


def adc32(lut, codes, n_sub=None):
    """[nq, N] fp32: np.float32 additions in ascending s from 0.0f."""
    lut = lut.numpy().astype(np.float32)
    codes = codes.numpy().astype(np.int64)
    n_sub = lut.shape[1] if n_sub is None else n_sub
    acc = np.zeros((lut.shape[0], codes.shape[0]), dtype=np.float32)
    for s in range(n_sub):
        acc = (acc + lut[:, s, :][:, codes[:, s]]).astype(np.float32)
    return torch.from_numpy(acc)


def topk(d, k, ids=None, tie="low"):
    """Contract selection over d [nq, M] (float32 or float64): the k
    smallest (dist, id), padded with (-1, +inf). ``ids`` [M] or [nq, M]
    names the columns (negative = skip). tie="high" is the wrong rule."""
    d = d.numpy()
    nq, M = d.shape
    if ids is None:
        ids = np.arange(M)
    ids = np.broadcast_to(np.asarray(ids), (nq, M))
    out_i = np.full((nq, k), -1, dtype=np.int32)
    out_d = np.full((nq, k), np.inf, dtype=np.float32)
    for q in range(nq):
        keep = ids[q] >= 0
        dq, iq = d[q][keep] + 0.0, ids[q][keep]  # + 0.0: -0 ties with +0
        order = np.lexsort((iq if tie == "low" else -iq, dq))[:k]
        out_i[q, :len(order)] = iq[order]
        out_d[q, :len(order)] = dq[order].astype(np.float32)
    return torch.from_numpy(out_i), torch.from_numpy(out_d)


# ---------------------------------------------------------------------------
# references (mutant=None) and the wrong references the tests must tell
# from them on their own inputs
# ---------------------------------------------------------------------------
def flat_ref(X, Q, metric, k, cand=None, mutant=None, nq_for_slices=None):
    """(ids, dist fp32) from float64 distances; exact on the exact set."""
    N = X.shape[0]
    d, _ = dist64(Q, X, metric)
    nq = Q.shape[0]
    if cand is not None:
        c = cand.long().numpy()
        dd = torch.gather(d, 1, cand.long().clamp(min=0))
        if mutant == "cand_dup_twice":
            return topk(dd, k, ids=c)
        ids = c.copy()
        for q in range(nq):  # duplicates count once
            seen = set()
            for j in range(ids.shape[1]):
                if ids[q, j] in seen:
                    ids[q, j] = -1
                seen.add(ids[q, j])
        return topk(dd, k, ids=ids)
    if mutant == "drop_last_row":
        return topk(d[:, :N - 1], k)
    if mutant == "tie_high":
        return topk(d, k, tie="high")
    sr = slice_rows(N, nq if nq_for_slices is None else nq_for_slices)
    if mutant == "drop_slice_boundary":
        ids = np.arange(N)
        ids[sr - 1] = -1  # last row of the first slice
        return topk(d, k, ids=ids)
    if mutant == "unstable_merge":
        return merge_partials(d, k, sr, stable=False)
    return topk(d, k)


def merge_partials(d, k, sr, stable=True):
    """Per-slice top-k lists merged. The right merge orders by (dist, id);
    the unstable one orders by dist alone and lets the later slice win."""
    N = d.shape[1]
    parts = []
    for b in range(0, N, sr):
        i, v = topk(d[:, b:b + sr], k)
        parts.append((torch.where(i >= 0, i + b, i), v))
    if not stable:
        parts = parts[::-1]
    ids = torch.cat([p[0] for p in parts], 1)
    val = torch.cat([p[1] for p in parts], 1)
    if stable:
        return topk(val, k, ids=ids.numpy())
    order = torch.sort(val, dim=1, stable=True)[1][:, :k]
    return (torch.gather(ids, 1, order).int(), torch.gather(val, 1, order))


def adc_ref(lut, codes, k, mutant=None):
    if mutant == "drop_last_sub":
        return topk(adc32(lut, codes, lut.shape[1] - 1), k)
    d = adc32(lut, codes)
    if mutant == "drop_last_row":
        return topk(d[:, :-1], k)
    if mutant == "tie_high":
        return topk(d, k, tie="high")
    return topk(d, k)


def same(a, b):
    """both outputs equal (ids as values, dist bit for bit)"""
    return bool(torch.equal(a[0], b[0])) and bool(
        torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)))


# ---------------------------------------------------------------------------
# float-set check
# ---------------------------------------------------------------------------
def check_float_result(name, ids, dist, d64, mag, n_terms, k):
    """The float-set conditions of docs/TESTING.md for one search: ascending
    distances; each within ``n 2^-23 sum|term|`` of the float64 distance of
    its id; no omitted row closer than the k-th returned distance minus
    that bound. Returns the largest err/bound (information only)."""
    ids, dist = ids.cpu().long(), dist.cpu().double()
    nq, N = d64.shape
    bound = n_terms * U23 * mag
    worst = 0.0
    for q in range(nq):
        got = ids[q][ids[q] >= 0]
        kk = min(k, N)
        assert got.numel() == kk, f"{name}: query {q} returned {got.numel()}"
        assert got.unique().numel() == kk, f"{name}: query {q} repeats an id"
        dq = dist[q, :kk]
        assert bool((dq[1:] >= dq[:-1]).all()), f"{name}: not ascending"
        err = (dq - d64[q, got]).abs()
        b = bound[q, got]
        assert bool((err <= b).all()), (
            f"{name}: query {q} distance outside the sum rule, worst "
            f"{float((err / b.clamp(min=1e-300)).max()):.3g}")
        pos = b > 0
        if pos.any():
            worst = max(worst, float((err[pos] / b[pos]).max()))
        if kk < N:
            omitted = torch.ones(N, dtype=torch.bool)
            omitted[got] = False
            slack = d64[q][omitted] + bound[q][omitted]
            assert bool((slack >= dq[-1]).all()), (
                f"{name}: query {q} omits a row closer than its k-th")
    print(f"RATIO {name} {worst:.4f}")
    return worst
