"""GPU tests of the nearest-neighbour kernels (ops/csrc/knn_kernels.hip)
and of FlatIndex / PQIndex on ``cuda:0``.

Exact set: integer inputs (``knn_oracles`` exact-input rule) or an
arbitrary float LUT fed straight to the ADC scan; ids must be equal and
distances bit-equal to the CPU path, which ``test_knn.py`` holds to the
float64 / explicit-loop definitions. One axis is varied at a time around a
base case. Float set: the three sum-rule conditions of
``knn_oracles.check_float_result``."""

import pytest
import torch

import knn_oracles as ko
from kernel_oracles import check_bits
from lightctr_amd.ops._extension import require_hip_ops
from lightctr_amd.predict import FlatIndex, PQIndex
from lightctr_amd.predict.knn import (KNN_MAX_K, adc_distances, pq_lut,
                                      select_topk)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
METRICS = ("l2", "ip")
MID = {"l2": 0, "ip": 1}
SR = ko.MIN_SLICE
NS = sorted({1, 63, 64, 65, 255, 256, 257, 1025, SR - 1, SR, SR + 1,
             2 * SR + 1})
KS = [1, 2, 10, 63, 64, 65, KNN_MAX_K]


@pytest.fixture(scope="module")
def ops():
    return require_hip_ops()


def check(name, got, ref):
    assert torch.equal(got[0].cpu(), ref[0]), f"{name}: ids differ"
    check_bits(name, got[1], ref[1])


def flat_gpu(ops, X, Q, metric, k, cand=None):
    return ops.flat_topk(X.to(DEV), Q.to(DEV), MID[metric], k,
                         None if cand is None else cand.to(DEV))


def flat_cpu(X, Q, metric, k, cand=None):
    return FlatIndex(X, metric).search(Q, k, cand=cand)


def adc_cpu(lut, codes, k):
    return select_topk(adc_distances(lut, codes), k)


def adc_gpu(ops, lut, codes, k):
    return ops.pq_adc_topk(lut.to(DEV), codes.to(DEV), lut.shape[2], k)


# ---------------------------------------------------------------------------
# flat, exact set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N", NS)
def test_flat_rows(ops, metric, N):
    assert ops.knn_slice_rows(N, 3) == ko.slice_rows(N, 3) == SR
    X, Q = ko.flat_case(N, 16, 3, seed=N)
    check("flat", flat_gpu(ops, X, Q, metric, 10),
          flat_cpu(X, Q, metric, 10))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", KS)
def test_flat_k(ops, metric, k):
    X, Q, _, _ = ko.flat_base(metric)
    check("flat", flat_gpu(ops, X, Q, metric, k), flat_cpu(X, Q, metric, k))


@pytest.mark.parametrize("metric", METRICS)
def test_flat_k_above_n(ops, metric):
    X, Q = ko.flat_case(100, 16, 3)
    got = flat_gpu(ops, X, Q, metric, 103)
    check("flat", got, flat_cpu(X, Q, metric, 103))
    assert bool((got[0][:, 100:] == -1).all())
    assert bool((got[1][:, 100:] == ko.INF).all())


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nq", [1, 3, 64, 65])
def test_flat_queries(ops, metric, nq):
    X, Q = ko.flat_case(257, 16, nq, seed=nq)
    check("flat", flat_gpu(ops, X, Q, metric, 10),
          flat_cpu(X, Q, metric, 10))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("dim", [1, 3, 4, 63, 64, 100, 1024])
def test_flat_dim(ops, metric, dim):
    X, Q = ko.flat_case(257, dim, 3, seed=dim)
    check("flat", flat_gpu(ops, X, Q, metric, 10),
          flat_cpu(X, Q, metric, 10))


@pytest.mark.parametrize("metric", METRICS)
def test_flat_views(ops, metric):
    """an X that is only 4-byte aligned (scalar body although dim % 4 ==
    0), and column slices with a row stride that is not dim"""
    X, Q = ko.flat_case(257, 16, 3, seed=21)
    ref = flat_cpu(X, Q, metric, 10)
    Qd = Q.to(DEV)
    buf = torch.zeros(257 * 16 + 1, device=DEV)
    buf[1:] = X.reshape(-1).to(DEV)
    off = buf[1:].view(257, 16)
    assert off.data_ptr() % 16 == 4
    check("offset", ops.flat_topk(off, Qd, MID[metric], 10), ref)
    big = ko.ints((257, 40), 22).to(DEV)
    for c0 in (4, 1):  # 16-byte aligned and 4-byte aligned column slices
        big[:, c0:c0 + 16] = X.to(DEV)
        view = big[:, c0:c0 + 16]
        assert view.stride(0) == 40 and not view.is_contiguous()
        check(f"slice{c0}", ops.flat_topk(view, Qd, MID[metric], 10), ref)
        got = FlatIndex(view, metric).search(Qd, 10)
        check(f"index{c0}", got, ref)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [10, KNN_MAX_K])
def test_flat_two_slices_planted(ops, metric, k):
    """best row last in its slice (query 0), unique best row last in X
    (query 1), ties across the slice boundary"""
    X, Q, _, _ = ko.flat_sliced(metric)
    got = flat_gpu(ops, X, Q, metric, k)
    check("sliced", got, flat_cpu(X, Q, metric, k))
    assert int(got[0][0, 0]) == SR - 1 and int(got[0][1, 0]) == 2 * SR


@pytest.mark.parametrize("metric", METRICS)
def test_flat_k_best_in_final_slice(ops, metric):
    N = 2 * SR + 1
    X = torch.zeros(N, 8)
    Q = torch.stack([torch.full((8,), 3.0), torch.ones(8)])
    X[-7:] = Q[0]  # the 7 best of query 0 are the last 7 rows
    X[SR:SR + 3] = Q[1]
    got = flat_gpu(ops, X, Q, metric, 7)
    check("final", got, flat_cpu(X, Q, metric, 7))
    assert got[0][0].tolist() == list(range(N - 7, N))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N", [300, 2 * SR + 1])
def test_flat_all_distances_equal(ops, metric, N):
    X, Q = torch.ones(N, 8), torch.ones(2, 8)
    ids, dist = flat_gpu(ops, X, Q, metric, 65)
    assert torch.equal(ids.cpu(),
                       torch.arange(65, dtype=torch.int32).repeat(2, 1))
    check("equal", (ids, dist), flat_cpu(X, Q, metric, 65))


# ---------------------------------------------------------------------------
# candidate lists
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("k", [1, 10, 64])
def test_cand_minus_one_and_duplicates(ops, metric, k):
    X, Q, _, _, cand = ko.cand_base(metric)
    check("cand", flat_gpu(ops, X, Q, metric, k, cand),
          flat_cpu(X, Q, metric, k, cand))


@pytest.mark.parametrize("metric", METRICS)
def test_cand_shorter_than_k_and_empty_rows(ops, metric):
    X, Q, _, _, cand = ko.cand_base(metric)
    cand = cand[:, :4].contiguous()
    cand[1] = -1
    got = flat_gpu(ops, X, Q, metric, 10, cand)
    check("cand", got, flat_cpu(X, Q, metric, 10, cand))
    assert bool((got[0][1] == -1).all()) and bool((got[0][:, 4:] == -1).all())


@pytest.mark.parametrize("metric", METRICS)
def test_cand_duplicates_across_slices(ops, metric):
    """R = two slices + 1 over 300 rows: every row is listed many times,
    in more than one slice, and must come back once"""
    X, Q = ko.flat_case(300, 8, 2, seed=31)
    g = torch.Generator().manual_seed(32)
    R = 2 * SR + 1
    assert ops.knn_slice_rows(R, 2) == SR
    cand = torch.randint(-1, 300, (2, R), generator=g).to(torch.int32)
    got = flat_gpu(ops, X, Q, metric, KNN_MAX_K, cand)
    check("cand", got, flat_cpu(X, Q, metric, KNN_MAX_K, cand))
    check("cand=all", got, flat_cpu(X, Q, metric, KNN_MAX_K))


# ---------------------------------------------------------------------------
# ADC on arbitrary float LUTs (bit-equal: ascending-s adds from 0.0f)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("N", NS)
def test_adc_rows(ops, tied, N):
    assert ops.knn_slice_rows(N, 3) == SR
    lut, codes = ko.adc_case(N, 16, 256, 3, seed=N, tied=tied)
    check("adc", adc_gpu(ops, lut, codes, 10), adc_cpu(lut, codes, 10))


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("n_sub", [1, 2, 3, 4, 5, 8, 16, 64])
def test_adc_sub_vectors(ops, tied, n_sub):
    lut, codes = ko.adc_case(1025, n_sub, 256, 3, seed=n_sub, tied=tied)
    check("adc", adc_gpu(ops, lut, codes, 10), adc_cpu(lut, codes, 10))


@pytest.mark.parametrize("ncb", [2, 16, 255, 256])
def test_adc_codebook_size(ops, ncb):
    lut, codes = ko.adc_case(1025, 8, ncb, 3, seed=ncb)
    check("adc", adc_gpu(ops, lut, codes, 10), adc_cpu(lut, codes, 10))


@pytest.mark.parametrize("tied", [False, True])
@pytest.mark.parametrize("k", KS)
def test_adc_k(ops, tied, k):
    lut, codes, _ = ko.adc_base(tied)
    check("adc", adc_gpu(ops, lut, codes, k), adc_cpu(lut, codes, k))


def test_adc_k_above_n(ops):
    lut, codes = ko.adc_case(100, 4, 16, 3)
    got = adc_gpu(ops, lut, codes, 103)
    check("adc", got, adc_cpu(lut, codes, 103))
    assert bool((got[0][:, 100:] == -1).all())


@pytest.mark.parametrize("nq", [1, 3, 64, 65])
def test_adc_queries(ops, nq):
    lut, codes = ko.adc_case(1025, 8, 16, nq, seed=nq, tied=True)
    check("adc", adc_gpu(ops, lut, codes, 10), adc_cpu(lut, codes, 10))


@pytest.mark.parametrize("k", [10, KNN_MAX_K])
def test_adc_two_slices(ops, k):
    N = 2 * SR + 1
    lut, codes = ko.adc_case(N, 4, 4, 3, seed=41, tied=True)
    # query 0: unique best row last in its slice; query 1: last in X
    lut[:2, :, 3] = -1.0
    codes[codes == 3] = 0
    codes[SR - 1] = 3
    lut[1, :, 2] = -2.0
    codes[codes == 2] = 1
    codes[N - 1] = 2
    got = adc_gpu(ops, lut, codes, k)
    check("adc", got, adc_cpu(lut, codes, k))
    assert int(got[0][0, 0]) == SR - 1 and int(got[0][1, 0]) == N - 1


def test_adc_code_views(ops):
    """a view one code row into its buffer, one a single byte in (byte
    body although n_sub % 8 == 0), and column slices of a wider table"""
    lut, codes = ko.adc_case(1025, 8, 16, 3, seed=51, tied=True)
    ref = adc_cpu(lut, codes, 10)
    lutd = lut.to(DEV)
    buf = torch.zeros(1026, 8, dtype=torch.uint8, device=DEV)
    buf[1:] = codes.to(DEV)
    check("row", ops.pq_adc_topk(lutd, buf[1:], 16, 10), ref)
    flat = torch.zeros(1025 * 8 + 1, dtype=torch.uint8, device=DEV)
    flat[1:] = codes.reshape(-1).to(DEV)
    view = flat[1:].view(1025, 8)
    assert view.data_ptr() % 4 == 1
    check("byte", ops.pq_adc_topk(lutd, view, 16, 10), ref)
    big = torch.zeros(1025, 32, dtype=torch.uint8, device=DEV)
    for c0 in (8, 3):
        big[:, c0:c0 + 8] = codes.to(DEV)
        view = big[:, c0:c0 + 8]
        assert view.stride(0) == 32
        check(f"cols{c0}", ops.pq_adc_topk(lutd, view, 16, 10), ref)


# ---------------------------------------------------------------------------
# float set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N,dim", [(257, 3), (257, 64), (257, 1024),
                                   (2 * SR + 1, 100)])
def test_flat_float_set(ops, metric, N, dim):
    X, Q = ko.flat_case(N, dim, 3, seed=dim, exact=False)
    ids, dist = flat_gpu(ops, X, Q, metric, 10)
    d64, mag = ko.dist64(Q, X, metric)
    ko.check_float_result(f"flat_{metric}_{dim}", ids, dist, d64, mag, dim,
                          10)


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_sub,d_sub,ncb", [(4, 6, 16), (16, 4, 256),
                                             (1, 64, 255), (32, 2, 256),
                                             (64, 1, 256)])
def test_pq_lut_float_and_exact(ops, metric, n_sub, d_sub, ncb):
    cent, _, Q = ko.pq_case(1, n_sub, d_sub, ncb, 5)
    got = ops.pq_lut(Q.to(DEV), cent.to(DEV), MID[metric])
    check_bits("lut", got, pq_lut(Q, cent, metric))
    if d_sub == 1 and metric == "l2":
        return  # one-term l2 sums are on the exact set only (knn_oracles)
    cent, _, Q = ko.pq_case(1, n_sub, d_sub, ncb, 5, exact=False)
    got = ops.pq_lut(Q.to(DEV), cent.to(DEV), MID[metric])
    l64, mag = ko.lut64(Q, cent, metric)
    err = (got.cpu().double() - l64).abs()
    assert bool((err <= d_sub * ko.U23 * mag).all())


# ---------------------------------------------------------------------------
# output hygiene
# ---------------------------------------------------------------------------
def poison_outputs(nq, k, n_slices):
    """blocks of the exact shapes of ids, dist and the partial keys, filled
    with values a correct result cannot hold, then freed (kernel_oracles.
    poison for shapes that cannot hold NaN). A partial key of 0 sorts in
    front of every real key."""
    blocks = [torch.full((nq, k), -7, dtype=torch.int32, device=DEV),
              torch.full((nq, k), float("nan"), device=DEV)]
    if n_slices > 1:
        blocks.append(torch.zeros(nq, n_slices, k, dtype=torch.int64,
                                  device=DEV))
    torch.cuda.synchronize()
    del blocks


@pytest.mark.parametrize("N", [100, 2 * SR + 1])
def test_poisoned_outputs_and_run_to_run(ops, N):
    k, nq = 103, 3  # k > N at N = 100: the padding must be written too
    n_slices = -(-N // SR)
    X, Q = ko.flat_case(N, 8, nq, seed=61)
    Xd, Qd = X.to(DEV), Q.to(DEV)
    lut, codes = ko.adc_case(N, 8, 16, nq, seed=62, tied=True)
    lutd, cd = lut.to(DEV), codes.to(DEV)
    cand = torch.arange(N, dtype=torch.int32).repeat(nq, 1).to(DEV)
    runs = []
    for _ in range(2):
        poison_outputs(nq, k, n_slices)
        a = ops.flat_topk(Xd, Qd, 0, k)
        poison_outputs(nq, k, n_slices)
        b = ops.pq_adc_topk(lutd, cd, 16, k)
        poison_outputs(nq, k, n_slices)
        c = ops.flat_topk(Xd, Qd, 0, k, cand)
        runs.append((a, b, c))
    check("flat", runs[0][0], flat_cpu(X, Q, "l2", k))
    check("adc", runs[0][1], adc_cpu(lut, codes, k))
    check("cand", runs[0][2], flat_cpu(X, Q, "l2", k))
    for first, second in zip(*runs):
        assert torch.equal(first[0], second[0])
        check_bits("rerun", second[1], first[1].cpu())


# ---------------------------------------------------------------------------
# bindings
# ---------------------------------------------------------------------------
def test_bindings_raise(ops):
    X, Q = (t.to(DEV) for t in ko.flat_case(10, 8, 2))
    lut, codes = (t.to(DEV) for t in ko.adc_case(10, 4, 16, 2))
    assert ops.knn_max_k() == KNN_MAX_K >= 256
    with pytest.raises(RuntimeError):
        ops.flat_topk(X, Q, 0, KNN_MAX_K + 1)
    with pytest.raises(RuntimeError):
        ops.flat_topk(X, Q, 0, 0)
    with pytest.raises(RuntimeError):
        ops.pq_adc_topk(lut, codes, 16, KNN_MAX_K + 1)
    with pytest.raises(RuntimeError):  # n_sub > 64
        ops.pq_adc_topk(torch.zeros(2, 65, 4, device=DEV),
                        torch.zeros(10, 65, dtype=torch.uint8, device=DEV),
                        4, 1)
    with pytest.raises(RuntimeError):
        ops.pq_lut(torch.zeros(2, 65, device=DEV),
                   torch.zeros(65, 4, 1, device=DEV), 0)
    with pytest.raises(RuntimeError):  # dim > 1024
        ops.flat_topk(torch.zeros(4, 1025, device=DEV),
                      torch.zeros(1, 1025, device=DEV), 0, 1)
    with pytest.raises(RuntimeError):  # dtypes
        ops.flat_topk(X.double(), Q, 0, 1)
    with pytest.raises(RuntimeError):
        ops.flat_topk(X, Q.double(), 0, 1)
    with pytest.raises(RuntimeError):
        ops.flat_topk(X, Q, 0, 1, torch.zeros(2, 3, dtype=torch.int64,
                                              device=DEV))
    with pytest.raises(RuntimeError):
        ops.pq_adc_topk(lut, codes.int(), 16, 1)
    with pytest.raises(RuntimeError):
        ops.pq_adc_topk(lut.double(), codes, 16, 1)
    with pytest.raises(RuntimeError):  # lut width != ncb
        ops.pq_adc_topk(lut, codes, 8, 1)
    with pytest.raises(RuntimeError):  # metric
        ops.flat_topk(X, Q, 2, 1)
    with pytest.raises(RuntimeError):  # Q / X widths
        ops.flat_topk(X, Q[:, :4].contiguous(), 0, 1)
    with pytest.raises(RuntimeError):  # CPU tensors
        ops.flat_topk(X.cpu(), Q.cpu(), 0, 1)
    # N == 0 is an all-padding answer, not an error
    ids, dist = ops.flat_topk(X[:0], Q, 0, 3)
    assert bool((ids == -1).all()) and bool((dist == ko.INF).all())


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_pq_index_on_device_equals_cpu_index(metric):
    """iters=0 keeps the centroids sampled rows, i.e. integers, so the LUT
    is exact and the whole search must equal the CPU index built from the
    same centroids and codes."""
    X, Q = ko.flat_case(500, 16, 5, seed=71)
    gx = PQIndex.build(X, 4, n_centroids=16, iters=0, metric=metric,
                       device=DEV)
    assert gx.codes.is_cuda and gx.centroids.is_cuda
    cx = PQIndex(ko.FakePQ(gx.centroids.cpu()), gx.codes.cpu(), metric,
                 vectors=X)
    check_bits("lut", gx.lut(Q), cx.lut(Q))
    for rerank in (0, 16, 500):
        got = gx.search(Q, 10, rerank=rerank)
        assert got[0].is_cuda
        check(f"rerank{rerank}", got, cx.search(Q, 10, rerank=rerank))
    check("flat", gx.search(Q, 10, rerank=500), flat_cpu(X, Q, metric, 10))


def test_pq_index_float_rerank_all_is_flat_within_the_sum_rule():
    X, Q = ko.flat_case(600, 32, 4, seed=81, exact=False)
    gx = PQIndex.build(X, 8, n_centroids=32, iters=3, device=DEV)
    ids, dist = gx.search(Q, 10, rerank=600)
    d64, mag = ko.dist64(Q, X, "l2")
    ko.check_float_result("pq_rerank_all", ids, dist, d64, mag, 32, 10)
    ids, dist = gx.search(Q, 10, rerank=64)  # exact distances of its ids
    err = (dist.cpu().double() - torch.gather(d64, 1, ids.cpu().long())).abs()
    assert bool((err <= 32 * ko.U23 * torch.gather(mag, 1,
                                                   ids.cpu().long())).all())


def test_embed_model_neighbors_on_device():
    from lightctr_amd.models.embedding import EmbedHyper, EmbedModel

    vocab = [f"w{i}" for i in range(200)]
    E = ko.normals((200, 32), 91)
    models = []
    for dev in ("cpu", DEV):
        m = EmbedModel(vocab, [3] * 200, EmbedHyper(dim=32), device=dev)
        m.E = E.to(dev)
        models.append(m)
    words = vocab[:7]
    cpu, gpu = (m.neighbors(words, 5) for m in models)
    assert models[1].build_index().X.is_cuda
    for w, a, b in zip(words, cpu, gpu):
        assert [n for n, _ in a] == [n for n, _ in b] and w not in dict(b)
        assert {n for n, _ in b} == {n for n, _ in
                                     models[0].most_similar(w, 5)}
        for (_, sa), (_, sb) in zip(a, b):  # unit vectors, 32 terms
            assert abs(sa - sb) <= 2 * 32 * ko.U23
    models[1].build_index(kind="pq", n_sub=4, n_centroids=16, iters=2)
    assert models[1].neighbors(words, 5, rerank=200) == \
        models[1].neighbors(words, 5, rerank=10 ** 6)
    assert all(len(r) == 5 for r in models[1].neighbors(words, 5))
