"""CPU tests of the nearest-neighbour search (predict/knn.py): the result
contract, the CPU paths against the float64 / explicit-loop definitions of
``knn_oracles.py``, the wrong references the GPU tests' inputs must expose,
the EmbedModel and CLI entry points, and recall on planted clusters."""

import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import knn_oracles as ko
from lightctr_amd.predict import FlatIndex, PQIndex
from lightctr_amd.predict.knn import (KNN_MAX_K, adc_distances, pq_lut,
                                      select_topk)

REPO = Path(__file__).resolve().parent.parent
METRICS = ("l2", "ip")


def bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_same(got, ref, name=""):
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert torch.equal(got[0], ref[0]), f"{name}: ids differ"
    assert bits_equal(got[1], ref[1]), f"{name}: distances differ bitwise"


# ---------------------------------------------------------------------------
# contract
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_tie_goes_to_lower_id(metric):
    X = torch.ones(37, 5)
    ids, dist = FlatIndex(X, metric).search(torch.ones(3, 5), 9)
    assert torch.equal(ids, torch.arange(9, dtype=torch.int32).repeat(3, 1))
    assert bool((dist == (0.0 if metric == "l2" else -5.0)).all())


def test_negative_zero_ties_with_positive_zero():
    d = torch.tensor([[0.0, -0.0, -0.0, 0.0]])
    ids, _ = select_topk(d, 4)
    assert ids.tolist() == [[0, 1, 2, 3]]
    ids, _ = ko.topk(d, 4)
    assert ids.tolist() == [[0, 1, 2, 3]]


@pytest.mark.parametrize("metric", METRICS)
def test_k_above_n_pads(metric):
    X, Q = ko.flat_case(4, 3, 2)
    ids, dist = FlatIndex(X, metric).search(Q, 7)
    assert_same((ids, dist), ko.flat_ref(X, Q, metric, 7))
    assert bool((ids[:, 4:] == -1).all())
    assert bool((dist[:, 4:] == ko.INF).all())
    assert bool((ids[:, :4] >= 0).all())


def test_k_out_of_range_raises():
    X, Q = ko.flat_case(10, 4, 1)
    ix = FlatIndex(X)
    for k in (0, -1, KNN_MAX_K + 1, 2.0):
        with pytest.raises(ValueError):
            ix.search(Q, k)
    ix.search(Q, KNN_MAX_K)
    cent, codes, Qp = ko.pq_case(10, 2, 2, 4, 1)
    with pytest.raises(ValueError):
        PQIndex(ko.FakePQ(cent), codes).search(Qp, KNN_MAX_K + 1)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_input_raises(bad):
    X, Q = ko.flat_case(10, 4, 2)
    Xb, Qb = X.clone(), Q.clone()
    Xb[3, 1] = bad
    Qb[1, 0] = bad
    with pytest.raises(ValueError):
        FlatIndex(Xb)
    with pytest.raises(ValueError):
        FlatIndex(X).search(Qb, 1)
    cent, codes, Qp = ko.pq_case(10, 2, 2, 4, 2)
    cb = cent.clone()
    cb[1, 2, 0] = bad
    with pytest.raises(ValueError):
        PQIndex(ko.FakePQ(cb), codes)
    Qpb = Qp.clone()
    Qpb[0, 3] = bad
    with pytest.raises(ValueError):
        PQIndex(ko.FakePQ(cent), codes).search(Qpb, 1)
    with pytest.raises(ValueError):
        PQIndex.build(Xb, 2)


def test_bad_arguments_raise():
    X, Q = ko.flat_case(10, 4, 2)
    with pytest.raises(ValueError):
        FlatIndex(X, metric="cosine")
    with pytest.raises(ValueError):
        FlatIndex(X.double())
    with pytest.raises(ValueError):
        FlatIndex(X).search(Q[:, :3], 1)
    with pytest.raises(ValueError):
        FlatIndex(X).search(Q, 1, cand=torch.tensor([[0], [10]]))
    with pytest.raises(ValueError):
        FlatIndex(X).search(Q, 1, cand=torch.tensor([[0, 1]]))
    cent, codes, Qp = ko.pq_case(10, 2, 2, 4, 2)
    with pytest.raises(ValueError):  # a code past the codebook
        PQIndex(ko.FakePQ(cent[:, :3]), torch.full_like(codes, 3))
    with pytest.raises(ValueError):
        PQIndex(ko.FakePQ(cent), codes[:, :1])
    with pytest.raises(ValueError):  # rerank without vectors
        PQIndex(ko.FakePQ(cent), codes).search(Qp, 1, rerank=4)
    ix = PQIndex(ko.FakePQ(cent), codes, vectors=ko.ints((10, 4), 3))
    with pytest.raises(ValueError):
        ix.search(Qp, 4, rerank=2)


# ---------------------------------------------------------------------------
# CPU paths against the definitions
# ---------------------------------------------------------------------------
FLAT_SHAPES = [(1, 1, 1), (65, 3, 3), (257, 16, 5), (1025, 4, 2)]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("N,dim,nq", FLAT_SHAPES)
def test_flat_cpu_exact(metric, N, dim, nq):
    X, Q = ko.flat_case(N, dim, nq)
    for k in (1, 10, min(N + 3, KNN_MAX_K)):
        assert_same(FlatIndex(X, metric).search(Q, k),
                    ko.flat_ref(X, Q, metric, k), f"k={k}")


@pytest.mark.parametrize("metric", METRICS)
def test_flat_cpu_float_set(metric):
    X, Q = ko.flat_case(300, 24, 4, exact=False)
    ids, dist = FlatIndex(X, metric).search(Q, 10)
    d64, mag = ko.dist64(Q, X, metric)
    ko.check_float_result("flat_cpu", ids, dist, d64, mag, 24, 10)


@pytest.mark.parametrize("metric", METRICS)
def test_cand_skips_minus_one_and_counts_duplicates_once(metric):
    X, Q = ko.flat_case(50, 3, 3)
    cand = torch.tensor([[7, -1, 7, 3, 3, 49, -1, 0],
                         [-1, -1, -1, -1, -1, -1, -1, -1],
                         [5, 5, 5, 5, 5, 5, 5, 5]], dtype=torch.int32)
    for k in (1, 3, 6):
        got = FlatIndex(X, metric).search(Q, k, cand=cand)
        assert_same(got, ko.flat_ref(X, Q, metric, k, cand=cand), f"k={k}")
    ids, dist = FlatIndex(X, metric).search(Q, 6, cand=cand)
    assert sorted(ids[0].tolist()) == [-1, -1, 0, 3, 7, 49]
    assert ids[1].tolist() == [-1] * 6 and ids[2].tolist() == [5] + [-1] * 5
    assert bool((dist[1] == ko.INF).all())


@pytest.mark.parametrize("tied", [False, True])
def test_adc_cpu_is_the_explicit_fp32_loop(tied):
    lut, codes = ko.adc_case(333, 5, 7, 3, tied=tied)
    d = adc_distances(lut, codes)
    acc = torch.zeros(3, 333)
    for s in range(5):  # explicit fp32 adds in ascending s from 0.0f
        for q in range(3):
            acc[q] = acc[q] + lut[q, s][codes[:, s].long()]
    assert torch.equal(d, acc) and bits_equal(d, ko.adc32(lut, codes))
    assert_same(select_topk(d, 10), ko.adc_ref(lut, codes, 10))


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n_sub,d_sub", [(1, 8), (8, 1), (4, 3)])
def test_pq_cpu_exact_and_n_sub_edges(metric, n_sub, d_sub):
    """n_sub = 1 and n_sub = dim; the LUT is exact on integer inputs, so
    the whole search equals the definition."""
    cent, codes, Q = ko.pq_case(200, n_sub, d_sub, 16, 3)
    ix = PQIndex(ko.FakePQ(cent), codes, metric)
    l64, _ = ko.lut64(Q, cent, metric)
    assert torch.equal(ix.lut(Q).double(), l64)
    assert bits_equal(pq_lut(Q, cent, metric), l64.float())
    assert_same(ix.search(Q, 10), ko.adc_ref(l64.float(), codes, 10))


@pytest.mark.parametrize("metric", METRICS)
def test_pq_lut_float_set(metric):
    cent, codes, Q = ko.pq_case(10, 4, 6, 16, 3, exact=False)
    l64, mag = ko.lut64(Q, cent, metric)
    err = (pq_lut(Q, cent, metric).double() - l64).abs()
    assert bool((err <= 6 * ko.U23 * mag).all())


@pytest.mark.parametrize("metric", METRICS)
def test_rerank_all_rows_equals_flat(metric):
    X, Q = ko.flat_case(120, 8, 4)
    ix = PQIndex.build(X, 4, n_centroids=16, iters=3, metric=metric)
    flat = FlatIndex(X, metric).search(Q, 10)
    assert_same(ix.search(Q, 10, rerank=120), flat)
    assert_same(ix.search(Q, 10, rerank=10 ** 6), flat)
    # a partial re-rank returns exact distances of ADC-chosen rows
    ids, dist = ix.search(Q, 5, rerank=20)
    d64, _ = ko.dist64(Q, X, metric)
    assert torch.equal(dist.double(), torch.gather(d64, 1, ids.long()))
    cand, _ = ix.search(Q, 20)
    assert_same((ids, dist), ko.flat_ref(X, Q, metric, 5, cand=cand))


def test_build_honours_a_shrunk_codebook():
    """ProductQuantizer.fit shrinks the codebook when N < n_centroids."""
    X, Q = ko.flat_case(40, 8, 3)
    ix = PQIndex.build(X, 2, n_centroids=256, iters=2)
    assert ix.ncb == 40 and ix.lut(Q).shape == (3, 2, 40)
    ids, dist = ix.search(Q, 5)
    assert_same((ids, dist), ko.adc_ref(ix.lut(Q), ix.codes, 5))
    assert_same(ix.search(Q, 5, rerank=40), FlatIndex(X).search(Q, 5))


def test_quantize_codes_are_searchable():
    from lightctr_amd.models.embedding import EmbedHyper, EmbedModel

    vocab = [f"w{i}" for i in range(30)]
    m = EmbedModel(vocab, [5] * 30, EmbedHyper(dim=8, seed=1))
    m.E = ko.normals((30, 8), 4)
    pq, codes = m.quantize(n_sub=2)
    ix = PQIndex(pq, codes)
    ids, dist = ix.search(m.E[:4].contiguous(), 3)
    assert_same((ids, dist), ko.adc_ref(ix.lut(m.E[:4].contiguous()),
                                        codes, 3))


@pytest.mark.parametrize("keep", [True, False])
def test_save_load_round_trip(tmp_path, keep):
    X, Q = ko.flat_case(90, 6, 3)
    ix = PQIndex.build(X, 3, n_centroids=8, iters=2, metric="ip",
                       keep_vectors=keep)
    p = str(tmp_path / "ix.pt")
    ix.save(p)
    jx = PQIndex.load(p)
    assert jx.metric == "ip" and (jx.flat is not None) == keep
    assert torch.equal(jx.codes, ix.codes)
    assert bits_equal(jx.centroids, ix.centroids)
    assert_same(jx.search(Q, 7), ix.search(Q, 7))
    if keep:
        assert_same(jx.search(Q, 7, rerank=16), ix.search(Q, 7, rerank=16))


# ---------------------------------------------------------------------------
# wrong references, on the GPU tests' own inputs
# ---------------------------------------------------------------------------
# test_knn_gpu.py runs the kernels on these same builders' outputs
@pytest.mark.parametrize("metric", METRICS)
def test_wrong_references_differ_flat(metric):
    base, sliced = ko.flat_base(metric), ko.flat_sliced(metric)
    for X, Q, _, k in (base, sliced):
        ref = ko.flat_ref(X, Q, metric, k)
        assert_same(FlatIndex(X, metric).search(Q, k), ref)
        assert not ko.same(ref, ko.flat_ref(X, Q, metric, k,
                                            mutant="tie_high"))
    X, Q, _, k = sliced  # query 1's unique best row is the last row
    ref = ko.flat_ref(X, Q, metric, k)
    assert not ko.same(ref, ko.flat_ref(X, Q, metric, k,
                                        mutant="drop_last_row"))
    for mutant in ("drop_slice_boundary", "unstable_merge"):
        assert not ko.same(ref, ko.flat_ref(X, Q, metric, k,
                                            mutant=mutant)), mutant
    # the right merge of slice partials is the definition
    d, _ = ko.dist64(Q, X, metric)
    assert ko.same(ref, ko.merge_partials(d, k, ko.slice_rows(X.shape[0],
                                                              Q.shape[0])))


@pytest.mark.parametrize("metric", METRICS)
def test_wrong_references_differ_cand(metric):
    X, Q, _, k, cand = ko.cand_base(metric)
    ref = ko.flat_ref(X, Q, metric, k, cand=cand)
    assert_same(FlatIndex(X, metric).search(Q, k, cand=cand), ref)
    assert not ko.same(ref, ko.flat_ref(X, Q, metric, k, cand=cand,
                                        mutant="cand_dup_twice"))


def test_wrong_references_differ_adc():
    for lut, codes, k in (ko.adc_base(tied=False), ko.adc_base(tied=True)):
        ref = ko.adc_ref(lut, codes, k)
        assert_same(select_topk(adc_distances(lut, codes), k), ref)
        assert not ko.same(ref, ko.adc_ref(lut, codes, k,
                                           mutant="drop_last_sub"))
    lut, codes, k = ko.adc_base(tied=False)  # row N-1 is query 0's best
    assert not ko.same(ko.adc_ref(lut, codes, k),
                       ko.adc_ref(lut, codes, k, mutant="drop_last_row"))
    lut, codes, k = ko.adc_base(tied=True)
    assert not ko.same(ko.adc_ref(lut, codes, k),
                       ko.adc_ref(lut, codes, k, mutant="tie_high"))


def test_slice_rule_edges():
    assert ko.slice_rows(1, 1) == ko.MIN_SLICE
    assert ko.slice_rows(2 * ko.MIN_SLICE + 1, 1) == ko.MIN_SLICE
    assert ko.slice_rows(1 << 20, 1) == ko.MIN_SLICE
    assert ko.slice_rows(1 << 20, 64) == 65536
    assert ko.slice_rows(1 << 20, 1024) == 1 << 20
    assert ko.slice_rows((1 << 20) + 1, 1024) == (1 << 20) + ko.ROUND


# ---------------------------------------------------------------------------
# EmbedModel, CLI, bench tool
# ---------------------------------------------------------------------------
def toy_embed_model(device="cpu"):
    from lightctr_amd.models.embedding import (EmbedHyper, EmbedModel,
                                               vocab_from_tokens)

    g = torch.Generator().manual_seed(0)
    toks = []
    for _ in range(300):
        grp = "a" if torch.rand(1, generator=g) < 0.5 else "b"
        toks.extend(f"{grp}{int(i)}" for i in torch.randperm(5, generator=g))
    vocab, counts = vocab_from_tokens(toks)
    m = EmbedModel(vocab, counts, EmbedHyper(dim=16, seed=3), device=device)
    m.train_stream(torch.tensor([m.word2id[t] for t in toks]), epochs=2)
    return m


def test_embed_neighbors_agree_with_most_similar():
    m = toy_embed_model()
    m.build_index(kind="flat")
    words = list(m.vocab)
    res = m.neighbors(words, 3)
    for w, got in zip(words, res):
        want = m.most_similar(w, 3)
        assert len(got) == 3 and w not in [n for n, _ in got]
        assert {n for n, _ in got} == {n for n, _ in want}
        sw = dict(want)
        for n, s in got:  # unit vectors: sum|term| <= 1, dim terms
            assert abs(s - sw[n]) <= 2 * 16 * ko.U23
    # pq with a full re-rank is the flat answer
    m.build_index(kind="pq", n_sub=4, n_centroids=8, iters=3)
    assert m.neighbors(words, 3, rerank=len(words)) == res
    assert all(len(r) == 3 for r in m.neighbors(words, 3))


def run_cli(*argv):
    r = subprocess.run([sys.executable, "-m", "lightctr_amd.cli", *argv],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()


def test_cli_neighbors_round_trip(tmp_path):
    p = str(tmp_path / "emb.pt")
    run_cli("train", "--model", "embed", "--epochs", "1", "--rows", "200",
            "--device", "cpu", "--no-watchdog", "--save", p)
    out = json.loads(run_cli("neighbors", "--load", p, "--words", "a0,b1",
                             "--topk", "5", "--device", "cpu")[-1])
    assert set(out["neighbors"]) == {"a0", "b1"}
    for w, hits in out["neighbors"].items():
        assert len(hits) == 5 and w not in [n for n, _ in hits]
        scores = [s for _, s in hits]
        assert scores == sorted(scores, reverse=True)
    pq = json.loads(run_cli("neighbors", "--load", p, "--words", "a0,b1",
                            "--topk", "5", "--index", "pq", "--pq-sub", "4",
                            "--rerank", "32", "--device", "cpu")[-1])
    # 10 words: rerank 32 >= N is the exact search
    assert pq["neighbors"] == out["neighbors"]


def test_bench_knn_cpu_smoke():
    r = subprocess.run([sys.executable, str(REPO / "tools" / "bench_knn.py"),
                        "--device", "cpu", "--small"], cwd=REPO,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [json.loads(line) for line in r.stdout.strip().splitlines()]
    assert {(x["path"], x["nq"]) for x in rows} >= {("flat", 1), ("adc", 1)}
    assert all(x["outputs_match"] for x in rows)


# ---------------------------------------------------------------------------
# recall on planted clusters (seeded, CPU only)
# ---------------------------------------------------------------------------
# measured on the CPU path (docs/TESTING.md)
RECALL_ADC = 0.4781
RECALL_RERANK64 = 0.9969


@pytest.fixture(scope="module")
def planted():
    g = torch.Generator().manual_seed(11)
    centres = torch.randn(64, 32, generator=g) * 4
    X = centres[torch.randint(0, 64, (4096,), generator=g)] \
        + torch.randn(4096, 32, generator=g)
    Q = X[torch.randperm(4096, generator=g)[:64]] \
        + 0.1 * torch.randn(64, 32, generator=g)
    ix = PQIndex.build(X, 8, n_centroids=256, iters=10, seed=0)
    truth, _ = FlatIndex(X).search(Q, 10)
    return ix, Q, truth


def recall(ids, truth):
    hit = sum(len(set(a.tolist()) & set(b.tolist()))
              for a, b in zip(ids, truth))
    return hit / truth.numel()


def test_recall_on_planted_clusters(planted):
    ix, Q, truth = planted
    assert recall(ix.search(Q, 10, rerank=4096)[0], truth) == 1.0
    r0 = recall(ix.search(Q, 10)[0], truth)
    r64 = recall(ix.search(Q, 10, rerank=64)[0], truth)
    print(f"RECALL adc {r0:.4f} rerank64 {r64:.4f}")
    assert r0 >= RECALL_ADC - 0.05
    assert r64 >= RECALL_RERANK64 - 0.05
    assert r64 >= r0
