"""Word-embedding trainer (CBOW) — MI355X-native.

Capability parity with the reference Train_Embed_Algo
(/root/reference/LightCTR/train/train_embed_algo.{h,cpp}):
  * CBOW objective over a sliding window
  * BOTH output losses: hierarchical softmax over a Huffman tree
    (train_embed_algo.cpp:15-72, :140-170) and negative sampling with the
    pow-0.75 unigram table (train_embed_algo.h:175-200)
  * frequent-word subsampling (:111-118)
  * post-training L2 normalization (:87-92)
  * product-quantization hook for compressed export (:208-225)
  * pretrained-vector load (loadPretrainFile, train_embed_algo.h:76-98)

Rebuilt batched for GPU: examples are (center, context) pairs assembled on
device; hierarchical-softmax paths are padded [B, max_depth] gathers;
negative sampling draws from a precomputed alias-free cumulative table via
torch.searchsorted. All updates are dense batched index_add (the
reference's lock-free Hogwild update maps to scatter-add determinism here).
"""

from __future__ import annotations

import heapq
from collections import Counter
from dataclasses import dataclass

import torch


@dataclass
class EmbedHyper:
    dim: int = 64
    window: int = 5
    negatives: int = 5
    lr: float = 0.5  # minibatch-mean semantics (batched, not per-example)
    min_count: int = 1
    subsample_t: float = 1e-3
    loss: str = "negsample"  # negsample | hsoftmax
    seed: int = 1234


def build_huffman(counts: list[int]):
    """Huffman tree for hierarchical softmax (reference :15-72).
    Returns (codes, paths): per word, the bit code and inner-node ids."""
    V = len(counts)
    heap = [(c, i) for i, c in enumerate(counts)]
    heapq.heapify(heap)
    parent = {}
    bit = {}
    nxt = V
    while len(heap) > 1:
        c1, n1 = heapq.heappop(heap)
        c2, n2 = heapq.heappop(heap)
        parent[n1], bit[n1] = nxt, 0
        parent[n2], bit[n2] = nxt, 1
        heapq.heappush(heap, (c1 + c2, nxt))
        nxt += 1
    root = heap[0][1] if heap else V
    codes, paths = [], []
    for w in range(V):
        code, path = [], []
        n = w
        while n != root:
            code.append(bit[n])
            path.append(parent[n] - V)  # inner-node index
            n = parent[n]
        codes.append(list(reversed(code)))
        paths.append(list(reversed(path)))
    return codes, paths, max(1, nxt - V)


class EmbedModel:
    def __init__(self, vocab: list[str], counts: list[int],
                 hyper: EmbedHyper, device: str = "cpu"):
        self.h = hyper
        self.vocab = vocab
        self.word2id = {w: i for i, w in enumerate(vocab)}
        self.counts = torch.tensor(counts, dtype=torch.float64)
        self.device = torch.device(device)
        V, D = len(vocab), hyper.dim
        g = torch.Generator().manual_seed(hyper.seed)
        self.E = ((torch.rand(V, D, generator=g) - 0.5) / D).to(self.device)
        if hyper.loss == "hsoftmax":
            codes, paths, n_inner = build_huffman(counts)
            md = max(len(c) for c in codes)
            self.path = torch.full((V, md), -1, dtype=torch.long)
            self.code = torch.zeros(V, md)
            for w, (c, p) in enumerate(zip(codes, paths)):
                self.path[w, :len(p)] = torch.tensor(p)
                self.code[w, :len(c)] = torch.tensor(c, dtype=torch.float32)
            self.path = self.path.to(self.device)
            self.code = self.code.to(self.device)
            self.O = torch.zeros(n_inner, D, device=self.device)
        else:
            # pow-0.75 unigram cumulative table (reference 1e8-slot table
            # becomes an exact cumulative-probability search)
            p = self.counts.pow(0.75)
            self.neg_cdf = (torch.cumsum(p, 0) / p.sum()).float().to(
                self.device)
            self.O = torch.zeros(V, D, device=self.device)
        self._gen = torch.Generator(device="cpu")
        self._gen.manual_seed(hyper.seed + 1)

    # ---- data prep ----
    def subsample_keep(self, ids: torch.Tensor) -> torch.Tensor:
        """Frequent-word subsampling mask (reference :111-118)."""
        freq = (self.counts / self.counts.sum()).float()
        t = self.h.subsample_t
        keep_p = (torch.sqrt(freq / t) + 1) * (t / freq)
        keep_p = keep_p.clamp(max=1.0)[ids.cpu()]
        return (torch.rand(ids.numel(), generator=self._gen)
                < keep_p).to(ids.device)

    def train_stream(self, ids: torch.Tensor, epochs: int = 1,
                     batch: int = 4096, log=None):
        """ids: long tensor token stream."""
        ids = ids.to(self.device)
        keep = self.subsample_keep(ids)
        ids = ids[keep]
        n = ids.numel()
        W = self.h.window
        for ep in range(epochs):
            total, nb = 0.0, 0
            for s in range(W, n - W, batch):
                e = min(s + batch, n - W)
                centers = ids[s:e]
                # context window gather [B, 2W]
                offs = torch.cat([torch.arange(-W, 0),
                                  torch.arange(1, W + 1)]).to(self.device)
                ctx = ids[(torch.arange(s, e, device=self.device)
                           .unsqueeze(1) + offs)]
                loss = self._step(centers, ctx)
                total += loss
                nb += 1
            if log:
                log(f"epoch {ep}: loss={total / max(nb, 1):.5f}")
        return self

    # ---- one CBOW step ----
    def _step(self, centers: torch.Tensor, ctx: torch.Tensor) -> float:
        h = self.h
        B, C = ctx.shape
        x = self.E[ctx].mean(dim=1)  # [B, D] context mean
        if h.loss == "hsoftmax":
            path = self.path[centers]  # [B, md]
            code = self.code[centers]
            mask = path >= 0
            pid = path.clamp(min=0)
            o = self.O[pid]  # [B, md, D]
            z = torch.einsum("bd,bmd->bm", x, o)
            p = torch.sigmoid(z.clamp(-16, 16))
            # label: code bit (go-right probability); minibatch-mean grads
            gz = (p - code) * mask.float() / B  # [B, md]
            loss = -(torch.log(p.clamp(1e-7)) * code
                     + torch.log((1 - p).clamp(1e-7)) * (1 - code))
            loss = float((loss * mask).sum() / mask.sum())
            gx = torch.einsum("bm,bmd->bd", gz, o)
            go = gz.unsqueeze(2) * x.unsqueeze(1)  # [B, md, D]
            self.O.index_add_(0, pid.reshape(-1),
                              -h.lr * go.reshape(-1, o.shape[2]))
        else:
            neg = torch.searchsorted(
                self.neg_cdf,
                torch.rand(B, h.negatives, generator=self._gen)
                .to(self.device)).clamp(max=self.E.shape[0] - 1)
            if self.device.type == "cuda" and h.dim <= 64:
                # fused CDNA4 kernel (Hogwild across examples, like the
                # reference's lock-free update)
                from ..ops._extension import require_hip_ops

                loss_t = require_hip_ops().w2v_negsample_step(
                    self.E, self.O, centers.long().contiguous(),
                    ctx.long().contiguous(), neg.long().contiguous(),
                    h.lr, 1.0 / B)
                return float(loss_t.mean())
            tgt = torch.cat([centers.unsqueeze(1), neg], dim=1)  # [B, 1+N]
            lbl = torch.zeros(B, 1 + h.negatives, device=self.device)
            lbl[:, 0] = 1.0
            o = self.O[tgt]
            z = torch.einsum("bd,bnd->bn", x, o)
            p = torch.sigmoid(z.clamp(-16, 16))
            gz = (p - lbl) / B  # minibatch-mean grads
            loss = float(-(lbl * torch.log(p.clamp(1e-7)) + (1 - lbl)
                           * torch.log((1 - p).clamp(1e-7))).sum(1).mean())
            gx = torch.einsum("bn,bnd->bd", gz, o)
            go = gz.unsqueeze(2) * x.unsqueeze(1)
            self.O.index_add_(0, tgt.reshape(-1),
                              -h.lr * go.reshape(-1, o.shape[2]))
        # context embedding update (mean backward: 1/C to each ctx word)
        gctx = (gx / C).unsqueeze(1).expand(B, C, gx.shape[1])
        self.E.index_add_(0, ctx.reshape(-1),
                          -self.h.lr * gctx.reshape(-1, gx.shape[1]))
        return loss

    # ---- post-processing & export ----
    def normalize(self):
        """L2-normalize embeddings (reference :87-92)."""
        self.E /= self.E.norm(dim=1, keepdim=True).clamp(min=1e-12)
        return self

    def quantize(self, n_sub: int = 4):
        """PQ export hook (reference :208-225)."""
        from ..utils.compress import ProductQuantizer

        pq = ProductQuantizer(self.h.dim, n_sub=n_sub,
                              n_centroids=min(256, self.E.shape[0]))
        pq.fit(self.E)
        return pq, pq.encode(self.E)

    def most_similar(self, word: str, k: int = 5):
        wid = self.word2id[word]
        e = self.E / self.E.norm(dim=1, keepdim=True).clamp(min=1e-12)
        sims = e @ e[wid]
        vals, idx = sims.topk(k + 1)
        return [(self.vocab[i], float(v)) for v, i in zip(vals, idx)
                if i != wid][:k]

    def build_index(self, kind: str = "flat", metric: str = "ip", **kw):
        """Index the table for batched search (predict/knn.py): ``flat``
        is exact, ``pq`` takes PQIndex.build's keywords (n_sub, ...),
        ``forest`` ForestIndex.build's (n_trees, leaf_size, seed). For
        ``ip`` a unit-length copy of E is indexed, so the ranking is the
        cosine ranking of ``most_similar``. Rebuild after more training."""
        from ..predict.knn import FlatIndex, PQIndex
        from ..predict.rp_forest import ForestIndex

        E = self.E
        if metric == "ip":
            E = E / E.norm(dim=1, keepdim=True).clamp(min=1e-12)
        E = E.contiguous()
        if kind == "flat":
            index = FlatIndex(E, metric)
        elif kind == "pq":
            kw.setdefault("n_sub", 4)
            index = PQIndex.build(E, metric=metric, **kw)
        elif kind == "forest":
            index = ForestIndex.build(E, metric=metric, **kw)
        else:
            raise ValueError(f"kind must be 'flat', 'pq' or 'forest', "
                             f"got {kind!r}")
        self._index, self._index_vectors = index, E
        return index

    def neighbors(self, words: list[str], k: int = 5, **search_kw):
        """Per word, its k nearest other words as [(word, score)] from the
        index of ``build_index`` (built with the defaults if absent), all
        words in one batched search. score is the cosine similarity for
        an ``ip`` index and the squared distance for ``l2``."""
        index = getattr(self, "_index", None) or self.build_index()
        wids = [self.word2id[w] for w in words]
        Q = self._index_vectors[torch.tensor(wids, dtype=torch.long,
                                             device=self.device)]
        ids, dist = index.search(Q, k + 1, **search_kw)
        sign = -1.0 if index.metric == "ip" else 1.0
        out = []
        for wid, row_i, row_d in zip(wids, ids.tolist(), dist.tolist()):
            hits = [(self.vocab[i], sign * d)
                    for i, d in zip(row_i, row_d) if i >= 0 and i != wid]
            out.append(hits[:k])
        return out

    def save(self, path: str):
        torch.save({"vocab": self.vocab, "E": self.E,
                    "counts": self.counts}, path)

    @classmethod
    def load_pretrain(cls, path: str, hyper: EmbedHyper,
                      device: str = "cpu"):
        d = torch.load(path, map_location=device, weights_only=False)
        m = cls(d["vocab"], d["counts"].tolist(), hyper, device=device)
        m.E = d["E"].to(device)
        return m


def vocab_from_tokens(tokens: list[str], min_count: int = 1):
    c = Counter(tokens)
    vocab = [w for w, n in c.most_common() if n >= min_count]
    counts = [c[w] for w in vocab]
    return vocab, counts
