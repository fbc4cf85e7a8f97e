"""ForestIndex search (forest_candidates_kernel + the candidate re-rank of
flat_topk on a GPU) against exact search on the same device, same process,
same data and queries: FlatIndex.search, and the same exact search written
as torch ops (squared norms + matmul + ``topk``).

Data: Gaussian clusters (spread 3, unit noise); the queries are data rows
plus noise of 0.1. The forest is built on the device by
``ForestIndex.build`` and its build time is reported.

Protocol (that of bench_knn.py): outputs compared first (the forest's
answer must be bit-equal to ``flat.search(cand=candidates)`` and no returned
distance may lie below the exact search's at the same rank), warm-up of all
paths, then alternating rounds (forest, flat, torch, forest, ...) timed with
device events (host clock on CPU); median and min..max per path. One JSON
line per (search_k, nq) with recall@k against FlatIndex.search, and one for
the build.

One wavefront walks the forest per query, so nq = 1 runs on a single
wavefront of the device.

    python tools/bench_rp_forest.py                       # N = 2^20, dim 64
    python tools/bench_rp_forest.py --device cpu --small  # smoke run
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from lightctr_amd.predict.knn import FlatIndex
from lightctr_amd.predict.rp_forest import ForestIndex


def sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()


def timed(fn, dev):
    if dev.type == "cuda":
        s, e = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e-3
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def torch_flat(X, x2, Q, k):
    d = (Q * Q).sum(1, keepdim=True) - 2.0 * (Q @ X.t()) + x2[None, :]
    v, i = d.topk(k, dim=1, largest=False)
    return i, v


def recall(ids, truth):
    hit = sum(len(set(a) & set(b))
              for a, b in zip(ids.tolist(), truth.tolist()))
    return hit / truth.numel()


def stats(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default=None)
    ap.add_argument("--small", action="store_true",
                    help="tiny shapes (a smoke run; timings mean nothing)")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--clusters", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--trees", type=int, default=8)
    ap.add_argument("--leaf-size", type=int, default=16)
    ap.add_argument("--search-k", default="160,640,2560")
    ap.add_argument("--nq", default="1,64,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.small:
        args.rows, args.dim, args.clusters = 5000, 16, 16
        args.nq, args.search_k, args.rounds = "1,64", "64,256", 2
    dev = torch.device(args.device or
                       ("cuda" if torch.cuda.is_available() else "cpu"))
    if dev.type == "cuda" and not torch.cuda.is_available():
        sys.exit("bench_rp_forest: no GPU (use --device cpu --small)")

    g = torch.Generator().manual_seed(7)
    N, dim, k = args.rows, args.dim, args.k
    centres = 3.0 * torch.randn(args.clusters, dim, generator=g)
    X = (centres[torch.randint(0, args.clusters, (N,), generator=g)]
         + torch.randn(N, dim, generator=g)).to(dev).contiguous()
    extra = {"device": dev.type, "rows": N, "dim": dim, "k": k,
             "trees": args.trees, "leaf_size": args.leaf_size}

    sync(dev)
    t0 = time.perf_counter()
    forest = ForestIndex.build(X, n_trees=args.trees,
                               leaf_size=args.leaf_size, seed=0)
    sync(dev)
    print(json.dumps({
        "path": "build", **extra, "build_s": time.perf_counter() - t0,
        "n_inner": forest.n_inner, "n_leaves": forest.n_leaves,
        "max_leaf": forest.max_leaf}), flush=True)
    flat = forest.flat
    x2 = (X * X).sum(1)

    for nq in (int(v) for v in args.nq.split(",")):
        Q = (X[torch.randperm(N, generator=g)[:nq].to(dev)]
             + 0.1 * torch.randn(nq, dim, generator=g).to(dev)).contiguous()
        truth, tdist = flat.search(Q, k)
        for sk in (int(v) for v in args.search_k.split(",")):
            ids, dist = forest.search(Q, k, search_k=sk)
            cand = forest.candidates(Q, sk)
            ri, rd = flat.search(Q, k, cand=cand)
            ok = bool(torch.equal(ids, ri)) and bool(torch.equal(
                dist.view(torch.int32), rd.view(torch.int32))) and bool(
                (dist >= tdist).all())
            paths = (lambda: forest.search(Q, k, search_k=sk),
                     lambda: flat.search(Q, k),
                     lambda: torch_flat(X, x2, Q, k))
            for _ in range(args.warmup):
                for fn in paths:
                    fn()
            times = [[], [], []]
            for _ in range(args.rounds):
                for t, fn in zip(times, paths):
                    t.append(timed(fn, dev))
            mf = statistics.median(times[0])
            print(json.dumps({
                "path": "forest", **extra, "nq": nq, "search_k": sk,
                "width": int(cand.shape[1]), "rounds": args.rounds,
                "outputs_match": ok,
                "recall": recall(ids.cpu(), truth.cpu()),
                "forest_s": stats(times[0]), "flat_s": stats(times[1]),
                "torch_s": stats(times[2]),
                "speedup_vs_flat": statistics.median(times[1]) / mf,
                "speedup_vs_torch": statistics.median(times[2]) / mf,
                "queries_per_s": nq / mf}), flush=True)


if __name__ == "__main__":
    main()
