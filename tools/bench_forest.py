"""Compiled-forest GBM inference throughput: CompiledForest.predict_margin
against the unchanged GBMModel.predict_margin on the same device, same
process, same rows.

Protocol: a synthetic forest of random full-depth trees over quantile bins
fitted on the data; warm-up of both paths, then alternating rounds (A, B,
A, B, ...), each timed with device events (host clock on CPU); median and
min..max spread per path. The two outputs are compared bit for bit before
any timing. Bytes/s is the compiled kernel's compulsory traffic
(N*D*4 read + N*K*4 written) over its median time.

    python tools/bench_forest.py                      # 1M x 39, 100 trees
    python tools/bench_forest.py --cols 128
    python tools/bench_forest.py --rows 2000 --trees 5 --rounds 2 --cpu
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from lightctr_amd.models.gbm import GBMHyper, GBMModel, Tree


def full_tree(g, D, depth):
    """Full binary tree with `depth` split levels in parent-first order."""
    n_int = (1 << depth) - 1
    n = (1 << (depth + 1)) - 1
    ids = torch.arange(n)
    internal = ids < n_int
    feature = torch.where(internal, torch.randint(0, D, (n,), generator=g),
                          torch.full((n,), -1)).int()
    thr = torch.where(internal, torch.randint(0, 255, (n,), generator=g),
                      torch.zeros(n, dtype=torch.long)).int()
    left = torch.where(internal, 2 * ids + 1, torch.full((n,), -1)).int()
    right = torch.where(internal, 2 * ids + 2, torch.full((n,), -1)).int()
    value = torch.where(internal, torch.zeros(n),
                        torch.randn(n, generator=g) * 0.1)
    nanl = (torch.rand(n, generator=g) < 0.5) & internal
    return Tree(feature, thr, nanl, left, right, value)


def timed(fn, dev):
    if dev == "cuda":
        s, e = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e-3
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--cols", type=int, default=39)
    ap.add_argument("--trees", type=int, default=100)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu", action="store_true",
                    help="smoke the tool on CPU (timings mean nothing)")
    args = ap.parse_args()

    if args.cpu:
        dev = "cpu"
    elif torch.cuda.is_available():
        dev = "cuda"
    else:
        sys.exit("bench_forest: no GPU (use --cpu for a smoke run)")
    g = torch.Generator().manual_seed(7)
    X = torch.randn(args.rows, args.cols, generator=g)
    X[torch.rand(args.rows, args.cols, generator=g) < 0.02] = float("nan")
    m = GBMModel(GBMHyper(n_classes=2, max_depth=args.depth), device=dev)
    m._fit_bins(X[:100_000])
    m.trees = [[full_tree(g, args.cols, args.depth)]
               for _ in range(args.trees)]
    X = X.to(dev)
    forest = m.compile()

    a, b = forest.predict_margin(X), m.predict_margin(X)
    if not torch.equal(a, b):
        sys.exit("bench_forest: compiled margins differ from GBMModel's")
    for _ in range(args.warmup):
        forest.predict_margin(X)
        m.predict_margin(X)
    tc, tp = [], []
    for _ in range(args.rounds):
        tc.append(timed(lambda: forest.predict_margin(X), dev))
        tp.append(timed(lambda: m.predict_margin(X), dev))
    mc, mp = statistics.median(tc), statistics.median(tp)
    nbytes = args.rows * args.cols * 4 + args.rows * forest.n_classes * 4
    print(json.dumps({
        "device": dev, "rows": args.rows, "cols": args.cols,
        "trees": args.trees, "depth": args.depth, "rounds": args.rounds,
        "nodes": int(forest.nodes.shape[0]),
        "chunks": int(forest.chunks.shape[0]),
        "bit_identical": True,
        "compiled_s": {"median": mc, "min": min(tc), "max": max(tc)},
        "parent_s": {"median": mp, "min": min(tp), "max": max(tp)},
        "compiled_rows_per_s": args.rows / mc,
        "parent_rows_per_s": args.rows / mp,
        "speedup": mp / mc,
        "compulsory_bytes": nbytes,
        "compiled_bytes_per_s": nbytes / mc,
    }))


if __name__ == "__main__":
    main()
