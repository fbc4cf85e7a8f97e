"""Batched top-k search throughput: FlatIndex / PQIndex (the HIP kernels on
a GPU) against the same search written as torch ops on the same device,
same process, same data.

Baselines: flat = squared norms + matmul + ``topk``; ADC = the same LUT,
one ``gather`` per sub-vector summed in ascending order + ``topk``.

Protocol: outputs compared first (ADC distances bit for bit; flat
distances to 1e-3 relative and >= 99.9% id overlap, since the matmul
expansion rounds differently), warm-up of both paths, then alternating
rounds (A, B, A, B, ...) timed with device events (host clock on CPU);
median and min..max per path. One JSON line per (path, nq). bytes/s is the
kernel's compulsory traffic per query tile (one query per block here):
N * n_sub code bytes (ADC) or N * dim * 4 (flat), times nq.

    python tools/bench_knn.py                       # N = 2^20, dim 64
    python tools/bench_knn.py --device cpu --small  # smoke run
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from lightctr_amd.predict.knn import FlatIndex, PQIndex
from lightctr_amd.utils.compress import ProductQuantizer


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


def torch_adc(lut, codes_long, k):
    acc = torch.zeros(lut.shape[0], codes_long.shape[0], device=lut.device)
    for s in range(lut.shape[1]):
        acc = acc + lut[:, s, :][:, codes_long[:, s]]
    v, i = acc.topk(k, dim=1, largest=False)
    return i, v


def overlap(a, b):
    hit = sum(len(set(x.tolist()) & set(y.tolist())) for x, y in zip(a, b))
    return hit / a.numel()


def bench(name, ours, base, match, nq, nbytes, args, dev, extra):
    for _ in range(args.warmup):
        ours()
        base()
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed(ours, dev))
        tb.append(timed(base, dev))
    ma, mb = statistics.median(ta), statistics.median(tb)
    print(json.dumps({
        "path": name, "device": dev.type, "nq": nq, **extra,
        "rounds": args.rounds, "outputs_match": bool(match),
        "index_s": {"median": ma, "min": min(ta), "max": max(ta)},
        "torch_s": {"median": mb, "min": min(tb), "max": max(tb)},
        "speedup": mb / ma, "queries_per_s": nq / ma,
        "compulsory_bytes": nbytes, "index_bytes_per_s": nbytes / ma,
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default=None)
    ap.add_argument("--small", action="store_true",
                    help="tiny shapes (a smoke run; timings mean nothing)")
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--n-sub", type=int, default=16)
    ap.add_argument("--ncb", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", default="1,64,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    if args.small:
        args.rows, args.dim, args.n_sub, args.ncb = 5000, 16, 4, 16
        args.nq, args.rounds = "1,8", 2
    dev = torch.device(args.device or
                       ("cuda" if torch.cuda.is_available() else "cpu"))
    if dev.type == "cuda" and not torch.cuda.is_available():
        sys.exit("bench_knn: no GPU (use --device cpu --small)")

    g = torch.Generator().manual_seed(7)
    N, dim, k = args.rows, args.dim, args.k
    X = torch.randn(N, dim, generator=g).to(dev)
    # a codebook of sampled sub-vectors: the scan does not care how good
    # the quantiser is, and k-means on 2^20 rows is not what is timed
    pq = ProductQuantizer(dim, n_sub=args.n_sub, n_centroids=args.ncb)
    pick = torch.randperm(N, generator=g)[:args.ncb].to(dev)
    pq.centroids = X[pick].view(args.ncb, args.n_sub, pq.d_sub) \
        .transpose(0, 1).contiguous()
    codes = torch.cat([pq.encode(X[i:i + (1 << 16)])
                       for i in range(0, N, 1 << 16)])
    flat = FlatIndex(X, "l2")
    adc = PQIndex(pq, codes, "l2")
    x2 = (X * X).sum(1)
    codes_long = codes.long()
    extra = {"rows": N, "dim": dim, "n_sub": args.n_sub, "ncb": args.ncb,
             "k": k}

    for nq in (int(v) for v in args.nq.split(",")):
        Q = (X[torch.randperm(N, generator=g)[:nq].to(dev)]
             + 0.1 * torch.randn(nq, dim, generator=g).to(dev)).contiguous()
        ia, da = flat.search(Q, k)
        ib, db = torch_flat(X, x2, Q, k)
        ok = overlap(ia.cpu(), ib.cpu()) >= 0.999 and bool(
            torch.allclose(da, db, rtol=1e-3, atol=1e-3))
        bench("flat", lambda: flat.search(Q, k),
              lambda: torch_flat(X, x2, Q, k), ok, nq, nq * N * dim * 4,
              args, dev, extra)
        lut = adc.lut(Q)
        ia, da = adc.search(Q, k)
        ib, db = torch_adc(lut, codes_long, k)
        ok = bool(torch.equal(da, db.sort(dim=1)[0]))
        bench("adc", lambda: adc.search(Q, k),
              lambda: torch_adc(adc.lut(Q), codes_long, k), ok, nq,
              nq * N * args.n_sub, args, dev, extra)


if __name__ == "__main__":
    main()
