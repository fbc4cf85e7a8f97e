"""Sweeps behind the recompute segment backward (GPU):

  1. the radix sort alone, 4-byte index payload (radix_sort_index, iota fill
     included: that is what a step pays) against the 8-byte record payload
     (radix_sort_rec), device events, flagship nnz and end_bit;
  2. FM step time under hipGraph on the flagship batch pool for
     backward_mode x segment_cap. (The reduce's batch depth is a template
     parameter, kFmRecomputeDepth in fm_kernels.hip: sweeping it means
     rebuilding with the other value.)

    python tools/bench_fm_recompute.py [--steps 2000] [--passes 2]
"""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from lightctr_amd.data.synthetic import SyntheticCriteo
from lightctr_amd.models.fm import FMHyper, FMModel
from lightctr_amd.ops._extension import require_hip_ops


def event_us(fn, reps=200, warm=10):
    for _ in range(warm):
        fn()
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def graph_ms(model, pool, steps):
    def eager(i):
        row_ptr, _fields, fids, vals, labels = pool[i % len(pool)]
        return model.train_step(row_ptr, fids, vals, labels)

    for i in range(len(pool)):
        eager(i)
    torch.cuda.synchronize()
    graphs, keep = [], []
    for i in range(len(pool)):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            keep.append(eager(i))
        graphs.append(gr)
    for i in range(50):
        graphs[i % len(graphs)].replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        graphs[i % len(graphs)].replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--features", type=int, default=1 << 24)
    args = ap.parse_args()

    ops = require_hip_ops()
    F = args.features
    gen = SyntheticCriteo(num_features=F, seed=1234, device="cuda")
    pool = [gen.batch(args.batch) for _ in range(4)]

    # -- 1. the sort alone -------------------------------------------------
    fids = pool[0][2]
    nnz = fids.numel()
    end_bit = max(1, (F - 1).bit_length())
    rec = torch.randint(0, args.batch, (nnz, 2), dtype=torch.int32,
                        device="cuda")
    print(f"# sort alone, nnz={nnz} end_bit={end_bit}, us per call "
          "(device events, 200 calls)")
    for p in range(3):
        t4 = event_us(lambda: ops.radix_sort_index(fids, end_bit))
        t8 = event_us(lambda: ops.radix_sort_rec(fids, rec, end_bit))
        print(f"pass {p}: int32 index payload (iota incl.) {t4:7.1f}   "
              f"8-byte record payload {t8:7.1f}", flush=True)

    # -- 2. step time: mode x depth x cap -----------------------------------
    h = FMHyper(num_features=F, k=16, optimizer="ftrl", seed=1234)
    m = FMModel(h, device="cuda")
    configs = [("segment_emit", 256)]
    configs += [("segment", cap) for cap in (64, 128, 256, 512, 1024)]
    print(f"# step ms under hipGraph, {args.steps} steps, flagship pool")
    for p in range(args.passes):
        for mode, cap in configs:
            m.backward_mode = mode
            m.segment_cap = cap
            ms = graph_ms(m, pool, args.steps)
            print(f"pass {p}: {mode:12s} cap {cap:4d}  {ms:.4f} ms/step",
                  flush=True)


if __name__ == "__main__":
    main()
