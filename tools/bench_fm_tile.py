"""Sweep behind the tile-local segment backward (GPU): FM step time under
hipGraph on the flagship batch pool, backward_mode="segment" (tile reduce)
against "segment_list" (work list + per-piece reduce) in one process.

The tile reduce's shape (entries per block, longest unit, units a subgroup
keeps in flight) is a set of template parameters, kFmTile / kFmTileSplit /
kFmTileFlight in fm_kernels.hip. A build that instantiates the other values
behind a run-time selector (ops.fm_segment_tile_select(tile, split, flight),
as was done for profiles/r5_01_fm_tile.txt) gets the whole grid swept; the
shipped build has one instantiation, and then only segment_cap is swept.

    python tools/bench_fm_tile.py [--steps 2000] [--passes 2]
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

TILES = (256, 512, 1024)
SPLITS = (16, 32, 64)
FLIGHTS = (1, 2, 4)
CAPS = (256, 512, 1024)


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
    h = FMHyper(num_features=F, k=16, optimizer="ftrl", seed=1234)
    m = FMModel(h, device="cuda")

    select = getattr(ops, "fm_segment_tile_select", None)
    if select is None:
        shapes = [(ops.fm_segment_tile(), ops.fm_segment_split(), None)]
        print(f"# one tile shape built: TILE {shapes[0][0]} SPLIT "
              f"{shapes[0][1]}; sweeping segment_cap only")
    else:
        shapes = [(t, s, f) for t in TILES for s in SPLITS for f in FLIGHTS]
    print(f"# step ms under hipGraph, {args.steps} steps, flagship pool")
    for p in range(args.passes):
        m.backward_mode = "segment_list"
        for cap in CAPS:
            m.segment_cap = cap
            ms = graph_ms(m, pool, args.steps)
            print(f"pass {p}: segment_list cap {cap:4d}  {ms:.4f} ms/step",
                  flush=True)
        m.backward_mode = "segment"
        for tile, split, flight in shapes:
            if select is not None:
                select(tile, split, flight)
            for cap in CAPS:
                if cap > tile:
                    continue
                m.segment_cap = cap
                ms = graph_ms(m, pool, args.steps)
                print(f"pass {p}: segment TILE {tile:4d} SPLIT {split:2d} "
                      f"flight {flight} cap {cap:4d}  {ms:.4f} ms/step",
                      flush=True)


if __name__ == "__main__":
    main()
