"""The record sort of the FM step alone (GPU), device events:

  * rocPRIM's radix sort at its default config (radix_sort_rec),
  * the single-purpose onesweep sort (onesweep_sort_rec) at its built tile,

on the fids of the flagship batch pool (SyntheticCriteo(seed=1234)
.batch(65536), end_bit 24) and on uniform-random keys of the same size.
Every timed variant is first checked against the rocPRIM default result.

The sweeps of profiles/r6_01_fm_sort.txt ran on builds that also had rocPRIM
at explicit onesweep configs (radix_sort_rec_cfg(keys, rec, end_bit, cfg))
and every onesweep tile shape behind a run-time selector (a `shape` argument
of onesweep_sort_rec, onesweep_sort_tile_of(shape)); where a build has those
bindings this tool times them too, under the names of the last sweep.

    python tools/bench_fm_sort.py [--passes 2] [--reps 200]
"""
import argparse
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch

from lightctr_amd.data.synthetic import SyntheticCriteo
from lightctr_amd.ops._extension import require_hip_ops

ROCPRIM_CFGS = {0: "256x8", 1: "512x8", 2: "512x12", 3: "256x16"}
_TILES = {0: "256x16", 1: "512x8", 2: "512x16"}
# sweep-build selector: tile shape + 4 * (window index) + 16 * (poll mode:
# 0 re-reads the window while it waits, 1 waits on the one word it needs)
_WINDOWS = {0: 2, 1: 4, 2: 8}
ONESWEEP_SHAPES = {
    t + 4 * w + 16 * p: f"{name} w{win} poll{p}"
    for p in (0, 1) for w, win in _WINDOWS.items()
    for t, name in _TILES.items()}


def event_us(fn, reps, warm=10):
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


def variants(ops, status):
    """name -> callable(keys, rec, end_bit)"""
    out = {"rocprim default": ops.radix_sort_rec}
    if hasattr(ops, "radix_sort_rec_cfg"):
        for cfg, name in ROCPRIM_CFGS.items():
            out[f"rocprim {name}"] = (
                lambda k, r, e, c=cfg: ops.radix_sort_rec_cfg(k, r, e, c))
    if hasattr(ops, "onesweep_sort_tile_of"):
        for shape, name in ONESWEEP_SHAPES.items():
            tile = ops.onesweep_sort_tile_of(shape)
            out[f"onesweep {name} (tile {tile})"] = (
                lambda k, r, e, s=shape: ops.onesweep_sort_rec(
                    k, r, e, status, s))
    else:
        out[f"onesweep (tile {ops.onesweep_sort_tile()})"] = (
            lambda k, r, e: ops.onesweep_sort_rec(k, r, e, status))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--features", type=int, default=1 << 24)
    args = ap.parse_args()

    ops = require_hip_ops()
    F = args.features
    end_bit = max(1, (F - 1).bit_length())
    gen = SyntheticCriteo(num_features=F, seed=1234, device="cuda")
    fids = gen.batch(args.batch)[2]
    nnz = fids.numel()
    g = torch.Generator(device="cuda").manual_seed(1)
    uniform = torch.randint(0, 1 << end_bit, (nnz,), generator=g,
                            dtype=torch.int32, device="cuda")
    rec = torch.randint(-(1 << 31), 1 << 31, (nnz, 2), generator=g,
                        dtype=torch.int64, device="cuda").to(torch.int32)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    fns = variants(ops, status)

    for label, keys in (("flagship fids", fids), ("uniform keys", uniform)):
        want = ops.radix_sort_rec(keys, rec, end_bit)
        for name, fn in fns.items():
            got = fn(keys, rec, end_bit)
            same = (torch.equal(got[0], want[0])
                    and torch.equal(got[1], want[1]))
            if not same:
                raise SystemExit(f"{name} differs from rocprim default on "
                                 f"{label}")
        print(f"# {label}: nnz={nnz} end_bit={end_bit}, us per call (device "
              f"events, {args.reps} calls), all variants equal", flush=True)
        for p in range(args.passes):
            for name, fn in fns.items():
                t = event_us(lambda: fn(keys, rec, end_bit), args.reps)
                print(f"pass {p}: {name:44s} {t:7.1f}", flush=True)
    torch.cuda.synchronize()
    print(f"status word: {int(status.item())}")


if __name__ == "__main__":
    main()
