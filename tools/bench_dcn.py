"""DCN train step: the fused cross kernels against the cross layers composed
from tensor ops, with the Wide&Deep step beside them.

Shape of the Wide&Deep benchmark (bench.py --model widedeep): B = 65536,
39 fields, K = 16 (d = 624), hidden (256, 128), F = 2^24, the default
(Adagrad) sparse optimizer, L = 3 cross layers. Arms:

    hip       DCNModel cross_impl="hip"   (ops/csrc/dcn_kernels.hip)
    torch     DCNModel cross_impl="torch" (layer by layer, 3L passes)
    widedeep  WideDeepModel, the step without a cross term

Default: 4 + 4 alternating timed runs (hip, torch, widedeep, hip, ...), each
`--steps` eager steps between device synchronisations, nothing overlapping;
prints one JSON line with the times of every run, the number of pairs in
which hip is not slower than torch, and the least bytes the two cross
kernels have to move a step (x0 once each way, dDeep read and written, P).

    python tools/bench_dcn.py
    rocprofv3 --kernel-trace --stats -d out -- \\
        python tools/bench_dcn.py --arms hip --pairs 1 --steps 24  # kernels
"""

import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--features", type=int, default=1 << 24)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--cross-layers", type=int, default=3)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--arms", default="hip,torch,widedeep")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dcn.py measures on the GPU; none found")

    from lightctr_amd.data.synthetic import SyntheticCriteo
    from lightctr_amd.models.dcn import DCNHyper, DCNModel
    from lightctr_amd.models.wide_deep import WideDeepHyper, WideDeepModel

    dev = "cuda:0"
    arms = args.arms.split(",")
    kw = dict(num_features=args.features, num_fields=39, k=args.k,
              hidden=(256, 128), seed=1234)

    def build(arm):
        if arm == "widedeep":
            return WideDeepModel(WideDeepHyper(**kw), device=dev)
        return DCNModel(DCNHyper(cross_layers=args.cross_layers, **kw),
                        device=dev, cross_impl=arm)

    models = {a: build(a) for a in arms}
    gen = SyntheticCriteo(num_features=args.features, seed=1234, device=dev)
    pool = [gen.batch(args.batch) for _ in range(4)]

    def run(arm, steps):
        m = models[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            row_ptr, fields, fids, vals, labels = pool[i % len(pool)]
            m.train_step(row_ptr, fids, vals, labels, fields=fields)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for a in arms:
        run(a, args.warmup)
    times = {a: [] for a in arms}
    for _ in range(args.pairs):
        for a in arms:
            times[a].append(run(a, args.steps))
    B, d, L = args.batch, 39 * args.k, args.cross_layers
    out = {"batch": B, "features": args.features, "k": args.k,
           "cross_layers": L, "steps": args.steps,
           "cross_forward_min_bytes": B * (2 * d + 4 * (L + 2)),
           "cross_backward_min_bytes": B * (10 * d + 4 * (L + 2))}
    for a in arms:
        out[a + "_ms_per_step"] = [round(t / args.steps * 1e3, 4)
                                   for t in times[a]]
        out[a + "_examples_per_sec"] = round(
            B * args.steps * len(times[a]) / sum(times[a]))
    if "hip" in arms and "torch" in arms:
        wins = [h < t for h, t in zip(times["hip"], times["torch"])]
        out["hip_beats_torch_pairs"] = f"{sum(wins)} of {len(wins)}"
        out["hip_over_torch"] = round(sum(times["hip"]) /
                                      sum(times["torch"]), 4)
    if "hip" in arms and "widedeep" in arms:
        out["hip_over_widedeep"] = round(sum(times["hip"]) /
                                         sum(times["widedeep"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
