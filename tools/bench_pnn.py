"""PNN train step: the fused MFMA inner-product-layer kernels against the layer
composed from tensor ops, with the Wide&Deep step beside them.

Shape of the Wide&Deep benchmark (bench.py --model widedeep): B = 65536,
39 fields, K = 16, hidden (256, 128), F = 2^24, the default (Adagrad) sparse
optimizer. The MLP's first layer is Dz = 1368 wide under PNN, 624 under
Wide&Deep. Arms:

    hip       PNNModel pnn_impl="hip"   (ops/csrc/pnn_kernels.hip)
    torch     PNNModel pnn_impl="torch" (ops/pnn_ref.py: bmm, triangular
              gather, pad and cast, 1024 rows at a time, each way)
    widedeep  WideDeepModel, the step the product layer is put into

Default: 4 alternating rounds (hip, torch, widedeep, hip, ...), each
`--steps` eager steps between device synchronisations, nothing overlapping;
prints one JSON line with the times of every run and the number of pairs in
which hip is faster than torch.

    python tools/bench_pnn.py
    rocprofv3 --kernel-trace --stats -d out -- \\
        python tools/bench_pnn.py --arms hip --pairs 1 --steps 8  # kernels
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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--arms", default="hip,torch,widedeep")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pnn.py measures on the GPU; none found")

    from lightctr_amd.data.synthetic import SyntheticCriteo
    from lightctr_amd.models.pnn import PNNHyper, PNNModel
    from lightctr_amd.models.wide_deep import WideDeepHyper, WideDeepModel

    dev = "cuda:0"
    arms = args.arms.split(",")
    kw = dict(num_features=args.features, num_fields=39, k=args.k,
              hidden=(256, 128), seed=1234)

    def build(arm):
        if arm == "widedeep":
            return WideDeepModel(WideDeepHyper(**kw), device=dev)
        return PNNModel(PNNHyper(**kw), device=dev, pnn_impl=arm)

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
    out = {"batch": args.batch, "features": args.features, "k": args.k,
           "steps": args.steps}
    for a in arms:
        out[a + "_ms_per_step"] = [round(t / args.steps * 1e3, 4)
                                   for t in times[a]]
        out[a + "_examples_per_sec"] = round(
            args.batch * args.steps * len(times[a]) / sum(times[a]))
    if "hip" in arms and "torch" in arms:
        wins = [h < t for h, t in zip(times["hip"], times["torch"])]
        out["hip_beats_torch_pairs"] = f"{sum(wins)} of {len(wins)}"
        out["hip_over_torch"] = round(sum(times["hip"]) /
                                      sum(times["torch"]), 4)
    if "hip" in arms and "widedeep" in arms:
        out["hip_over_widedeep"] = round(
            sum(times["hip"]) / sum(times["widedeep"]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
