"""DeepFM train step, fused kernels against the composed baseline.

Shape of the Wide&Deep benchmark (bench.py --model widedeep): B = 65536,
39 fields, K = 16, hidden (256, 128), F = 2^24, the default (Adagrad) sparse
optimizer. forward_impl="composed" launches only kernels that predate the
fused ones (fm_forward + embed_gather, fm_backward_emit +
embed_backward_emit + add), so it is the baseline; "fused" runs
deepfm_forward / deepfm_backward_emit.

Default: 4 + 4 alternating timed runs (fused, composed, fused, ...), each
`--steps` eager steps between device synchronisations, nothing overlapping;
prints the eight times, the per-pair verdicts and one JSON line. The fused
step "holds" when it is not slower in the majority of the pairs.

--layout field addresses the concat by field (deepfm_bag_* kernels, or
fm_forward + embed_bag_forward ... composed), --pooling picks sum or mean,
--multihot draws rows from SyntheticMultiHot (10 % of the fields missing,
4 fields with up to 8 values, shuffled tokens: ~48 entries a row) instead
of one entry per field in order. --arms names the two arms outright as
impl:layout[:pooling], e.g. the cost of field addressing on data that does
not need it:

    python tools/bench_deepfm.py
    python tools/bench_deepfm.py --arms fused:field,fused:position
    python tools/bench_deepfm.py --layout field --multihot
    rocprofv3 --kernel-trace --stats -d out -- \\
        python tools/bench_deepfm.py --arm fused --pairs 1   # per-kernel
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
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--arm", default="both",
                    choices=["both", "fused", "composed"],
                    help="one arm only (for a kernel trace)")
    ap.add_argument("--layout", default="position",
                    choices=["position", "field"])
    ap.add_argument("--pooling", default="sum", choices=["sum", "mean"])
    ap.add_argument("--multihot", action="store_true",
                    help="multi-hot rows with missing fields")
    ap.add_argument("--arms", default=None,
                    help="two arms as impl:layout[:pooling],... "
                         "(first against second)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deepfm.py measures on the GPU; none found")

    from lightctr_amd.data.synthetic import SyntheticCriteo, SyntheticMultiHot
    from lightctr_amd.models.deepfm import DeepFMHyper, DeepFMModel

    dev = "cuda:0"
    arms = ["fused", "composed"] if args.arm == "both" else [args.arm]
    if args.arms:
        arms = args.arms.split(",")

    def build(arm):
        parts = arm.split(":")
        impl = parts[0]
        layout = parts[1] if len(parts) > 1 else args.layout
        pooling = parts[2] if len(parts) > 2 else args.pooling
        hyper = DeepFMHyper(num_features=args.features, num_fields=39,
                            k=args.k, hidden=(256, 128), seed=1234,
                            layout=layout, pooling=pooling)
        return DeepFMModel(hyper, device=dev, forward_impl=impl)

    models = {a: build(a) for a in arms}
    if args.multihot:
        gen = SyntheticMultiHot(num_features=args.features, num_fields=39,
                                seed=1234, device=dev)
    else:
        gen = SyntheticCriteo(num_features=args.features, seed=1234,
                              device=dev)
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
    if args.layout != "position" or args.multihot or args.arms:
        out.update(layout=args.layout, pooling=args.pooling,
                   multihot=args.multihot,
                   entries_per_row=round(pool[0][2].numel() / args.batch, 2))
    for a in arms:
        ms = [t / args.steps * 1e3 for t in times[a]]
        out[a + "_ms_per_step"] = [round(x, 4) for x in ms]
        out[a + "_examples_per_sec"] = round(
            args.batch * args.steps * len(ms) / sum(times[a]))
    if len(arms) == 2:
        a, b = arms
        wins = [f <= c for f, c in zip(times[a], times[b])]
        first = "fused" if not args.arms else "first"
        out[first + "_not_slower_pairs"] = sum(wins)
        out[first + "_holds"] = sum(wins) * 2 > len(wins)
        out[f"{a}_over_{b}"] = round(sum(times[a]) / sum(times[b]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
