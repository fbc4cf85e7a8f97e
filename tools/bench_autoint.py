"""AutoInt train step: the fused MFMA attention kernels against the layers
composed from tensor ops, with the xDeepFM and DCN-v2 steps beside them.

Shape of the Wide&Deep benchmark (bench.py --model widedeep): B = 65536,
39 fields, K = 16, hidden (256, 128), F = 2^24, the default (Adagrad) sparse
optimizer, L = 3 attention layers of 2 heads of 32. Arms:

    hip      AutoIntModel attn_impl="hip"   (ops/csrc/autoint_kernels.hip)
    torch    AutoIntModel attn_impl="torch" (ops/autoint_ref.py: Q, K, V, the
             scores and the probabilities materialised, each way)
    xdeepfm  XDeepFMModel, 2 CIN layers of 64 maps (ops/csrc/cin_kernels.hip)
    dcn2     DCNv2Model, 3 cross layers of rank 64 (ops/csrc/dcn2_kernels.hip)

Default: 4 alternating rounds (hip, torch, xdeepfm, dcn2, hip, ...), each
`--steps` eager steps between device synchronisations, nothing overlapping;
prints one JSON line with the times of every run and the number of pairs in
which hip is faster than torch.

    python tools/bench_autoint.py
    rocprofv3 --kernel-trace --stats -d out -- \\
        python tools/bench_autoint.py --arms hip --pairs 1 --steps 8  # kernels
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
    ap.add_argument("--attn-layers", type=int, default=3)
    ap.add_argument("--attn-heads", type=int, default=2)
    ap.add_argument("--attn-dim", type=int, default=32)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--arms", default="hip,torch,xdeepfm,dcn2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoint.py measures on the GPU; none found")

    from lightctr_amd.data.synthetic import SyntheticCriteo
    from lightctr_amd.models.dcn2 import DCNv2Hyper, DCNv2Model
    from lightctr_amd.models.autoint import AutoIntHyper, AutoIntModel
    from lightctr_amd.models.xdeepfm import XDeepFMHyper, XDeepFMModel

    dev = "cuda:0"
    arms = args.arms.split(",")
    kw = dict(num_features=args.features, num_fields=39, k=args.k,
              hidden=(256, 128), seed=1234)

    def build(arm):
        if arm == "dcn2":
            return DCNv2Model(DCNv2Hyper(**kw), device=dev)
        if arm == "xdeepfm":
            return XDeepFMModel(XDeepFMHyper(**kw), device=dev)
        return AutoIntModel(AutoIntHyper(attn_layers=args.attn_layers,
                                         attn_heads=args.attn_heads,
                                         attn_dim=args.attn_dim, **kw),
                            device=dev, attn_impl=arm)

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
           "attn_layers": args.attn_layers, "attn_heads": args.attn_heads,
           "attn_dim": args.attn_dim,
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
    for other in ("xdeepfm", "dcn2"):
        if "hip" in arms and other in arms:
            out["hip_over_" + other] = round(
                sum(times["hip"]) / sum(times[other]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
