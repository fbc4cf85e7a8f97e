"""FwFM train step against the two models it sits between.

Shape of the Wide&Deep / DeepFM benchmark: B = 65536, 39 fields (one entry
per field, SyntheticCriteo), F = 2^24, Adagrad. Arms, all eager steps of
unchanged models except the first two:

    fwfm16  FwFMModel k = 16
    fwfm8   FwFMModel k = 8
    ffm8    FFMModel k = 8, bf16, its default modes: what FwFM is the cheap
            alternative to
    deepfm  DeepFMModel k = 16: fm_forward + fm_backward_emit and the shared
            sparse tail (sort, sorted apply, compact, Adagrad) with the MLP
            left out, as the cost of that tail

Default: `--pairs` rounds, each running every arm once for `--steps` steps
between device synchronisations (alternating, nothing overlapping); prints
the per-run times, their spread and one JSON line.

    python tools/bench_fwfm.py
    rocprofv3 --kernel-trace --stats -d out -- \\
        python tools/bench_fwfm.py --arms fwfm16 --pairs 1   # per-kernel
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
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--arms", default="fwfm16,fwfm8,ffm8,deepfm")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fwfm.py measures on the GPU; none found")

    from lightctr_amd.data.synthetic import SyntheticCriteo
    from lightctr_amd.models.deepfm import DeepFMHyper, DeepFMModel
    from lightctr_amd.models.ffm import FFMHyper, FFMModel
    from lightctr_amd.models.fwfm import FwFMHyper, FwFMModel
    from lightctr_amd.ops._extension import require_hip_ops, sort_ids

    dev, F, nf = "cuda:0", args.features, 39
    ops = require_hip_ops()

    def deepfm_sparse_step(m):
        """DeepFMModel.train_step's sparse half on the model's own state:
        the FM kernels and the tail, no concat and no MLP (dDeep == 0)"""
        def step(row_ptr, fields, fids, vals, labels):
            fm, sumVX = ops.fm_forward(row_ptr, fids, vals, m.W, m.E)
            _, dpred = ops.logloss_grad(fm, labels, 1.0 / labels.numel())
            gw, gv = ops.fm_backward_emit(row_ptr, fids, vals, m.E, sumVX,
                                          dpred, None)
            sorted_fids, perm = sort_ids(fids, F)
            ops.fm_sorted_apply(sorted_fids, perm, gw, gv, m.gradW, m.gradE,
                                m.touched)
            m.count.zero_()
            ops.bitmap_compact(m.touched, m.uniq, m.count)
            live = m.uniq[: min(m.uniq.numel(), fids.numel())]
            ops.fm_adagrad_apply(live, m.count, m.W, m.E, m.nW, m.nE,
                                 m.gradW, m.gradE, m.h.lr, m.h.eps, m.h.l2)
        return step

    def build(arm):
        if arm.startswith("fwfm"):
            return FwFMModel(FwFMHyper(num_features=F, num_fields=nf,
                                       k=int(arm[4:]), seed=1234),
                             device=dev).train_step
        if arm == "ffm8":
            return FFMModel(FFMHyper(num_features=F, num_fields=nf, k=8,
                                     seed=1234, dtype="bf16"),
                            device=dev).train_step
        assert arm == "deepfm", arm
        return deepfm_sparse_step(DeepFMModel(
            DeepFMHyper(num_features=F, num_fields=nf, k=16, hidden=(8,),
                        seed=1234), device=dev))

    arms = args.arms.split(",")
    steps = {a: build(a) for a in arms}
    gen = SyntheticCriteo(num_features=F, seed=1234, device=dev)
    pool = [gen.batch(args.batch) for _ in range(4)]

    def run(arm, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            steps[arm](*pool[i % len(pool)])
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for a in arms:
        run(a, args.warmup)
    times = {a: [] for a in arms}
    for _ in range(args.pairs):
        for a in arms:
            times[a].append(run(a, args.steps))
    out = {"batch": args.batch, "features": F, "fields": nf,
           "steps": args.steps}
    for a in arms:
        ms = [t / args.steps * 1e3 for t in times[a]]
        out[a + "_ms_per_step"] = [round(x, 4) for x in ms]
        out[a + "_spread"] = round((max(ms) - min(ms)) / min(ms), 4)
        out[a + "_examples_per_sec"] = round(
            args.batch * args.steps * len(ms) / sum(times[a]))
    for a in arms[1:]:
        out[f"{arms[0]}_over_{a}"] = round(
            sum(times[arms[0]]) / sum(times[a]), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
