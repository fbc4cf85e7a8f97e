"""Aux subsystem tests: ANN index, PCA, stats, ensembling, watchdog,
persistent buffer, shm hashtable, batch predictor."""

import os
import time

import pytest
import torch

from lightctr_amd.predict.ann_index import ANNIndex
from lightctr_amd.predict.predictor import BatchPredictor
from lightctr_amd.utils.ensembling import AdaBoost, VotingEnsemble
from lightctr_amd.utils.pca import SangerPCA, remove_top_pc
from lightctr_amd.utils.persistent import PersistentBuffer, ShmHashTable
from lightctr_amd.utils.stats import (normal_cdf, normal_cdf_inv,
                                      shuffle_pick_k, z_test)
from lightctr_amd.utils.watchdog import Watchdog

_REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ann_index_recall():
    g = torch.Generator().manual_seed(0)
    X = torch.randn(2000, 16, generator=g)
    idx = ANNIndex(X, n_trees=10, leaf_size=32, seed=1)
    hits = 0
    for i in range(20):
        q = X[i * 7] + torch.randn(16, generator=g) * 0.01
        approx, _ = idx.query(q, k=10, search_k=400)
        exact, _ = idx.query_exact(q, k=10)
        hits += len(set(approx.tolist()) & set(exact.tolist()))
    assert hits / 200 > 0.6, hits / 200


def test_sanger_pca_finds_top_direction():
    g = torch.Generator().manual_seed(1)
    basis = torch.tensor([[3.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    X = torch.randn(2000, 2, generator=g) @ basis
    pca = SangerPCA(3, 1, lr=0.05, seed=2)
    pca.fit(X, iters=100)
    c = pca.components()[0]
    assert abs(float(c[0])) > 0.97  # dominant axis = x
    Xr = remove_top_pc(X, 1)
    assert float(Xr[:, 0].var()) < float(X[:, 0].var()) * 0.1


def test_stats_helpers():
    assert abs(normal_cdf(0.0) - 0.5) < 1e-9
    assert abs(float(normal_cdf_inv(0.975)) - 1.95996) < 1e-3
    z, p = z_test(1.0, 0.0, 1.0, 1.0, 100, 100)
    assert p < 1e-10
    picks = shuffle_pick_k(100, 10, seed=3)
    assert picks.unique().numel() == 10


def test_voting_and_adaboost():
    g = torch.Generator().manual_seed(2)
    X = torch.randn(500, 2, generator=g)
    y = (X[:, 0] + 0.5 * X[:, 1] > 0).float()

    def make_stump(X, y, w):
        # best threshold stump on feature 0 or 1 under weights
        best = None
        for f in range(2):
            for thr in torch.linspace(-1, 1, 21):
                for sign in (1, -1):
                    pred = ((X[:, f] * sign) > thr * sign).float()
                    err = float((w * (pred != y).float()).sum())
                    if best is None or err < best[0]:
                        best = (err, f, float(thr), sign)
        _, f, thr, sign = best
        return lambda X: ((X[:, f] * sign) > thr * sign).float()

    ada = AdaBoost(make_stump, n_rounds=8).fit(X, y)
    acc = (ada.predict(X) == y).float().mean()
    assert acc > 0.9, float(acc)

    vote = VotingEnsemble([lambda X: torch.full((X.shape[0],), 0.8),
                           lambda X: torch.full((X.shape[0],), 0.4)],
                          weights=[1.0, 1.0])
    assert torch.allclose(vote.predict_proba(X),
                          torch.full((500,), 0.6))


def test_watchdog_detects_stale_rank():
    events = []
    # generous margins so a briefly-starved CI box cannot flake the test
    wd = Watchdog(2, soft_s=0.5, dead_s=1.0, period_s=0.1,
                  on_soft=lambda r: events.append(("soft", r)),
                  on_dead=lambda r: events.append(("dead", r))).start()
    for _ in range(16):
        wd.heartbeat(0)
        time.sleep(0.1)
    wd.stop()
    states = wd.snapshot()
    assert states[0] == "alive"
    assert states[1] == "dead"
    assert ("dead", 1) in events


def test_persistent_buffer_roundtrip(tmp_path):
    p = str(tmp_path / "buf.bin")
    b = PersistentBuffer(p, capacity=1024)
    b.write(b"hello ")
    b.write(b"world")
    b.flush()
    b.close()
    b2 = PersistentBuffer(p, capacity=1024)
    assert b2.read_all() == b"hello world"
    b2.clear()
    assert b2.size == 0
    b2.close()


def test_shm_hashtable(tmp_path):
    p = str(tmp_path / "shm.bin")
    t = ShmHashTable(p, slots_per_table=64, n_tables=4, value_dim=2)
    import numpy as np

    for k in range(50):
        assert t.put(k * 977 + 3, np.array([k, k * 0.5], dtype=np.float32))
    for k in range(50):
        v = t.get(k * 977 + 3)
        assert v is not None and abs(v[0] - k) < 1e-6
    assert t.get(123456789) is None
    # adjacent even/odd keys must not alias (round-1 advisor finding:
    # `key | 1` mapped 2 and 3 to the same slot key)
    assert t.put(2, np.array([20.0, 0.0], dtype=np.float32))
    assert t.put(3, np.array([30.0, 0.0], dtype=np.float32))
    assert t.get(2)[0] == 20.0 and t.get(3)[0] == 30.0
    # key 0 is representable (maps to stored 1, still nonzero)
    assert t.put(0, np.array([7.0, 0.0], dtype=np.float32))
    assert t.get(0)[0] == 7.0
    t.close()
    # reopen persists
    t2 = ShmHashTable(p, slots_per_table=64, n_tables=4, value_dim=2)
    v = t2.get(3)
    assert v is not None and v[0] == 30.0
    t2.close()


def test_batch_predictor_report():
    from lightctr_amd.data import LibffmDataset
    from lightctr_amd.data.synthetic import SyntheticCriteo
    from lightctr_amd.models.fm import FMHyper, FMModel

    gen = SyntheticCriteo(num_features=1 << 12, seed=9)
    row_ptr, fields, fids, vals, labels = gen.batch(512)
    ds = LibffmDataset(row_ptr, fields, fids, vals, labels)
    model = FMModel(FMHyper(num_features=1 << 12, k=8), device="cpu")
    bp = BatchPredictor(model, batch_size=128)
    pred = bp.predict_csr(ds)
    rep = bp.report(pred, ds.labels)
    for key in ("auc", "logloss", "accuracy", "precision", "recall", "f1"):
        assert key in rep


def test_cli_train_and_predict(tmp_path):
    from lightctr_amd.cli import main

    model_path = str(tmp_path / "m.pt")
    rc = main(["train", "--model", "fm", "--data", "synthetic", "--rows",
               "512", "--features", "8192", "--k", "8", "--epochs", "2",
               "--device", "cpu", "--save", model_path])
    assert rc == 0
    rc = main(["predict", "--model", "fm", "--data", "synthetic", "--rows",
               "256", "--features", "8192", "--k", "8", "--device", "cpu",
               "--load", model_path])
    assert rc == 0


def test_cli_predict_all_sparse_models(tmp_path):
    """Every sparse model family round-trips train --save -> predict
    --load --dump (the reference's FM_Predict covers its whole zoo)."""
    from lightctr_amd.cli import main

    for m in ("ffm", "nfm", "widedeep", "lr"):
        model_path = str(tmp_path / f"{m}.pt")
        dump_path = str(tmp_path / f"{m}.scores")
        rc = main(["train", "--model", m, "--data", "synthetic", "--rows",
                   "256", "--features", "4096", "--k", "8", "--epochs", "1",
                   "--batch", "128", "--device", "cpu", "--save", model_path])
        assert rc == 0, m
        rc = main(["predict", "--model", m, "--data", "synthetic", "--rows",
                   "128", "--features", "4096", "--k", "8", "--device",
                   "cpu", "--load", model_path, "--dump", dump_path])
        assert rc == 0, m
        with open(dump_path) as f:
            assert len(f.readlines()) == 128, m


def test_bundled_datasets_train():
    """The repo ships small example datasets like the reference's data/
    directory (train_sparse.csv libffm, train_dense.csv MNIST-style,
    vocab.txt); FM trains to a meaningful AUC on them end-to-end."""
    import os

    from lightctr_amd.data.libffm import load_libffm
    from lightctr_amd.models.fm import FMHyper, FMTrainer
    from lightctr_amd.utils.metrics import auc_score

    root = os.path.join(os.path.dirname(__file__), "..")
    tr_ds = load_libffm(os.path.join(root, "data", "train_sparse.csv"))
    te_ds = load_libffm(os.path.join(root, "data", "test_sparse.csv"))
    assert tr_ds.num_rows == 800 and te_ds.num_rows == 200
    F = max(tr_ds.num_features, te_ds.num_features)
    tr = FMTrainer(tr_ds, FMHyper(num_features=F, k=8, lr=0.3,
                                  optimizer="adagrad"),
                   device="cpu", batch_size=128, epochs=8)
    tr.train(log=None)
    p = tr.model.predict_proba(te_ds.row_ptr, te_ds.fids, te_ds.vals)
    auc = auc_score(p, te_ds.labels)
    assert auc > 0.72, f"bundled-data AUC too low: {auc}"

    from lightctr_amd.data.dense import load_dense_csv

    X, y = load_dense_csv(os.path.join(root, "data", "train_dense.csv"),
                          scale=1.0)
    assert X.shape == (400, 256) and y.numel() == 400


def test_libffm_native_python_parser_parity(tmp_path):
    """The native C++ parser and the Python fallback agree on a fuzzed
    file with blank lines, exponent floats and a max_rows cut."""
    import random

    import torch

    from lightctr_amd.data import libffm as lf
    from lightctr_amd.ops._extension import has_hip_ops

    if not has_hip_ops():
        import pytest

        pytest.skip("native extension not built")

    rnd = random.Random(5)
    path = tmp_path / "fuzz.csv"
    with open(path, "w") as f:
        for i in range(60):
            if i % 13 == 7:
                f.write("\n")  # blank line must be skipped
            n = rnd.randint(1, 9)
            toks = [str(rnd.randint(0, 1))]
            for _ in range(n):
                toks.append(f"{rnd.randint(0, 30)}:{rnd.randint(0, 5000)}:"
                            f"{rnd.uniform(-2, 2):.4g}")
            f.write(" ".join(toks) + ("  \n" if i % 5 == 0 else "\n"))

    for max_rows in (None, 17):
        nat = lf.load_libffm(str(path), max_rows=max_rows)  # native path

        # force the python fallback: temporarily hide the extension
        from lightctr_amd.ops import _extension as ext

        orig = ext.has_hip_ops
        ext.has_hip_ops = lambda: False
        try:
            py = lf.load_libffm(str(path), max_rows=max_rows)
        finally:
            ext.has_hip_ops = orig

        assert torch.equal(nat.row_ptr, py.row_ptr), max_rows
        assert torch.equal(nat.fields, py.fields)
        assert torch.equal(nat.fids, py.fids)
        assert torch.allclose(nat.vals, py.vals, atol=1e-6)
        assert torch.equal(nat.labels, py.labels)


def test_tools_cpu_smokes():
    """The measurement tools (train-to-AUC harness, GBM bench) run on CPU
    with tiny configs — keeps them from rotting between GPU rounds."""
    import subprocess
    import sys
    import os

    root = os.path.join(os.path.dirname(__file__), "..")
    r = subprocess.run(
        [sys.executable, os.path.join(root, "tools", "train_auc.py"),
         "--model", "fm", "--steps", "2", "--batch", "512", "--features",
         "20000", "--eval-rows", "1024"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    assert "held-out AUC" in r.stdout

    r = subprocess.run(
        [sys.executable, os.path.join(root, "tools", "bench_gbm.py"),
         "--rows", "2000", "--cols", "16", "--rounds", "3", "--depth", "3"],
        capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    assert "rounds/s" in r.stdout


def test_proc_file_split_tool(tmp_path):
    """The per-rank data sharder splits a libffm file into N shards that
    cover every row exactly once (the reference's offline splitter)."""
    import os
    import subprocess
    import sys

    src = tmp_path / "d.csv"
    lines = [f"{i % 2} 0:{i}:1\n" for i in range(103)]
    src.write_text("".join(lines))
    root = os.path.join(os.path.dirname(__file__), "..")
    r = subprocess.run(
        [sys.executable, os.path.join(root, "tools", "proc_file_split.py"),
         str(src), "4"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = []
    for i in range(1, 5):
        p = tmp_path / f"d_{i}.csv"
        assert p.exists()
        got += p.read_text().splitlines(keepends=True)
    assert sorted(got) == sorted(lines)


# ---------------------------------------------------------------------------
# §5.3 failure detection end-to-end: a rank dies mid-training; the
# surviving rank's TrainGuard detects the stalled collective, checkpoints
# its last completed step, and exits with the watchdog status; a restarted
# world resumes from the checkpoints. (Reference master.h:202-262
# heartbeat -> declare-dead, modernized to checkpoint-restart.)
# ---------------------------------------------------------------------------

def _failover_phase1_worker(rank, port, tmpdir):
    import os

    import torch.distributed as dist

    from conftest import make_random_csr
    from lightctr_amd.models.fm import FMHyper
    from lightctr_amd.parallel.sharded_fm import ShardedFMModel
    from lightctr_amd.utils.watchdog import TrainGuard

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    F = 512
    h = FMHyper(num_features=F, k=8, optimizer="adagrad", seed=5)
    model = ShardedFMModel(h, device="cpu")
    guard = TrainGuard(model, ckpt_path=f"{tmpdir}/ck{rank}",
                       soft_s=1.0, dead_s=3.0, period_s=0.25,
                       ckpt_every=1).start()
    row_ptr, fids, vals, labels = make_random_csr(
        B=32, F_total=F, seed=10 + rank, binary_vals=False)
    for step in range(10):
        if rank == 1 and step == 3:
            os._exit(17)  # simulated rank death (no checkpoint, no FIN)
        # gloo raises on the dead peer (run_step path); a hung transport
        # would instead trip the stall watchdog — same checkpoint-abort
        guard.run_step(model.train_step, row_ptr, fids, vals, labels)
    os._exit(0)  # unreachable for rank 0: it must die via the guard


def _failover_phase2_worker(rank, port, tmpdir):
    import os

    import torch
    import torch.distributed as dist

    from conftest import make_random_csr
    from lightctr_amd.models.fm import FMHyper
    from lightctr_amd.parallel.sharded_fm import ShardedFMModel
    from lightctr_amd.utils.watchdog import TrainGuard

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    F = 512
    h = FMHyper(num_features=F, k=8, optimizer="adagrad", seed=5)
    model = ShardedFMModel(h, device="cpu")
    guard = TrainGuard(model, ckpt_path=f"{tmpdir}/ck{rank}",
                       soft_s=5.0, dead_s=30.0, ckpt_every=0).start()
    resumed = guard.maybe_resume()
    assert resumed, f"rank {rank} found no checkpoint to resume"
    row_ptr, fids, vals, labels = make_random_csr(
        B=32, F_total=F, seed=10 + rank, binary_vals=False)
    for _ in range(2):
        loss = model.train_step(row_ptr, fids, vals, labels)
        assert torch.isfinite(loss).all()
        guard.step()
    guard.stop()
    os._exit(0)


def test_failover_checkpoint_restart(tmp_path):
    import torch.multiprocessing as mp

    from lightctr_amd.utils.watchdog import TrainGuard

    ctx = mp.get_context("spawn")
    tmpdir = str(tmp_path)
    # phase 1: rank 1 dies at step 3; rank 0 blocks in the step-4
    # all-to-all, its watchdog declares death, checkpoints, exits 3
    procs = [ctx.Process(target=_failover_phase1_worker,
                         args=(r, 29741, tmpdir)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert procs[1].exitcode == 17  # the killed rank
    assert procs[0].exitcode == TrainGuard.EXIT_CODE, procs[0].exitcode
    import os

    # rank 0 checkpointed on death; rank 1 has its ckpt_every=1 saves
    assert os.path.exists(f"{tmpdir}/ck0.shard0of2.pt")
    assert os.path.exists(f"{tmpdir}/ck1.shard1of2.pt")

    # phase 2: restart resumes both ranks from the checkpoints
    procs = [ctx.Process(target=_failover_phase2_worker,
                         args=(r, 29742, tmpdir)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert procs[0].exitcode == 0 and procs[1].exitcode == 0, \
        (procs[0].exitcode, procs[1].exitcode)


def test_batch_validators(monkeypatch):
    """LIGHTCTR_CHECK=1 batch validation (§5.2 invariant layer): catches
    malformed CSR, out-of-range ids/fields, non-finite values."""
    import importlib

    import lightctr_amd.utils.checks as checks

    monkeypatch.setenv("LIGHTCTR_CHECK", "1")
    importlib.reload(checks)
    rp = torch.tensor([0, 2, 4], dtype=torch.int32)
    fids = torch.tensor([1, 2, 3, 4], dtype=torch.int32)
    vals = torch.ones(4)
    checks.validate_csr_batch(rp, fids, vals, 10)  # ok
    try:
        checks.validate_csr_batch(rp, fids, vals, 3)  # fid 4 >= 3
        raise SystemExit("should have raised")
    except AssertionError:
        pass
    bad_vals = vals.clone()
    bad_vals[1] = float("nan")
    try:
        checks.validate_csr_batch(rp, fids, bad_vals, 10)
        raise SystemExit("should have raised")
    except AssertionError:
        pass
    fields = torch.tensor([0, 1, 5, 1], dtype=torch.int32)
    try:
        checks.validate_csr_batch(rp, fids, vals, 10, fields, 4)
        raise SystemExit("should have raised")
    except AssertionError:
        pass
    checks.validate_finite("state", torch.ones(3))
    try:
        checks.validate_finite("state", torch.tensor([1.0, float("inf")]))
        raise SystemExit("should have raised")
    except AssertionError:
        pass
    monkeypatch.setenv("LIGHTCTR_CHECK", "0")
    importlib.reload(checks)


def test_tools_importable():
    """Every tools/ script parses and imports its module-level deps (the
    GPU-only main()s are not run)."""
    import ast
    import pathlib

    tools = pathlib.Path(__file__).resolve().parent.parent / "tools"
    files = sorted(tools.glob("*.py"))
    assert files, tools
    for f in files:
        src = f.read_text()
        tree = ast.parse(src)  # syntax
        assert tree.body, f.name  # non-empty module


def test_bench_contract_cpu_smoke():
    """The driver's bench.py contract: runs on CPU (world 1) and prints
    exactly one JSON line with the required fields and honest dtype."""
    import json
    import subprocess
    import sys

    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "512", "--features", "16384", "--model", "fm"],
        capture_output=True, text=True, timeout=300, cwd=_REPO_ROOT)
    assert out.returncode == 0, out.stderr[-800:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
              "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config"):
        assert k in d, k
    assert d["steps"] == 2 and d["data"] == "synthetic"
    assert d["config"]["global_batch"] == 512


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs writes the last timed step's per-row loss as float
    .npy, identically on a second run with the same arguments (seeded
    inputs), and --full is accepted alongside it."""
    import json
    import subprocess
    import sys

    import numpy as np

    got = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "3",
             "--warmup", "1", "--batch", "256", "--features", "16384",
             "--dump-outputs", str(d)] + extra,
            capture_output=True, text=True, timeout=300, cwd=_REPO_ROOT)
        assert out.returncode == 0, out.stderr[-800:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout
        res = json.loads(lines[0])
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        files = sorted(p.name for p in d.iterdir())
        assert files == ["loss.npy"], files
        loss = np.load(d / "loss.npy")
        assert loss.dtype in (np.float32, np.float64)
        assert loss.shape == (256,) and np.isfinite(loss).all()
        assert loss.nbytes <= 64 << 20
        got.append(loss)
    assert np.array_equal(got[0], got[1])
