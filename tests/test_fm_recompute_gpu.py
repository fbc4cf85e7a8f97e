"""FM backward_mode="segment" with recomputed gradients: the training
forward (loss + per-entry (row, x) records fused in), the radix sort with
the records as payload, and the segment reduce that forms every entry's
gradient from its record. GPU tests (HIP kernels) against the unfused ops,
torch.sort, the CPU reference path and the emit-fed "segment_emit" mode.

Tolerances are the ones of the other FM tests: atol=rtol=1e-4 against the
CPU reference path, atol=1e-5 between two GPU modes."""

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel

from conftest import make_random_csr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (optimizer, ftrl_v): Adagrad, FTRL, FTRL-W + Adagrad-V
PAIRINGS = (("adagrad", "ftrl"), ("ftrl", "ftrl"), ("ftrl", "adagrad"))
STATE = ("W", "V", "nW", "nV", "zW", "zV")


def _state(m):
    return {k: getattr(m, k) for k in STATE if hasattr(m, k)}


def _assert_invariants(m, nnz):
    """Slabs and bitmap all-zero between steps; spill list within bound."""
    assert not m.gradW.any()
    assert not m.gradV.any()
    assert not m.touched.any()
    assert int(m.count) <= -(-nnz // m.segment_cap)


def _twin(h, mode, cap=None):
    m = FMModel(h, device=DEV)
    m.backward_mode = mode
    if cap is not None:
        m.segment_cap = cap
    return m


def _assert_state_close(a, b, atol, rtol, tag=""):
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for name in sa:
        x, y = sa[name].cpu(), sb[name].cpu()
        d = (x - y).abs().max().item()
        print(f"{tag} {name}: max abs diff {d:.3e}")
        assert torch.allclose(x, y, atol=atol, rtol=rtol), (tag, name, d)


# ---------------------------------------------------------------------------
# training forward == fm_forward + logloss_grad, records == (row, bits of x)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 16, 64])
def test_forward_train_matches_unfused(K):
    """B=6 ragged rows: an empty row, a row of one entry and a row of 70
    entries (at K=4, G=16 lanes groups: one turn of the 4-deep loop and a
    tail), non-binary vals."""
    from lightctr_amd.ops import hip_ops

    counts = torch.tensor([3, 0, 1, 70, 17, 5])
    B = counts.numel()
    nnz = int(counts.sum())
    F = 500
    g = torch.Generator().manual_seed(100 + K)
    row_ptr = torch.zeros(B + 1, dtype=torch.int32)
    row_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    fids = torch.randint(0, F, (nnz,), generator=g, dtype=torch.int32)
    vals = torch.rand(nnz, generator=g) * 2 - 0.7
    labels = torch.randint(0, 2, (B,), generator=g).float()
    W = torch.randn(F, generator=g) * 0.1
    V = torch.randn(F, K, generator=g) * 0.1
    row_ptr, fids, vals, labels, W, V = (
        t.to(DEV) for t in (row_ptr, fids, vals, labels, W, V))
    scale = 1.0 / B

    pred, sumVX0 = hip_ops.fm_forward(row_ptr, fids, vals, W, V)
    loss0, dpred0 = hip_ops.logloss_grad(pred, labels, scale)
    loss, dpred, sumVX, rec = hip_ops.fm_forward_train(
        row_ptr, fids, vals, W, V, labels, scale)
    assert torch.equal(sumVX, sumVX0)
    assert torch.equal(loss, loss0)
    assert torch.equal(dpred, dpred0)
    assert rec.shape == (nnz, 2) and rec.dtype == torch.int32
    rows = torch.repeat_interleave(torch.arange(B), counts).to(torch.int32)
    assert torch.equal(rec[:, 0].cpu(), rows)
    assert torch.equal(rec[:, 1].cpu(), vals.cpu().view(torch.int32))


# ---------------------------------------------------------------------------
# record sort
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("end_bit", [5, 24])
@pytest.mark.parametrize("n", [1, 37, 5000])
def test_record_sort(n, end_bit):
    """Keys equal torch.sort; per key the multiset of records survives."""
    from lightctr_amd.ops import hip_ops

    g = torch.Generator().manual_seed(n * 31 + end_bit)
    keys = torch.randint(0, 1 << end_bit, (n,), generator=g,
                         dtype=torch.int32)
    rec = torch.randint(-(1 << 31), (1 << 31) - 1, (n, 2), generator=g,
                        dtype=torch.int64).to(torch.int32)
    skeys, srec = hip_ops.radix_sort_rec(keys.to(DEV), rec.to(DEV), end_bit)
    skeys, srec = skeys.cpu(), srec.cpu()
    assert torch.equal(skeys, torch.sort(keys).values)
    want = sorted(zip(keys.tolist(), rec[:, 0].tolist(), rec[:, 1].tolist()))
    got = sorted(zip(skeys.tolist(), srec[:, 0].tolist(),
                     srec[:, 1].tolist()))
    assert got == want


# ---------------------------------------------------------------------------
# one step against the CPU FMModel
# ---------------------------------------------------------------------------
_STEP_BATCH = {}


def _step_batch():
    """make_random_csr(B=128, non-binary vals) with some fids repeated
    WITHIN a row (several entries of one row land in one piece)."""
    if not _STEP_BATCH:
        F = 20_000
        row_ptr, fids, vals, labels = make_random_csr(
            B=128, F_total=F, seed=42, binary_vals=False)
        rp = row_ptr.long()
        for r in range(0, 128, 5):  # rows have >= 5 entries
            fids[rp[r] + 1] = fids[rp[r]]
            fids[rp[r] + 3] = fids[rp[r]]
        _STEP_BATCH["b"] = (F, row_ptr, fids, vals, labels)
    return _STEP_BATCH["b"]


@pytest.mark.parametrize("opt,ftrl_v", PAIRINGS)
@pytest.mark.parametrize("K", [4, 8, 16, 32, 64])
def test_recompute_vs_cpu_one_step(K, opt, ftrl_v):
    F, row_ptr, fids, vals, labels = _step_batch()
    h = FMHyper(num_features=F, k=K, optimizer=opt, seed=7, ftrl_v=ftrl_v)
    cpu = FMModel(h, device="cpu")
    gpu = _twin(h, "segment")
    gpu.W.copy_(cpu.W)
    gpu.V.copy_(cpu.V)
    lc = cpu.train_step(row_ptr, fids, vals, labels)
    lg = gpu.train_step(row_ptr.cuda(), fids.cuda(), vals.cuda(),
                        labels.cuda())
    assert torch.allclose(lg.cpu(), lc, atol=1e-4, rtol=1e-4)
    _assert_state_close(gpu, cpu, 1e-4, 1e-4, f"K={K} {opt}/{ftrl_v}")
    _assert_invariants(gpu, fids.numel())


# ---------------------------------------------------------------------------
# boundary run-length shapes at segment_cap = 8
# ---------------------------------------------------------------------------
CAP = 8
# run lengths of the sorted stream (fid i has RUNS[i] entries)
BOUNDARY_RUNS = {
    "one_fid": [4096],            # every piece partial, one spilled run
    "all_distinct": [1] * 37,     # every piece whole, nothing spills
    "cap_run_aligned": [3, 5, 8, 2],   # [8,16): exactly one whole piece
    "cap_run_shifted": [8, 1, 8, 2],   # [9,17): split
    "ends_at_boundary": [5, 11, 3],    # [5,16): split, tail on a boundary
    "nnz_1": [1],
    "ragged_tail": [2, 3, 14],    # nnz=19, last run [5,19) reaches nnz
}


def _csr_from_runs(runs, seed):
    """CSR batch (rows of up to 4 entries) whose sorted fid stream has
    exactly the given run lengths, in this order; vals in [0.5, 1.5)."""
    g = torch.Generator().manual_seed(seed)
    fids = torch.repeat_interleave(
        torch.arange(len(runs), dtype=torch.int32) * 3 + 1,
        torch.tensor(runs))
    nnz = fids.numel()
    fids = fids[torch.randperm(nnz, generator=g)]
    B = -(-nnz // 4)
    row_ptr = torch.clamp(torch.arange(B + 1) * 4, max=nnz).to(torch.int32)
    vals = torch.rand(nnz, generator=g) + 0.5
    labels = torch.randint(0, 2, (B,), generator=g).float()
    return row_ptr, fids, vals, labels


def _runs_crossing(runs, cap):
    """Runs [a, b) of the sorted stream cut by a multiple of cap."""
    n, a = 0, 0
    for r in runs:
        b = a + r
        n += (b - 1) // cap != a // cap
        a = b
    return n


@pytest.mark.parametrize("opt,ftrl_v", PAIRINGS)
@pytest.mark.parametrize("shape", list(BOUNDARY_RUNS))
def test_recompute_boundary_shapes(shape, opt, ftrl_v):
    runs = BOUNDARY_RUNS[shape]
    F = 3 * len(runs) + 2
    row_ptr, fids, vals, labels = _csr_from_runs(runs, seed=10 + len(runs))
    nnz = fids.numel()
    h = FMHyper(num_features=F, k=16, optimizer=opt, seed=11, ftrl_v=ftrl_v)
    cpu = FMModel(h, device="cpu")
    gpu = _twin(h, "segment", cap=CAP)
    gpu.W.copy_(cpu.W)
    gpu.V.copy_(cpu.V)
    cpu.train_step(row_ptr, fids, vals, labels)
    gpu.train_step(row_ptr.cuda(), fids.cuda(), vals.cuda(), labels.cuda())
    _assert_invariants(gpu, nnz)
    assert int(gpu.count) == _runs_crossing(runs, CAP)
    _assert_state_close(gpu, cpu, 1e-4, 1e-4, f"{shape} {opt}/{ftrl_v}")


# ---------------------------------------------------------------------------
# against the emit-fed pipeline, and under graph capture
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("opt,ftrl_v", PAIRINGS)
def test_recompute_matches_segment_emit(opt, ftrl_v):
    """3 steps on skewed data (longest run ~3000: whole and split pieces
    mixed): every parameter and state tensor agrees with the emit-fed
    reduce."""
    from lightctr_amd.data.synthetic import SyntheticCriteo

    F = 1 << 15
    h = FMHyper(num_features=F, k=16, optimizer=opt, seed=31, ftrl_v=ftrl_v)
    a = _twin(h, "segment")
    b = _twin(h, "segment_emit")
    gen = SyntheticCriteo(num_features=F, seed=77, device=DEV)
    for _ in range(3):
        row_ptr, _fields, fids, vals, labels = gen.batch(4096)
        la = a.train_step(row_ptr, fids, vals, labels)
        lb = b.train_step(row_ptr, fids, vals, labels)
        assert torch.allclose(la, lb, atol=1e-5)
        _assert_invariants(a, fids.numel())
        _assert_invariants(b, fids.numel())
    _assert_state_close(a, b, 1e-5, 1e-5, f"{opt}/{ftrl_v}")


def test_recompute_graph_capture():
    """A captured step replayed twice == two eager steps of a twin."""
    F = 4096
    row_ptr, fids, vals, labels = make_random_csr(B=256, F_total=F, seed=5,
                                                  device=DEV,
                                                  binary_vals=False)
    fids[::3] = 17  # one hot run (~1900 entries) next to the singletons
    h = FMHyper(num_features=F, k=16, optimizer="ftrl", seed=3)
    a = _twin(h, "segment")
    b = _twin(h, "segment")
    # one eager step each first (allocator + kernels warm, same on both)
    a.train_step(row_ptr, fids, vals, labels)
    b.train_step(row_ptr, fids, vals, labels)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        a.train_step(row_ptr, fids, vals, labels)
    for _ in range(2):
        gr.replay()
        b.train_step(row_ptr, fids, vals, labels)
    torch.cuda.synchronize()
    _assert_invariants(a, fids.numel())
    _assert_state_close(a, b, 1e-5, 1e-5, "graph")
