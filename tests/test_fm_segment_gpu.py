"""FM backward_mode="segment": work list, per-piece reduce with the
optimizer fused in, spill apply. GPU tests (HIP kernels) against the sorted
mode, the CPU reference path and a few-line torch oracle of the work list."""

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel

from conftest import make_random_csr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (optimizer, ftrl_v): Adagrad, FTRL, FTRL-W + Adagrad-V
PAIRINGS = (("adagrad", "ftrl"), ("ftrl", "ftrl"), ("ftrl", "adagrad"))
STATE = ("W", "V", "nW", "nV", "zW", "zV")


def _worklist_ref(sorted_fids, cap):
    """Work-list definition on the CPU: entry e starts a piece if it is a
    run head or a multiple of cap. Returns (piece_start, whole, spilled):
    a piece is whole when it starts at a run head and ends at a run tail;
    the run of a head piece that is not whole spills."""
    s = sorted_fids.cpu().long()
    n = s.numel()
    e = torch.arange(n)
    head = torch.ones(n, dtype=torch.bool)
    head[1:] = s[1:] != s[:-1]
    starts = e[head | (e % cap == 0)]
    ends = torch.cat([starts[1:], torch.tensor([n])])
    is_head = head[starts]
    is_tail = (ends == n) | (s[ends.clamp(max=n - 1)] != s[ends - 1])
    return starts, is_head & is_tail, is_head & ~is_tail


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


@pytest.mark.parametrize("opt,ftrl_v", PAIRINGS)
def test_segment_matches_sorted(opt, ftrl_v):
    """3 steps on skewed data (longest run ~3000: whole and split pieces
    mixed): every parameter and state tensor agrees with the sorted mode."""
    from lightctr_amd.data.synthetic import SyntheticCriteo

    F = 1 << 15
    h = FMHyper(num_features=F, k=16, optimizer=opt, seed=31, ftrl_v=ftrl_v)
    a = _twin(h, "segment")
    b = _twin(h, "sorted")
    gen = SyntheticCriteo(num_features=F, seed=77, device=DEV)
    for _ in range(3):
        row_ptr, _fields, fids, vals, labels = gen.batch(4096)
        a.train_step(row_ptr, fids, vals, labels)
        b.train_step(row_ptr, fids, vals, labels)
        _assert_invariants(a, fids.numel())
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for name in sa:
        d = (sa[name] - sb[name]).abs().max().item()
        print(f"{opt}/{ftrl_v} {name}: max abs diff {d:.3e}")
        assert torch.allclose(sa[name], sb[name], atol=1e-5), (name, d)


@pytest.mark.parametrize("K", [4, 8, 16, 32, 64])
def test_segment_vs_cpu_one_step(K):
    """One identical step, segment mode on the GPU vs the CPU reference."""
    F = 20_000
    row_ptr, fids, vals, labels = make_random_csr(B=128, F_total=F, seed=42,
                                                  binary_vals=False)
    h = FMHyper(num_features=F, k=K, optimizer="adagrad", seed=7)
    cpu = FMModel(h, device="cpu")
    gpu = _twin(h, "segment")
    gpu.W.copy_(cpu.W)
    gpu.V.copy_(cpu.V)
    cpu.train_step(row_ptr, fids, vals, labels)
    gpu.train_step(row_ptr.cuda(), fids.cuda(), vals.cuda(), labels.cuda())
    assert torch.allclose(gpu.W.cpu(), cpu.W, atol=1e-4, rtol=1e-4)
    assert torch.allclose(gpu.V.cpu(), cpu.V, atol=1e-4, rtol=1e-4)
    _assert_invariants(gpu, fids.numel())


CAP = 8
# run lengths of the sorted stream (fid i has RUNS[i] entries), at CAP = 8
BOUNDARY_RUNS = {
    "one_fid": [4096],            # all pieces partial, one spill entry
    "all_distinct": [1] * 37,     # all pieces whole, empty spill list
    "cap_run_aligned": [3, 5, 8, 2],   # [8,16): exactly one whole piece
    "cap_run_shifted": [8, 1, 8, 2],   # [9,17): split
    "ends_at_boundary": [5, 11, 3],    # [5,16): split, tail on a boundary
    "nnz_1": [1],
    "ragged_tail": [2, 3, 14],    # nnz=19, last run [5,19) reaches nnz
}


def _csr_from_runs(runs, seed):
    """CSR batch (rows of up to 4 entries) whose sorted fid stream has
    exactly the given run lengths, in this order."""
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


@pytest.mark.parametrize("opt,ftrl_v", PAIRINGS)
@pytest.mark.parametrize("shape", list(BOUNDARY_RUNS))
def test_segment_boundary_shapes(shape, opt, ftrl_v):
    """Tiny streams at CAP=8 that hit every branch: the work list equals
    its torch definition, the spill list holds exactly the runs that cross
    a boundary, and one step equals the CPU reference path."""
    from lightctr_amd.ops import hip_ops
    from lightctr_amd.ops._extension import sort_ids

    runs = BOUNDARY_RUNS[shape]
    F = 3 * len(runs) + 2
    row_ptr, fids, vals, labels = _csr_from_runs(runs, seed=len(runs))
    nnz = fids.numel()

    # work list against the definition
    sorted_fids, _ = sort_ids(fids.cuda(), F)
    starts, whole, spilled = _worklist_ref(sorted_fids, CAP)
    junk = torch.full((1,), 123, dtype=torch.int32, device=DEV)
    piece_start, n_pieces = hip_ops.segment_worklist(sorted_fids, CAP, junk)
    P = int(n_pieces)
    assert P == starts.numel() <= nnz
    assert torch.equal(piece_start[:P].cpu().long(), starts)
    assert int(junk) == 0  # the pass resets the spill counter
    expect = {"one_fid": (0, 1), "all_distinct": (37, 0),
              "cap_run_aligned": (4, 0), "cap_run_shifted": (3, 1),
              "ends_at_boundary": (2, 1), "nnz_1": (1, 0),
              "ragged_tail": (2, 1)}[shape]
    assert (int(whole.sum()), int(spilled.sum())) == expect

    h = FMHyper(num_features=F, k=16, optimizer=opt, seed=11, ftrl_v=ftrl_v)
    cpu = FMModel(h, device="cpu")
    gpu = _twin(h, "segment", cap=CAP)
    gpu.W.copy_(cpu.W)
    gpu.V.copy_(cpu.V)
    cpu.train_step(row_ptr, fids, vals, labels)
    gpu.train_step(row_ptr.cuda(), fids.cuda(), vals.cuda(), labels.cuda())
    _assert_invariants(gpu, nnz)
    assert int(gpu.count) == int(spilled.sum())
    spilled_fids = sorted_fids.cpu().long()[starts[spilled]]
    got = gpu.uniq[: int(gpu.count)].cpu().long().sort().values
    assert torch.equal(got, spilled_fids.sort().values)
    sg, sc = _state(gpu), _state(cpu)
    for name in sg:
        assert torch.allclose(sg[name].cpu(), sc[name], atol=1e-4,
                              rtol=1e-4), \
            (name, (sg[name].cpu() - sc[name]).abs().max())


def test_segment_graph_capture():
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
    sa, sb = _state(a), _state(b)
    for name in sa:
        assert torch.allclose(sa[name], sb[name], atol=1e-5), \
            (name, (sa[name] - sb[name]).abs().max())
