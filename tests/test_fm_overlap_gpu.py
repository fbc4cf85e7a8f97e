"""FMModel.overlap_sort: the record sort on a pool stream beside a forward
that writes no records (bindings.cpp, fm_forward_train_sorted) against the
earlier sequence (forward writes the records, the sort follows it).

Both hand the reduce a bit-identical sorted stream. Where no run of equal
fids crosses a multiple of segment_cap nothing spills, no atomic runs and the
twins stay bit-identical; where hot runs do cross, the spilled partial sums
arrive in any order and the bound is the project's 1e-5 between two GPU
modes (tests/test_fm_gpu.py)."""

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STATE = ("W", "V", "nW", "nV", "zW")
STEPS = 3


def _batch(B, per_row, F, seed):
    g = torch.Generator().manual_seed(seed)
    nnz = B * per_row
    row_ptr = (torch.arange(B + 1) * per_row).to(torch.int32)
    fids = torch.randint(0, F, (nnz,), generator=g, dtype=torch.int32)
    vals = torch.rand(nnz, generator=g) * 2
    labels = torch.randint(0, 2, (B,), generator=g).float()
    return tuple(t.to(DEV) for t in (row_ptr, fids, vals, labels))


def _small():
    """6 rows x 39 entries: nnz 234 <= segment_cap, nothing can spill."""
    return 300, _batch(6, 39, 300, seed=11)


def _twins(F, K, opt, modes=(True, False)):
    h = FMHyper(num_features=F, k=K, optimizer=opt, seed=7)
    out = []
    for mode in modes:
        m = FMModel(h, device=DEV)
        m.overlap_sort = mode
        out.append(m)
    for m in out[1:]:  # copied, not merely equally seeded
        m.W.copy_(out[0].W)
        m.V.copy_(out[0].V)
    return out


def _states(m):
    return [(n, getattr(m, n)) for n in STATE if hasattr(m, n)]


def _assert_identical(a, b):
    for (name, x), (_, y) in zip(_states(a), _states(b)):
        assert torch.equal(x, y), (name, (x - y).abs().max().item())
    assert int(a.count) == int(b.count)
    assert int(a.sort_status) == int(b.sort_status) == 0


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_twins_bit_identical_without_spill(K, opt):
    F, batch = _small()
    a, b = _twins(F, K, opt)
    assert batch[1].numel() <= a.segment_cap
    for _ in range(STEPS):
        la, lb = a.train_step(*batch), b.train_step(*batch)
        assert torch.equal(la, lb)
    torch.cuda.synchronize()
    _assert_identical(a, b)
    assert int(a.count) == 0


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_twins_close_with_spill(K, opt):
    """B = 320 x 39 entries over 64 fids: about three sort tiles, every run
    ~195 long and most crossing a cap multiple."""
    F = 64
    batch = _batch(320, 39, F, seed=12)
    a, b = _twins(F, K, opt)
    for _ in range(STEPS):
        la, lb = a.train_step(*batch), b.train_step(*batch)
        assert torch.allclose(la, lb, atol=1e-5, rtol=0)
    torch.cuda.synchronize()
    assert int(a.count) > 0  # the spill path did run
    assert int(a.count) == int(b.count)
    assert int(a.sort_status) == int(b.sort_status) == 0
    for (name, x), (_, y) in zip(_states(a), _states(b)):
        d = (x - y).abs().max().item()
        print(f"K={K} {opt} {name}: max abs diff {d:.3e}")
        assert torch.allclose(x, y, atol=1e-5, rtol=0), (name, d)


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_captured_step_bit_identical(K, opt):
    """The overlapped step captured once and replayed three times against
    the eager twin: the fork and the join are graph dependencies."""
    F, batch = _small()
    a, b, warm = _twins(F, K, opt, modes=(True, False, True))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm.train_step(*batch)  # kernels and allocator, on another model
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        la = a.train_step(*batch)
    for _ in range(STEPS):
        gr.replay()
        lb = b.train_step(*batch)
        torch.cuda.synchronize()
        assert torch.equal(la, lb)
    _assert_identical(a, b)


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_non_default_current_stream(K, opt):
    F, batch = _small()
    a, b = _twins(F, K, opt)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    losses = []
    with torch.cuda.stream(s):
        for _ in range(STEPS):
            losses.append(a.train_step(*batch))
    s.synchronize()
    for la in losses:
        assert torch.equal(la, b.train_step(*batch))
    torch.cuda.synchronize()
    _assert_identical(a, b)


def test_serial_arm_bit_identical():
    """overlap_sort="serial": the same launches on one stream."""
    F, batch = _small()
    a, b = _twins(F, 16, "ftrl", modes=("serial", False))
    for _ in range(STEPS):
        assert torch.equal(a.train_step(*batch), b.train_step(*batch))
    torch.cuda.synchronize()
    _assert_identical(a, b)


def test_empty_batch():
    """Rows without entries: a loss per row, no sort, no reduce, no update;
    no rows at all: nothing launched, the spill counter zeroed."""
    from lightctr_amd.ops import hip_ops

    F, K = 300, 16
    (a,) = _twins(F, K, "ftrl", modes=(True,))
    W0, V0 = a.W.clone(), a.V.clone()
    row_ptr = torch.zeros(5, dtype=torch.int32, device=DEV)
    fids = torch.zeros(0, dtype=torch.int32, device=DEV)
    vals = torch.zeros(0, device=DEV)
    labels = torch.tensor([0., 1., 1., 0.], device=DEV)
    loss = a.train_step(row_ptr, fids, vals, labels)
    torch.cuda.synchronize()
    # pred 0: loss log(2) through the fast-math log and exp
    assert torch.allclose(loss, torch.full_like(loss, 0.6931472), atol=1e-5)
    assert int(a.count) == 0 and int(a.sort_status) == 0
    assert torch.equal(a.W, W0) and torch.equal(a.V, V0)

    count = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    out = hip_ops.fm_forward_train_sorted(
        row_ptr[:1], fids, vals, a.W, a.V, labels[:0], 1.0, 9, reset=count,
        status=a.sort_status, overlap=True)
    assert [t.numel() for t in out] == [0, 0, 0, 0, 0]
    assert tuple(out[4].shape) == (0, 2)
    assert int(count) == 0


def test_bad_arguments_raise():
    from lightctr_amd.ops import hip_ops

    F, (row_ptr, fids, vals, labels) = _small()
    (m,) = _twins(F, 16, "ftrl", modes=(True,))
    st = m.sort_status

    def call(rp=row_ptr, f=fids, v=vals, y=labels, end_bit=9, status=st):
        return hip_ops.fm_forward_train_sorted(
            rp, f, v, m.W, m.V, y, 1.0, end_bit, reset=m.count,
            status=status, overlap=True)

    call()
    for end_bit in (0, 32):
        with pytest.raises(RuntimeError):
            call(end_bit=end_bit)
    with pytest.raises(RuntimeError):
        call(v=vals[:-1])
    with pytest.raises(RuntimeError):
        call(y=labels[:-1])
    with pytest.raises(RuntimeError):
        call(f=fids.long())
    with pytest.raises(RuntimeError):
        call(v=vals.double())
    with pytest.raises(RuntimeError):
        call(status=st[:0])
    torch.cuda.synchronize()
    assert int(st) == 0
