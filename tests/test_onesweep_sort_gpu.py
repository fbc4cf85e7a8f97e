"""onesweep_sort_rec: the single-purpose onesweep sort of the (fid, record)
stream (sort_kernels.hip). GPU tests against torch.sort(stable=True) on the
CPU with the records gathered through its indices: keys and records must be
equal element for element (the same stable permutation), and equal to
radix_sort_rec's. Records are random full-range int32 pairs (NaN patterns
included). Every test leaves the status word at 0: no look-back spin gave up.

The binding allocates its outputs, so "every element written" is asserted by
equality with the oracle."""

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel

from conftest import make_random_csr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_STATUS = {}


def _status():
    if not _STATUS:
        _STATUS["s"] = torch.zeros(1, dtype=torch.int32, device=DEV)
    return _STATUS["s"]


@pytest.fixture(autouse=True)
def _status_stays_zero():
    yield
    torch.cuda.synchronize()
    assert int(_status().item()) == 0


def _tile():
    from lightctr_amd.ops import hip_ops

    return hip_ops.onesweep_sort_tile()


def _records(n, g):
    return torch.randint(-(1 << 31), 1 << 31, (n, 2), generator=g,
                         dtype=torch.int64).to(torch.int32)


def _oracle(keys, rec):
    skeys, idx = torch.sort(keys.long(), stable=True)
    return skeys.to(torch.int32), rec[idx]


def _check(keys, rec, end_bit, against_rocprim=False):
    from lightctr_amd.ops import hip_ops

    kd, rd = keys.to(DEV), rec.to(DEV)
    skeys, srec = hip_ops.onesweep_sort_rec(kd, rd, end_bit, _status())
    want_k, want_r = _oracle(keys, rec)
    assert skeys.shape == kd.shape and srec.shape == rd.shape
    assert torch.equal(skeys.cpu(), want_k)
    assert torch.equal(srec.cpu(), want_r)
    assert torch.equal(kd.cpu(), keys)  # the input keys are never written
    if against_rocprim:
        rk, rr = hip_ops.radix_sort_rec(kd, rd, end_bit)
        assert torch.equal(skeys, rk)
        assert torch.equal(srec, rr)


# n = a * T + b with T the built tile
SIZES = [(0, 1), (0, 2), (0, 63), (0, 64), (0, 65), (1, -1), (1, 0), (1, 1),
         (2, 0), (3, 5), (64, 3)]


@pytest.mark.parametrize("a,b", SIZES)
def test_sizes(a, b):
    """end_bit 17: three passes, a partial last digit. 64T+3 makes the
    look-back chain long."""
    n = a * _tile() + b
    assert n <= 600_000
    g = torch.Generator().manual_seed(1000 + n)
    keys = torch.randint(0, 1 << 17, (n,), generator=g, dtype=torch.int32)
    _check(keys, _records(n, g), 17)


@pytest.mark.parametrize("end_bit", [1, 7, 8, 9, 16, 17, 24, 31])
def test_end_bits(end_bit):
    """1-4 passes, every ping-pong parity, partial last digits."""
    n = 3 * _tile() + 5
    g = torch.Generator().manual_seed(2000 + end_bit)
    keys = torch.randint(0, 1 << end_bit, (n,), generator=g,
                         dtype=torch.int64).to(torch.int32)
    _check(keys, _records(n, g), end_bit)


def _dist_keys(name, n, g):
    if name == "all_equal":
        return torch.full((n,), 0x5A5A5A, dtype=torch.int32)
    if name == "two_keys":
        pick = torch.randint(0, 2, (n,), generator=g)
        return torch.where(pick == 0, 3, 0xC00101).to(torch.int32)
    if name == "ascending":
        return torch.arange(n, dtype=torch.int32)
    if name == "descending":
        return torch.arange(n - 1, -1, -1, dtype=torch.int32)
    if name == "top_digit_only":
        return (torch.randint(0, 256, (n,), generator=g) << 16).to(
            torch.int32) | 0x1234
    if name == "bottom_digit_only":
        return torch.randint(0, 256, (n,), generator=g).to(
            torch.int32) | 0xAB4500
    raise KeyError(name)


@pytest.mark.parametrize("dist", ["all_equal", "two_keys", "ascending",
                                  "descending", "top_digit_only",
                                  "bottom_digit_only"])
def test_key_distributions(dist):
    n = 8 * _tile() + 1
    g = torch.Generator().manual_seed(len(dist))
    _check(_dist_keys(dist, n, g), _records(n, g), 24, against_rocprim=True)


def test_workload_skew():
    """SyntheticCriteo fids: 13 of the fields have a cardinality near 60."""
    from lightctr_amd.data.synthetic import SyntheticCriteo

    gen = SyntheticCriteo(num_features=1 << 24, seed=9)
    fids = gen.batch(512)[2]
    g = torch.Generator().manual_seed(4)
    _check(fids, _records(fids.numel(), g), 24, against_rocprim=True)


def test_back_to_back_calls():
    """Different n and end_bit on one stream with no sync between, larger
    then smaller: no call depends on what the previous one left."""
    from lightctr_amd.ops import hip_ops

    T = _tile()
    g = torch.Generator().manual_seed(77)
    cases = []
    for n, end_bit in ((5 * T + 7, 24), (T + 3, 9), (2 * T, 31), (65, 24),
                       (5 * T + 7, 24)):
        keys = torch.randint(0, 1 << end_bit, (n,), generator=g,
                             dtype=torch.int64).to(torch.int32)
        cases.append((keys, _records(n, g), end_bit))
    dev = [(k.to(DEV), r.to(DEV), e) for k, r, e in cases]
    torch.cuda.synchronize()
    outs = [hip_ops.onesweep_sort_rec(k, r, e, _status()) for k, r, e in dev]
    torch.cuda.synchronize()
    for (keys, rec, _e), (skeys, srec) in zip(cases, outs):
        want_k, want_r = _oracle(keys, rec)
        assert torch.equal(skeys.cpu(), want_k)
        assert torch.equal(srec.cpu(), want_r)


def test_graph_replay_on_changed_input():
    """One captured call, replayed three times on new contents: the memset
    and the in-kernel zeroing re-initialise every polled word per replay."""
    from lightctr_amd.ops import hip_ops

    n, end_bit = 6 * _tile() + 11, 24
    g = torch.Generator().manual_seed(5)
    kd = torch.zeros(n, dtype=torch.int32, device=DEV)
    rd = torch.zeros(n, 2, dtype=torch.int32, device=DEV)
    status = _status()
    hip_ops.onesweep_sort_rec(kd, rd, end_bit, status)  # warm, eager
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        skeys, srec = hip_ops.onesweep_sort_rec(kd, rd, end_bit, status)
    for _ in range(3):
        keys = torch.randint(0, 1 << end_bit, (n,), generator=g,
                             dtype=torch.int32)
        rec = _records(n, g)
        kd.copy_(keys)
        rd.copy_(rec)
        gr.replay()
        torch.cuda.synchronize()
        want_k, want_r = _oracle(keys, rec)
        assert torch.equal(skeys.cpu(), want_k)
        assert torch.equal(srec.cpu(), want_r)


def test_empty_input_launches_nothing():
    from lightctr_amd.ops import hip_ops

    kd = torch.zeros(0, dtype=torch.int32, device=DEV)
    rd = torch.zeros(0, 2, dtype=torch.int32, device=DEV)
    skeys, srec = hip_ops.onesweep_sort_rec(kd, rd, 24, _status())
    assert skeys.numel() == 0 and srec.shape == (0, 2)


def test_bad_arguments_raise():
    from lightctr_amd.ops import hip_ops

    n = 100
    kd = torch.zeros(n, dtype=torch.int32, device=DEV)
    rd = torch.zeros(n, 2, dtype=torch.int32, device=DEV)
    for end_bit in (0, 32):
        with pytest.raises(RuntimeError):
            hip_ops.onesweep_sort_rec(kd, rd, end_bit, _status())
    wide = torch.zeros(n, 4, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):  # non-contiguous rec
        hip_ops.onesweep_sort_rec(kd, wide[:, :2], 24, _status())
    with pytest.raises(RuntimeError):  # wrong rec shape
        hip_ops.onesweep_sort_rec(kd, wide, 24, _status())
    with pytest.raises(RuntimeError):
        hip_ops.onesweep_sort_rec(kd, rd[:-1], 24, _status())
    with pytest.raises(RuntimeError):  # CPU tensors
        hip_ops.onesweep_sort_rec(kd.cpu(), rd.cpu(), 24, None)
    with pytest.raises(RuntimeError):
        hip_ops.onesweep_sort_rec(kd, rd.cpu(), 24, _status())


def test_wrapper_routes():
    """sort_ids_rec: both impls agree; end_bit 32 goes to rocPRIM."""
    from lightctr_amd.ops._extension import sort_ids_rec

    n = _tile() + 9
    g = torch.Generator().manual_seed(8)
    keys = torch.randint(0, 1 << 20, (n,), generator=g, dtype=torch.int32)
    rec = _records(n, g)
    kd, rd = keys.to(DEV), rec.to(DEV)
    a = sort_ids_rec(kd, rd, 1 << 20, impl="onesweep", status=_status())
    b = sort_ids_rec(kd, rd, 1 << 20, impl="rocprim")
    c = sort_ids_rec(kd, rd, (1 << 31) + 5, impl="onesweep",
                     status=_status())
    want_k, want_r = _oracle(keys, rec)
    for skeys, srec in (a, b, c):
        assert torch.equal(skeys.cpu(), want_k)
        assert torch.equal(srec.cpu(), want_r)
    with pytest.raises(ValueError):
        sort_ids_rec(kd, rd, 1 << 20, impl="bitonic")


# ---------------------------------------------------------------------------
# model level: FMModel twins, sort_impl "rocprim" against "onesweep"
# ---------------------------------------------------------------------------
STATE = ("W", "V", "nW", "nV", "zW", "zV")


def _step_batch():
    """make_random_csr(B=128, non-binary vals) with some fids repeated
    within a row, as tests/test_fm_recompute_gpu.py builds it."""
    F = 20_000
    row_ptr, fids, vals, labels = make_random_csr(
        B=128, F_total=F, seed=42, binary_vals=False)
    rp = row_ptr.long()
    for r in range(0, 128, 5):  # rows have >= 5 entries
        fids[rp[r] + 1] = fids[rp[r]]
        fids[rp[r] + 3] = fids[rp[r]]
    return F, row_ptr, fids, vals, labels


@pytest.mark.parametrize("cap", [1 << 13, None])
def test_model_twins(cap):
    """Three steps of ftrl + adagrad-V at K=16. cap 2^13 exceeds nnz, so no
    run is cut and nothing spills: same permutation, no atomics, equal
    states. Default cap: spilled runs add with atomics, atol 1e-5 (the
    project's bound between two GPU modes)."""
    F, row_ptr, fids, vals, labels = _step_batch()
    assert cap is None or fids.numel() < cap
    batch = tuple(t.to(DEV) for t in (row_ptr, fids, vals, labels))
    h = FMHyper(num_features=F, k=16, optimizer="ftrl", seed=7,
                ftrl_v="adagrad")
    twins = []
    for impl in ("rocprim", "onesweep"):
        m = FMModel(h, device=DEV)
        m.sort_impl = impl
        if cap is not None:
            m.segment_cap = cap
        twins.append(m)
    for _ in range(3):
        la, lb = (m.train_step(*batch) for m in twins)
        assert torch.allclose(la, lb, atol=1e-5)
        if cap is not None:
            assert int(twins[0].count) == 0 and int(twins[1].count) == 0
    torch.cuda.synchronize()
    a, b = twins
    assert int(b.sort_status.item()) == 0
    for name in STATE:
        x, y = getattr(a, name), getattr(b, name)
        d = (x - y).abs().max().item()
        print(f"cap={cap} {name}: max abs diff {d:.3e}")
        if cap is not None:
            assert torch.equal(x, y), (name, d)
        else:
            assert torch.allclose(x, y, atol=1e-5, rtol=0), (name, d)
