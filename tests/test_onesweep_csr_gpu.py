"""onesweep_sort_csr: the onesweep sort fed by a CSR batch, its records made
by the row-walking histogram kernel (sort_kernels.hip,
onesweep_hist_rec_kernel). Keys and records must equal, element for element,
onesweep_sort_rec's on the same keys with the records built in numpy from
row_ptr; equal sorted outputs for one to four passes also mean the kernel's
digit histograms equal onesweep_hist_kernel's. Every batch has rows of uneven
length, empty ones included. The status word stays 0 throughout."""

import numpy as np
import pytest
import torch

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


def _row_counts(n, rng):
    """Uneven rows summing to n: an empty row first and last, two adjacent
    empty ones inside, lengths 0..130 (some past the 64 lanes of a wave)."""
    counts, left = [0], n
    while left > 0:
        c = min(int(rng.integers(0, 131)), left)
        counts.append(c)
        left -= c
        if len(counts) == 3:
            counts += [0, 0]
    counts.append(0)
    return np.asarray(counts, dtype=np.int64)


def _batch(n, end_bit, keys_kind, seed):
    rng = np.random.default_rng(seed)
    counts = _row_counts(n, rng)
    row_ptr = np.zeros(len(counts) + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(counts)
    assert row_ptr[-1] == n and (counts == 0).sum() >= 2
    if keys_kind == "equal":
        keys = np.full(n, (1 << end_bit) - 1, dtype=np.int64)
    else:
        keys = rng.integers(0, 1 << end_bit, n)
    vals = rng.standard_normal(n).astype(np.float32)
    rows = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    rec = np.stack([rows, vals.view(np.int32)], axis=1).reshape(-1, 2)
    return (torch.from_numpy(row_ptr).to(DEV),
            torch.from_numpy(keys.astype(np.int32)).to(DEV),
            torch.from_numpy(vals).to(DEV), torch.from_numpy(rec).to(DEV))


# n = a * T + b with T the built tile
SIZES = [(0, 1), (1, -1), (1, 0), (1, 1), (2, 3)]


@pytest.mark.parametrize("keys_kind", ["equal", "random"])
@pytest.mark.parametrize("end_bit", [1, 8, 9, 16, 17, 24, 31])
@pytest.mark.parametrize("a,b", SIZES)
def test_equals_sort_of_numpy_records(a, b, end_bit, keys_kind):
    from lightctr_amd.ops import hip_ops

    n = a * _tile() + b
    rp, kd, vd, rd = _batch(n, end_bit, keys_kind, 100 * n + end_bit)
    keys_before = kd.clone()
    skeys, srec = hip_ops.onesweep_sort_csr(rp, kd, vd, end_bit, _status())
    want_k, want_r = hip_ops.onesweep_sort_rec(kd, rd, end_bit, _status())
    assert skeys.shape == want_k.shape and srec.shape == want_r.shape
    assert torch.equal(skeys, want_k)
    assert torch.equal(srec, want_r)
    assert torch.equal(kd, keys_before)  # the input keys are never written
    # a wrong reference (row + 1 in every record) must not pass
    bad = rd.clone()
    bad[:, 0] += 1
    bad_r = hip_ops.onesweep_sort_rec(kd, bad, end_bit, _status())[1]
    assert not torch.equal(srec, bad_r)


def test_empty_input_launches_nothing():
    from lightctr_amd.ops import hip_ops

    rp = torch.zeros(4, dtype=torch.int32, device=DEV)
    kd = torch.zeros(0, dtype=torch.int32, device=DEV)
    vd = torch.zeros(0, device=DEV)
    skeys, srec = hip_ops.onesweep_sort_csr(rp, kd, vd, 24, _status())
    assert skeys.numel() == 0 and srec.shape == (0, 2)


def test_bad_arguments_raise():
    from lightctr_amd.ops import hip_ops

    rp, kd, vd, _ = _batch(100, 24, "random", 5)
    for end_bit in (0, 32):
        with pytest.raises(RuntimeError):
            hip_ops.onesweep_sort_csr(rp, kd, vd, end_bit, _status())
    with pytest.raises(RuntimeError):  # one value short
        hip_ops.onesweep_sort_csr(rp, kd, vd[:-1], 24, _status())
    with pytest.raises(RuntimeError):  # dtypes
        hip_ops.onesweep_sort_csr(rp, kd.long(), vd, 24, _status())
    with pytest.raises(RuntimeError):
        hip_ops.onesweep_sort_csr(rp, kd, vd.double(), 24, _status())
    with pytest.raises(RuntimeError):
        hip_ops.onesweep_sort_csr(rp.long(), kd, vd, 24, _status())
    with pytest.raises(RuntimeError):  # no offsets at all
        hip_ops.onesweep_sort_csr(rp[:0], kd, vd, 24, _status())
    with pytest.raises(RuntimeError):  # a status word of no ints
        hip_ops.onesweep_sort_csr(rp, kd, vd, 24, _status()[:0])
    with pytest.raises(RuntimeError):  # CPU tensors
        hip_ops.onesweep_sort_csr(rp.cpu(), kd.cpu(), vd.cpu(), 24, None)
    with pytest.raises(RuntimeError):
        hip_ops.onesweep_sort_csr(rp, kd, vd, 24, _status().cpu())
