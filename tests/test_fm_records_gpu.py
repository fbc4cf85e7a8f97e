"""fm_records: the (row, bits of x) records of a CSR batch made without the
forward (fm_kernels.hip, fm_records_kernel). They must equal, bit for bit,
the fourth output of fm_forward_train and a numpy construction from row_ptr.
The vals carry -0.0, a denormal, inf and a NaN with a nonzero payload: the
record holds the bits, not the number."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F, K = 500, 16
# -0.0, smallest denormal, +inf, quiet NaN with payload 0x1234
SPECIAL_BITS = np.array([0x80000000, 0x00000001, 0x7F800000, 0x7FC01234],
                        dtype=np.uint32)


def _batch(counts, seed):
    """row_ptr, fids, vals (random bits of finite floats with the special
    patterns spread over the front, the middle and the end)."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    nnz = int(counts.sum())
    row_ptr = np.zeros(len(counts) + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(counts)
    fids = rng.integers(0, F, nnz).astype(np.int32)
    bits = rng.standard_normal(nnz).astype(np.float32).view(np.uint32)
    for i, pos in enumerate(np.linspace(0, max(nnz - 1, 0), 8).astype(int)):
        if nnz:
            bits[pos] = SPECIAL_BITS[i % 4]
    return row_ptr, fids, bits.view(np.int32)


def _numpy_records(row_ptr, val_bits):
    rows = np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int32),
                     np.diff(row_ptr))
    return np.stack([rows, val_bits], axis=1).reshape(-1, 2)


def _check(counts, seed=0):
    from lightctr_amd.ops import hip_ops

    row_ptr, fids, val_bits = _batch(counts, seed)
    B = len(counts)
    rp = torch.from_numpy(row_ptr).to(DEV)
    fd = torch.from_numpy(fids).to(DEV)
    vd = torch.from_numpy(val_bits).view(torch.float32).to(DEV)
    assert np.array_equal(vd.cpu().view(torch.int32).numpy(), val_bits)
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(F, generator=g).to(DEV)
    V = (torch.randn(F, K, generator=g) * 0.01).to(DEV)
    label = torch.randint(0, 2, (B,), generator=g).float().to(DEV)

    rec = hip_ops.fm_records(rp, vd)
    want = _numpy_records(row_ptr, val_bits)
    assert rec.dtype == torch.int32 and tuple(rec.shape) == want.shape
    assert np.array_equal(rec.cpu().numpy(), want)
    fwd_rec = hip_ops.fm_forward_train(rp, fd, vd, W, V, label, 1.0 / B)[3]
    assert torch.equal(rec, fwd_rec)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_single_row(n):
    _check([n], seed=n)


def test_empty_rows_first_last_adjacent():
    _check([0, 7, 70, 0, 0], seed=1)
    _check([0, 3, 0, 0, 0], seed=2)


def test_empty_batch():
    _check([0, 0, 0], seed=3)


def test_small_random():
    rng = np.random.default_rng(67)
    counts = rng.integers(0, 131, 67)
    counts[5] = 0
    counts[40] = 130
    _check(counts, seed=4)


def test_bad_arguments_raise():
    from lightctr_amd.ops import hip_ops

    rp = torch.tensor([0, 2], dtype=torch.int32, device=DEV)
    vd = torch.ones(2, device=DEV)
    with pytest.raises(RuntimeError):
        hip_ops.fm_records(rp.long(), vd)
    with pytest.raises(RuntimeError):
        hip_ops.fm_records(rp, vd.double())
    with pytest.raises(RuntimeError):
        hip_ops.fm_records(rp.cpu(), vd)
    with pytest.raises(RuntimeError):
        hip_ops.fm_records(rp[:0], vd)
