"""onesweep_sort_csr with its first scatter pass reading the CSR batch
(sort_kernels.hip, onesweep_scatter_kernel<.., CSR = true>): the pass loads
fids and vals and finds each entry's row in row_ptr itself: a wave-wide search
for the row of its chunk's first entry, then a search per entry among the
starts of the 64 rows behind it, or over row_ptr where more rows than that
start in the chunk. Checked against numpy alone: a stable argsort of
fids & mask, records (row, bits of val) built from row_ptr by np.repeat. Keys
and records must be bit-equal and the status word stays 0. Every case also
shows that a reference with the row off by one at row boundaries is caught on
the same inputs. The tile is 4096 entries, a wave's chunk 512."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 4096
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


def test_tile_is_what_the_cases_assume():
    from lightctr_amd.ops import hip_ops

    assert hip_ops.onesweep_sort_tile() == TILE


def _uneven_counts(n, rng):
    """Rows of 0..130 entries summing to n, two adjacent empty ones inside."""
    counts, left = [], n
    while left > 0:
        c = min(int(rng.integers(0, 131)), left)
        counts.append(c)
        left -= c
        if len(counts) == 2:
            counts += [0, 0]
    return counts


def _vals(n, rng):
    """Normal draws; the first entries are -0.0, a denormal and an inf."""
    vals = rng.standard_normal(n).astype(np.float32)
    special = np.array([0x80000000, 0x00000001, 0x7F800000], dtype=np.uint32)
    vals[:min(n, 3)] = special.view(np.float32)[:min(n, 3)]
    return vals


def _keys(n, end_bit, kind, rng):
    if kind == "equal":
        return np.full(n, (1 << end_bit) - 1, dtype=np.int64).astype(np.int32)
    return rng.integers(0, 1 << end_bit, n).astype(np.int32)


def _check(counts, keys, vals, end_bit):
    from lightctr_amd.ops import hip_ops

    counts = np.asarray(counts, dtype=np.int64)
    B, n = len(counts), int(counts.sum())
    assert n == len(keys) == len(vals) and n > 0
    row_ptr = np.zeros(B + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(counts)
    rows = np.repeat(np.arange(B, dtype=np.int32), counts)
    order = np.argsort(keys.astype(np.int64) & ((1 << end_bit) - 1),
                       kind="stable")
    want_k = keys[order]
    want_r = np.stack([rows, vals.view(np.int32)], axis=1)[order]

    kd = torch.from_numpy(keys).to(DEV)
    skeys, srec = hip_ops.onesweep_sort_csr(
        torch.from_numpy(row_ptr).to(DEV), kd, torch.from_numpy(vals).to(DEV),
        end_bit, _status())
    assert skeys.shape == (n,) and srec.shape == (n, 2)
    got_k, got_r = skeys.cpu().numpy(), srec.cpu().numpy()
    assert np.array_equal(got_k, want_k)
    assert np.array_equal(got_r, want_r)
    assert np.array_equal(kd.cpu().numpy(), keys)  # the input is never written

    # a wrong reference must not pass: the first entry of every row counted
    # to the row before it (row_ptr[r] < idx in place of <=)
    bad = rows.copy()
    starts = row_ptr[:-1][counts > 0]
    bad[starts] = np.maximum(bad[starts] - 1, 0)
    if (bad != rows).any():
        bad_r = np.stack([bad, vals.view(np.int32)], axis=1)[order]
        assert not np.array_equal(got_r, bad_r)
    else:  # nothing to be off by: the batch starts in row 0 and never leaves
        assert rows.max() == 0


SIZES = [1, 63, 65, 4095, 4096, 4097, 8191, 8193, 3 * 4096 + 17]


@pytest.mark.parametrize("keys_kind", ["equal", "random"])
@pytest.mark.parametrize("end_bit", [1, 8, 9, 24, 31])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_bit_ranges(n, end_bit, keys_kind):
    rng = np.random.default_rng(1000 * n + end_bit)
    _check(_uneven_counts(n, rng), _keys(n, end_bit, keys_kind, rng),
           _vals(n, rng), end_bit)


def _shapes():
    rng = np.random.default_rng(7)
    short = lambda k: [int(c) for c in rng.integers(1, 40, k)]  # noqa: E731
    head = short(20)
    return {
        # rows end exactly at 512 (a wave's chunk), 4096 and 8192 (tiles)
        "tile_edge_on_row_edge": [500, 12, 3000, 584, 1, 4095, 0, 300],
        # one row over three tiles, short rows around it
        "row_of_9000": head + [9000] + short(20),
        "empty_run_5000": head + [0] * 5000 + short(200),
        "empty_first_and_last": [0, 0, 0] + short(150) + [0, 0, 0],
        "one_row": [2 * TILE + 5],
        "one_row_one_entry": [1],
        "rows_of_one": [1] * (TILE + 130),
        # 63 and 64 rows start in the first wave's chunk behind row 0: the
        # last batch whose row starts fit the wave's window, and the first
        # that takes the general search
        "window_63_rows": [449] + [1] * 63 + [600],
        "window_64_rows": [448] + [1] * 64 + [600],
        # more rows than entries, by far: the wave search's widest range
        "mostly_empty": ([0] * 997 + [1]) * 70 + [0] * 3000,
    }


SHAPES = _shapes()


@pytest.mark.parametrize("keys_kind", ["equal", "random"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_row_shapes(shape, keys_kind):
    counts = SHAPES[shape]
    n = sum(counts)
    rng = np.random.default_rng(len(counts) + n)
    _check(counts, _keys(n, 24, keys_kind, rng), _vals(n, rng), 24)


@pytest.mark.parametrize("end_bit", [8, 24])
def test_value_bits_are_carried_verbatim(end_bit):
    """Every entry has its own bit pattern: denormals on even entries, normal
    numbers on odd ones, then -0.0, inf and -inf."""
    n = 2 * TILE + 77
    rng = np.random.default_rng(end_bit)
    bits = np.arange(1, n + 1, dtype=np.uint32)
    bits[1::2] += 0x3F800000
    bits[[0, 1, 2]] = [0x80000000, 0x7F800000, 0xFF800000]
    assert len(np.unique(bits)) == n
    _check(_uneven_counts(n, rng), _keys(n, end_bit, "random", rng),
           bits.view(np.float32), end_bit)
