"""FM backward_mode="segment" as the tile-local reduce (fm_segment_tile_rec):
every block finds the pieces of its own tile of sorted entries, short units
are summed by one subgroup, longer pieces are split over subgroups and
combined in LDS. GPU tests against the CPU reference path, the list-fed
"segment_list" mode and the step's invariants, on run-length shapes built
around the tile and split sizes the extension exports.

Tolerances are the ones of the other FM tests: atol=rtol=1e-4 against the
CPU reference path, atol=1e-5 between two GPU modes."""

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (optimizer, ftrl_v): Adagrad, FTRL, FTRL-W + Adagrad-V
PAIRINGS = (("adagrad", "ftrl"), ("ftrl", "ftrl"), ("ftrl", "adagrad"))
STATE = ("W", "V", "nW", "nV", "zW", "zV")
CAP = 256


def _tile_split():
    from lightctr_amd.ops import hip_ops

    return hip_ops.fm_segment_tile(), hip_ops.fm_segment_split()


def _shapes(shape, cap):
    """Run lengths of the sorted stream (fid i has runs[i] entries) for a
    named shape, from the built tile and split sizes."""
    T, S = _tile_split()
    table = {
        "distinct_1": lambda: [1],
        "distinct_tile_m1": lambda: [1] * (T - 1),
        "distinct_tile": lambda: [1] * T,
        "distinct_tile_p1": lambda: [1] * (T + 1),
        "distinct_2tile_p5": lambda: [1] * (2 * T + 5),
        # a run over a tile boundary / ending on one / starting on one
        "straddle": lambda: [T - 3, 7, 5],
        "ends_on_tile": lambda: [T - 4, 4, 9],
        "starts_on_tile": lambda: [T, 6],
        # every piece partial, one spilled run
        "one_fid": lambda: [3 * T + 1],
        # one whole piece (it starts on a multiple of cap) between singletons
        "whole_split_m1": lambda: [1] * cap + [S - 1] + [1] * 7,
        "whole_split": lambda: [1] * cap + [S] + [1] * 7,
        "whole_split_p1": lambda: [1] * cap + [S + 1] + [1] * 7,
        "whole_2split_p3": lambda: [1] * cap + [2 * S + 3] + [1] * 7,
        "whole_cap": lambda: [1] * cap + [cap] + [1] * 7,
        # the same off the split grid: first sub-range shorter than split
        "offgrid_split_m1": lambda: [1] * (cap + 5) + [S - 1] + [1] * 7,
        "offgrid_2split_p3": lambda: [1] * (cap + 5) + [2 * S + 3] + [1] * 7,
        # long pieces and singletons in one tile (at tile == cap the second
        # tile holds the singletons and the 70-entry piece)
        "mixed": lambda: ([cap] + [1] * 40 + [70]
                          + [1] * max(T - cap - 110, 0)),
    }
    return table[shape]()


DISTINCT = ("distinct_1", "distinct_tile_m1", "distinct_tile",
            "distinct_tile_p1", "distinct_2tile_p5")
BOUNDARY = ("straddle", "ends_on_tile", "starts_on_tile")
SPLITS = ("whole_split_m1", "whole_split", "whole_split_p1",
          "whole_2split_p3", "whole_cap", "offgrid_split_m1",
          "offgrid_2split_p3")
ALL_SHAPES = DISTINCT + BOUNDARY + ("one_fid",) + SPLITS + ("mixed",)


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


def _state(m):
    return {k: getattr(m, k) for k in STATE if hasattr(m, k)}


def _twin(h, mode, cap):
    m = FMModel(h, device=DEV)
    m.backward_mode = mode
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


def _assert_invariants(m, runs, cap):
    """Slabs and bitmap all-zero after the step; the spill count is the
    number of runs crossing a multiple of cap."""
    assert not m.gradW.any()
    assert not m.gradV.any()
    assert not m.touched.any()
    assert int(m.count) == _runs_crossing(runs, cap)


def _check_shape(shape, K, opt, ftrl_v, cap):
    """One step of the tile path against the CPU FMModel, the list path and
    the invariants."""
    runs = _shapes(shape, cap)
    F = 3 * len(runs) + 2
    row_ptr, fids, vals, labels = _csr_from_runs(runs, seed=10 + len(runs))
    h = FMHyper(num_features=F, k=K, optimizer=opt, seed=11, ftrl_v=ftrl_v)
    cpu = FMModel(h, device="cpu")
    tile = _twin(h, "segment", cap)
    lst = _twin(h, "segment_list", cap)
    for m in (tile, lst):
        m.W.copy_(cpu.W)
        m.V.copy_(cpu.V)
    batch = [t.to(DEV) for t in (row_ptr, fids, vals, labels)]
    lc = cpu.train_step(row_ptr, fids, vals, labels)
    lt = tile.train_step(*batch)
    ll = lst.train_step(*batch)
    tag = f"{shape} K={K} cap={cap} {opt}/{ftrl_v}"
    _assert_invariants(tile, runs, cap)
    _assert_invariants(lst, runs, cap)
    assert torch.allclose(lt.cpu(), lc, atol=1e-4, rtol=1e-4)
    assert torch.allclose(lt, ll, atol=1e-5)
    _assert_state_close(tile, cpu, 1e-4, 1e-4, tag + " vs cpu")
    _assert_state_close(tile, lst, 1e-5, 1e-5, tag + " vs list")


@pytest.mark.parametrize("opt,ftrl_v", PAIRINGS)
@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_tile_shapes(shape, opt, ftrl_v):
    T, _ = _tile_split()
    _check_shape(shape, 16, opt, ftrl_v, T if shape == "starts_on_tile"
                 else CAP)


@pytest.mark.parametrize("K", [4, 64])
@pytest.mark.parametrize("shape", SPLITS)
def test_tile_split_shapes_other_k(shape, K):
    """16 subgroups per wave (K=4) and one (K=64) on the split/combine
    path."""
    _check_shape(shape, K, "ftrl", "adagrad", CAP)


@pytest.mark.parametrize("cap", [8, "tile"])
@pytest.mark.parametrize("shape", BOUNDARY)
def test_tile_boundary_shapes_other_cap(shape, cap):
    T, _ = _tile_split()
    _check_shape(shape, 16, "ftrl", "adagrad", T if cap == "tile" else cap)


def test_cap_beyond_tile_takes_list_path():
    """segment_cap = 2 * tile cannot be tiled: the model routes it to the
    list path (the tile binding would refuse it) and still matches the
    CPU."""
    from lightctr_amd.ops import hip_ops

    T, _ = _tile_split()
    m = FMModel(FMHyper(num_features=16, k=16), device=DEV)
    m.segment_cap = 2 * T
    assert not m._cap_tiles(hip_ops)
    _check_shape("one_fid", 16, "ftrl", "adagrad", 2 * T)


def test_whole_pieces_deterministic():
    """No run crosses a cap multiple, so nothing goes through the slabs'
    atomics: twin models are bit-identical after 2 steps."""
    runs = _shapes("mixed", CAP)
    assert _runs_crossing(runs, CAP) == 0
    F = 3 * len(runs) + 2
    batch = [t.to(DEV) for t in _csr_from_runs(runs, seed=5)]
    h = FMHyper(num_features=F, k=16, optimizer="ftrl", seed=3)
    a = _twin(h, "segment", CAP)
    b = _twin(h, "segment", CAP)
    for _ in range(2):
        a.train_step(*batch)
        b.train_step(*batch)
    sa, sb = _state(a), _state(b)
    for name in sa:
        assert torch.equal(sa[name], sb[name]), name


def test_forward_train_reset():
    """reset=t is zeroed by the forward's launch; the outputs do not
    change."""
    from lightctr_amd.ops import hip_ops

    runs = [3, 1, 70, 17, 5]
    row_ptr, fids, vals, labels = (
        t.to(DEV) for t in _csr_from_runs(runs, seed=9))
    F, K = 3 * len(runs) + 2, 16
    g = torch.Generator().manual_seed(1)
    W = (torch.randn(F, generator=g) * 0.1).to(DEV)
    V = (torch.randn(F, K, generator=g) * 0.1).to(DEV)
    scale = 1.0 / labels.numel()
    want = hip_ops.fm_forward_train(row_ptr, fids, vals, W, V, labels, scale)
    t = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    got = hip_ops.fm_forward_train(row_ptr, fids, vals, W, V, labels, scale,
                                   reset=t)
    assert int(t) == 0
    assert len(got) == len(want) == 4
    for x, y in zip(got, want):
        assert torch.equal(x, y)


@pytest.mark.parametrize("opt,ftrl_v", PAIRINGS)
def test_tile_matches_segment_list(opt, ftrl_v):
    """3 steps on skewed data (longest run ~3000: whole and split pieces
    mixed): every parameter and state tensor agrees with the list-fed
    reduce."""
    from lightctr_amd.data.synthetic import SyntheticCriteo

    F = 1 << 15
    h = FMHyper(num_features=F, k=16, optimizer=opt, seed=31, ftrl_v=ftrl_v)
    a = _twin(h, "segment", CAP)
    b = _twin(h, "segment_list", CAP)
    gen = SyntheticCriteo(num_features=F, seed=77, device=DEV)
    for _ in range(3):
        row_ptr, _fields, fids, vals, labels = gen.batch(4096)
        la = a.train_step(row_ptr, fids, vals, labels)
        lb = b.train_step(row_ptr, fids, vals, labels)
        assert torch.allclose(la, lb, atol=1e-5)
        for m in (a, b):
            assert not m.gradW.any() and not m.gradV.any()
            assert not m.touched.any()
        assert int(a.count) == int(b.count)
    _assert_state_close(a, b, 1e-5, 1e-5, f"{opt}/{ftrl_v}")
