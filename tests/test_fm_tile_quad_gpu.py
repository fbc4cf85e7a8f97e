"""The tile reduce's float4 lane layout (fm_segment_tile_rec): a unit is
summed by K/4 lanes, lane q holding factors 4q..4q+3. GPU tests at the K the
other tile tests leave out, at unit counts around the number of subgroups of
a block, on integer inputs whose sums are exact (a factor in the wrong lane
of a float4 is then a bit difference), for twin determinism, and for the
binding's alignment check.

Shapes come from the tile, split and block size the extension exports.
Tolerances are the ones of test_fm_tile_gpu.py: atol=rtol=1e-4 against the
CPU reference path, atol=1e-5 between two GPU modes; the integer cases are
held to bit equality."""

import pytest
import torch

import fm_oracles as fo
import test_fm_kernels_gpu as tk
import test_fm_tile_gpu as tt
from lightctr_amd.models.fm import FMHyper, FMModel

pytestmark = pytest.mark.gpu

DEV = tt.DEV
CAP = tt.CAP


def _ops():
    from lightctr_amd.ops import hip_ops

    return hip_ops


def _nsg(K):
    """Units a block sums per turn: a unit takes K/4 lanes."""
    return _ops().fm_segment_threads() * 4 // K


def _check_runs(runs, K, cap, tag):
    """One step of the tile path on a batch with these run lengths against
    the CPU FMModel, the list path and the step's invariants."""
    F = 3 * len(runs) + 2
    row_ptr, fids, vals, labels = tt._csr_from_runs(runs, seed=10 + len(runs))
    h = FMHyper(num_features=F, k=K, optimizer="ftrl", seed=11,
                ftrl_v="adagrad")
    cpu = FMModel(h, device="cpu")
    tile = tt._twin(h, "segment", cap)
    lst = tt._twin(h, "segment_list", cap)
    for m in (tile, lst):
        m.W.copy_(cpu.W)
        m.V.copy_(cpu.V)
    batch = [t.to(DEV) for t in (row_ptr, fids, vals, labels)]
    lc = cpu.train_step(row_ptr, fids, vals, labels)
    lt = tile.train_step(*batch)
    ll = lst.train_step(*batch)
    tt._assert_invariants(tile, runs, cap)
    tt._assert_invariants(lst, runs, cap)
    assert torch.allclose(lt.cpu(), lc, atol=1e-4, rtol=1e-4)
    assert torch.allclose(lt, ll, atol=1e-5)
    tt._assert_state_close(tile, cpu, 1e-4, 1e-4, tag + " vs cpu")
    tt._assert_state_close(tile, lst, 1e-5, 1e-5, tag + " vs list")


@pytest.mark.parametrize("K", [8, 32])
@pytest.mark.parametrize("shape", tt.SPLITS + tt.BOUNDARY)
def test_split_and_boundary_shapes(shape, K):
    """Two lanes (K=8) and eight (K=32) per unit on the split/combine path
    and across tile boundaries."""
    T, _ = tt._tile_split()
    cap = T if shape == "starts_on_tile" else CAP
    _check_runs(tt._shapes(shape, cap), K, cap, f"{shape} K={K}")


@pytest.mark.parametrize("K", [4, 16, 64])
@pytest.mark.parametrize("units", ["nsg_m1", "nsg", "nsg_p1", "2nsg_p1",
                                   "full_units"])
def test_unit_counts_around_subgroups(units, K):
    """All-distinct fids one short of, exactly, one past and past twice the
    units a block takes per turn; and a tile of TILE/S runs of exactly S
    (every unit full, every piece one unit)."""
    T, S = tt._tile_split()
    n = _nsg(K)
    runs = {"nsg_m1": [1] * (n - 1), "nsg": [1] * n, "nsg_p1": [1] * (n + 1),
            "2nsg_p1": [1] * (2 * n + 1), "full_units": [S] * (T // S)}[units]
    _check_runs(runs, K, CAP, f"{units} K={K}")


@pytest.mark.parametrize("K", fo.KS)
def test_integer_inputs_match_list_reduce_bitwise(K):
    """Integer records, sumVX, V and state, dpred = +-2^-s: every sum is
    exact in any order (asserted by rec_totals), so the tile reduce and the
    list-fed reduce must leave bit-identical state on the `mixed` shape,
    whatever the lane layout of either."""
    runs = tt._shapes("mixed", CAP)
    assert tt._runs_crossing(runs, CAP) == 0
    for opt_mode in (2, 3):
        c = fo.record_case(K, runs, 900 * K + opt_mode, s=2)
        st = fo.int_state(c["F"], K, 13 * K + opt_mode, True)
        tk.rec_totals(c, st)
        a, gradW, gradV, _, cnt = tk.run_segment_rec(c, st, CAP, opt_mode, 4,
                                                     tile=True)
        b, _, _, _, _ = tk.run_segment_rec(c, st, CAP, opt_mode, 4)
        assert int(cnt) == 0
        assert not gradW.any() and not gradV.any()
        changed = False
        for name in st:
            assert torch.equal(a[name], b[name]), (K, opt_mode, name)
            changed |= not torch.equal(a[name].cpu(), st[name])
        assert changed


@pytest.mark.parametrize("K", [8, 32])
def test_whole_pieces_deterministic(K):
    """No run crosses a cap multiple, so nothing goes through the slabs'
    atomics: twin models are bit-identical after 2 steps."""
    runs = tt._shapes("mixed", CAP)
    assert tt._runs_crossing(runs, CAP) == 0
    F = 3 * len(runs) + 2
    batch = [t.to(DEV) for t in tt._csr_from_runs(runs, seed=5)]
    h = FMHyper(num_features=F, k=K, optimizer="ftrl", seed=3)
    a = tt._twin(h, "segment", CAP)
    b = tt._twin(h, "segment", CAP)
    for _ in range(2):
        a.train_step(*batch)
        b.train_step(*batch)
    sa, sb = tt._state(a), tt._state(b)
    for name in sa:
        assert torch.equal(sa[name], sb[name]), name


def test_alignment_is_checked():
    """sumVX starting one float into its buffer is refused before anything
    is launched; V[1:] of a longer table (rows of K floats, K % 4 == 0) is
    accepted and updated like a table of its own."""
    K, opt_mode = 8, 3
    c = fo.record_case(K, [3, 1, 5, 2], 77, s=2)
    st = fo.int_state(c["F"], K, 78, True)
    F, B = c["F"], c["B"]

    def run(V, sumVX):
        g = tk.up_state(st)
        g["V"] = V
        gradW, gradV, _ = tk.slabs(F, K)
        _, spill, cnt = tk.spill_buffers(4)
        _ops().fm_segment_tile_rec(
            c["sorted_fids"].to(DEV), c["rec"].to(DEV), sumVX,
            c["dpred"].to(DEV), CAP, gradW, gradV, spill, cnt, g["W"], V,
            g["nW"], g["nV"], g.get("zW"), g.get("zV"), opt_mode,
            *fo.opt_args(opt_mode))
        return g

    sumVX = c["sumVX"].to(DEV)
    V = st["V"].to(DEV)
    long_buf = torch.zeros(B * K + 1, device=DEV)
    off = long_buf[1:].view(B, K)
    off.copy_(sumVX)
    assert off.is_contiguous() and off.data_ptr() % 16 == 4
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        run(V.clone(), off)

    want = run(V.clone(), sumVX)
    table = torch.zeros(F + 1, K, device=DEV)
    table[1:] = V
    got = run(table[1:], sumVX)
    assert not table[0].any()
    assert not torch.equal(want["V"], V)
    for name in st:
        assert torch.equal(got[name], want[name]), name
