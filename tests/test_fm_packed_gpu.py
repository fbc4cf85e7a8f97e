"""FMModel(pack_linear=True): W, nW and zW are columns of one (W, nW, zW, 0)
cell per feature, the FM kernels read them at element stride 4 and the two
segment reduces move a whole cell as one float4.

A packed and an unpacked model must agree bit for bit wherever the result
does not depend on scheduling, i.e. on runs that never cross a multiple of
segment_cap (whole pieces). A run longer than segment_cap crosses one by
construction and goes through the slab atomics, whose order differs between
two runs of the same model; the fm_segment_tile() + 1 run therefore sits with
the spilled runs, which are compared with the CPU reference path at the
tolerance tests/test_fm_tile_gpu.py uses for that comparison
(atol = rtol = 1e-4)."""

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel
from lightctr_amd.ops._extension import sort_ids_rec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F, B = 600, 9
# opt_mode 1, 2, 3 as (optimizer, ftrl_v)
MODES = {1: ("adagrad", "ftrl"), 2: ("ftrl", "ftrl"), 3: ("ftrl", "adagrad")}
STATE = ("W", "nW", "zW", "V", "nV")
# (backward_mode, overlap_sort): the tile reduce behind the CSR-fed sort, and
# the list-fed reduce behind fm_forward_train
PATHS = (("segment", True), ("segment_list", False))


def _ops():
    from lightctr_amd.ops import hip_ops

    return hip_ops


def _batch(runs, seed):
    """B rows whose sorted fid stream has exactly these run lengths."""
    g = torch.Generator().manual_seed(seed)
    assert len(runs) <= F
    fids = torch.repeat_interleave(
        torch.arange(len(runs), dtype=torch.int32), torch.tensor(runs))
    nnz = fids.numel()
    fids = fids[torch.randperm(nnz, generator=g)]
    row_ptr = (torch.arange(B + 1) * nnz // B).to(torch.int32)
    vals = torch.rand(nnz, generator=g) + 0.5
    labels = torch.randint(0, 2, (B,), generator=g).float()
    return row_ptr, fids, vals, labels


def _whole_runs(cap):
    """Singletons, a run of exactly split entries, a cap-aligned run of cap
    entries; no run crosses a multiple of cap."""
    S = _ops().fm_segment_split()
    return [1] * cap + [S] + [1] * max(cap - S, 0) + [cap] + [1] * 3


def _spilled_runs(cap):
    T = _ops().fm_segment_tile()
    return [1] * 5 + [cap + 3] + [7] + [T + 1] + [1] * 2


def _model(K, mode, cap, path, pack, device=DEV):
    opt, ftrl_v = MODES[mode]
    h = FMHyper(num_features=F, k=K, optimizer=opt, ftrl_v=ftrl_v, seed=5)
    m = FMModel(h, device=device, pack_linear=pack)
    m.backward_mode, m.overlap_sort = path
    m.segment_cap = cap
    # a nonzero start for the linear state, the same in every model
    g = torch.Generator().manual_seed(17)
    m.W.copy_(torch.randn(F, generator=g) * 0.05)
    m.nW.copy_(torch.rand(F, generator=g))
    if hasattr(m, "zW"):
        m.zW.copy_(torch.randn(F, generator=g) * 0.1)
    return m


@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0])
@pytest.mark.parametrize("cap", [16, 256])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_twin_models_bit_identical(K, mode, cap, path):
    runs = _whole_runs(cap)
    packed = _model(K, mode, cap, path, True)
    plain = _model(K, mode, cap, path, False)
    assert packed.W.stride(0) == 4 and plain.W.is_contiguous()
    for step in range(3):
        batch = [t.to(DEV) for t in _batch(runs, seed=step)]
        lp = packed.train_step(*batch)
        lq = plain.train_step(*batch)
        assert torch.equal(lp, lq), step
    assert int(packed.count) == 0 and int(plain.count) == 0
    for name in STATE:
        if hasattr(plain, name):
            assert torch.equal(getattr(packed, name), getattr(plain, name)), \
                name
    assert not packed.lin[:, 3].any()
    if mode == 1:
        assert not packed.lin[:, 2].any()


@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0])
@pytest.mark.parametrize("cap", [16, 256])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_spilled_runs_match_cpu(K, mode, cap, path):
    runs = _spilled_runs(cap)
    packed = _model(K, mode, cap, path, True)
    cpu = _model(K, mode, cap, path, False, device="cpu")
    for step in range(3):
        batch = _batch(runs, seed=40 + step)
        lp = packed.train_step(*[t.to(DEV) for t in batch])
        lc = cpu.train_step(*batch)
        d = (lp.cpu() - lc).abs().max().item()
        print(f"step {step} loss max abs diff {d:.3e}")
        assert torch.allclose(lp.cpu(), lc, atol=1e-4, rtol=1e-4)
    crossing, a = 0, 0
    for r in runs:
        crossing += (a + r - 1) // cap != a // cap
        a += r
    assert crossing >= 2 and int(packed.count) == crossing
    for name in STATE:
        if hasattr(cpu, name):
            x, y = getattr(packed, name).cpu(), getattr(cpu, name)
            print(f"{name}: max abs diff {(x - y).abs().max().item():.3e}")
            assert torch.allclose(x, y, atol=1e-4, rtol=1e-4), name
    assert not packed.lin[:, 3].any()
    assert not packed.gradW.any() and not packed.gradV.any()


def test_empty_batch_leaves_lin_untouched():
    m = _model(16, 3, 256, PATHS[0], True)
    before = m.lin.clone()
    row_ptr = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    empty_i = torch.zeros(0, dtype=torch.int32, device=DEV)
    empty_f = torch.zeros(0, device=DEV)
    m.train_step(row_ptr, empty_i, empty_f, torch.zeros(B, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(m.lin, before)


# -- direct op calls ----------------------------------------------------------

SENT = 1234.5  # sentinel in the columns an op must not write


def _linear_state(layout, mode):
    """(table, W, nW, zW) for a layout: "flat" three contiguous tensors,
    "cell" columns 0..2 of one [F, 4] table, "mixed" a stride-4 W beside
    contiguous nW / zW (not a packed cell)."""
    g = torch.Generator().manual_seed(23)
    w = torch.randn(F, generator=g) * 0.05
    nw = torch.rand(F, generator=g)
    zw = torch.randn(F, generator=g) * 0.1
    table = torch.full((F, 4), SENT, device=DEV)
    if layout == "cell":
        W, nW, zW = table[:, 0], table[:, 1], table[:, 2]
    elif layout == "mixed":
        W = table[:, 0]
        nW, zW = torch.empty(F, device=DEV), torch.empty(F, device=DEV)
    else:
        W, nW, zW = (torch.empty(F, device=DEV) for _ in range(3))
    W.copy_(w)
    nW.copy_(nw)
    if mode != 1:
        zW.copy_(zw)
    return table, W, nW, (zW if mode != 1 else None)


@pytest.mark.parametrize("K", [4, 16, 64])
def test_fm_forward_strided_w(K):
    ops = _ops()
    g = torch.Generator().manual_seed(3)
    V = (torch.randn(F, K, generator=g) * 0.1).to(DEV)
    batch = [t.to(DEV) for t in _batch(_whole_runs(16), seed=9)]
    row_ptr, fids, vals, labels = batch
    _, flat, _, _ = _linear_state("flat", 2)
    table, col, _, _ = _linear_state("cell", 2)
    p1, s1 = ops.fm_forward(row_ptr, fids, vals, flat, V)
    p4, s4 = ops.fm_forward(row_ptr, fids, vals, col, V)
    assert torch.equal(p1, p4) and torch.equal(s1, s4)
    t1 = ops.fm_forward_train(row_ptr, fids, vals, flat, V, labels, 1.0 / B,
                              None)
    t4 = ops.fm_forward_train(row_ptr, fids, vals, col, V, labels, 1.0 / B,
                              None)
    for a, b in zip(t1, t4):
        assert torch.equal(a, b)
    assert (table[:, 3] == SENT).all()


@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_segment_tile_rec_layouts(K, mode):
    """Flat, packed-cell and mixed-stride linear state give equal results;
    the cell's fourth column, and its third in opt_mode 1, keep their
    sentinels."""
    ops = _ops()
    cap = 16
    g = torch.Generator().manual_seed(4)
    V0 = (torch.randn(F, K, generator=g) * 0.1).to(DEV)
    row_ptr, fids, vals, labels = [
        t.to(DEV) for t in _batch(_whole_runs(cap), seed=6)]
    knobs = (0.1, 1e-8, 1e-5, 0.0) if mode == 1 else (0.15, 1.0, 1e-4, 1e-4)
    out = {}
    for layout in ("flat", "cell", "mixed"):
        table, W, nW, zW = _linear_state(layout, mode)
        V, nV = V0.clone(), torch.zeros_like(V0)
        zV = torch.zeros_like(V0) if mode == 2 else None
        gradW, gradV = torch.zeros(F, device=DEV), torch.zeros_like(V0)
        spill = torch.zeros(8, dtype=torch.int32, device=DEV)
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        loss, dpred, sumVX, rec = ops.fm_forward_train(
            row_ptr, fids, vals, W, V, labels, 1.0 / B, None)
        sf, sr = sort_ids_rec(fids, rec, F)
        ops.fm_segment_tile_rec(sf, sr, sumVX, dpred, cap, gradW, gradV,
                                spill, count, W, V, nW, nV, zW, zV, mode,
                                *knobs, v_lr=0.1, v_eps=1e-8, v_l2=1e-5)
        assert int(count) == 0
        out[layout] = (loss, W.clone(), nW.clone(),
                       zW.clone() if zW is not None else None, V, nV)
        if layout == "cell":
            assert (table[:, 3] == SENT).all()
            if mode == 1:
                assert (table[:, 2] == SENT).all()
        if layout == "mixed":
            assert (table[:, 1:] == SENT).all()
    for layout in ("cell", "mixed"):
        for a, b in zip(out["flat"], out[layout]):
            assert (a is None and b is None) or torch.equal(a, b), layout
    # the step moved the linear state at all
    _, W0, nW0, _ = _linear_state("flat", mode)
    assert not torch.equal(out["flat"][2], nW0)
