"""CPU checks of ``fm_oracles.py``: the oracles agree with ``fm_ref`` and
one CPU ``FMModel.train_step``, the exactness conditions hold on every case
list ``test_fm_kernels_gpu.py`` feeds to the GPU, and every wrong reference
listed in docs/TESTING.md differs from the right one on those same inputs
(on the exact set in at least one element, on the float set by more than
the bound)."""

import numpy as np
import pytest
import torch

import fm_oracles as fo
import kernel_oracles as ko
from lightctr_amd.models.fm import FMHyper, FMModel
from lightctr_amd.ops import fm_ref

T_TILE, S_SPLIT = 256, 32   # shape of the tile reduce at the time of writing;
#                             the GPU test reads both from the extension


def _fw(c, mutant=None):
    return fo.fm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"],
                             c["V"], mutant)


# ---------------------------------------------------------------------------
# exactness of every case list
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", fo.KS)
def test_exact_conditions_hold(K):
    for c in fo.row_cases(K):
        fo.assert_exact(c)
    for chunk in fo.APPLY_CHUNKS:
        cs = [fo.apply_case(K, chunk, 100 * K + 1),
              fo.apply_case(K, chunk, 100 * K + 2, with_perm=False)]
        cs += [fo.apply_case(K, chunk, 100 * K + 10 + j, nnz=n)
               for j, n in enumerate(fo.apply_nnz_cases(K, chunk))]
        for c in cs:
            fo.assert_exact_totals(c["sorted_fids"], c["gw_sorted"],
                                   c["gv_sorted"], c["F"], 1.0)
            # strictly increasing run heads, F-1 unused
            f = c["sorted_fids"]
            assert (f[1:] >= f[:-1]).all() and int(f[-1]) < c["F"] - 1
    for mode in (1, 2, 3):
        c = fo.fused_case(K, 300 * K + mode, mode)
        # the six edge gradients are not integers: each is a one-entry run,
        # whose total is the entry itself
        n = c["sorted_fids"].numel() - 6
        fo.assert_exact_totals(c["sorted_fids"][:n], c["gw_sorted"][:n],
                               c["gv_sorted"][:n], c["F"], 1.0)
    for ci, cap in enumerate((1, 2, 32, 256)):
        runs = fo.segment_runs(cap)
        c = fo.record_case(K, runs, 600 * K + cap, s=2 + ci)
        st = fo.int_state(c["F"], K, 9 * K + cap, True)
        gw, gv = fo.record_gradients(c, st["V"])
        fo.assert_exact_totals(c["sorted_fids"], gw, gv, c["F"],
                               2.0 ** -c["s"])
        pred = fo.spill_set(c["sorted_fids"], cap)
        assert 3 <= pred.numel() < torch.unique(c["sorted_fids"]).numel()
    for ci, cap in enumerate((1, 32, 64, T_TILE)):
        runs = fo.tile_runs(cap, T_TILE, S_SPLIT)
        c = fo.record_case(K, runs, 700 * K + 10 * cap, s=1 + ci)
        st = fo.int_state(c["F"], K, 11 * K + cap, True)
        gw, gv = fo.record_gradients(c, st["V"])
        fo.assert_exact_totals(c["sorted_fids"], gw, gv, c["F"],
                               2.0 ** -c["s"])
        pred = fo.spill_set(c["sorted_fids"], cap)
        assert 0 < pred.numel() < torch.unique(c["sorted_fids"]).numel()


def test_assert_exact_rejects_large_cases():
    """a case outside the conditions fails instead of passing loosely"""
    c = fo.row_case(4, [5000], 3)
    c["V"][:-1] = 2.0
    c["vals"][:] = 2.0
    with pytest.raises(AssertionError):
        fo.assert_exact(c)
    with pytest.raises(AssertionError):
        fo.check_value("x", torch.tensor([0.1]), torch.tensor([0.1],
                       dtype=torch.float64))


def test_run_placements():
    """the builders put runs where their comments say"""
    for b in (1, 3, 24, 96, 384):
        runs = fo.place_at([b])
        pos = np.cumsum(runs)
        i = len(runs) - 2
        assert pos[i] % b == 0 and runs[i] == 3 and runs[i + 1] == 5
    _, unit = fo.apply_units(16, -1)
    assert unit == 64
    assert fo.apply_units(32, -1) == ("walk", 384)
    assert fo.apply_units(32, -2) == ("scan", 8)
    runs = fo.tile_runs(32, T_TILE, S_SPLIT)
    starts = np.r_[0, np.cumsum(runs)[:-1]]
    ends = np.cumsum(runs)
    strad = [(a, b) for a, b in zip(starts, ends)
             if a // T_TILE != (b - 1) // T_TILE]
    assert strad and strad[0][0] % T_TILE != 0
    # a multi-unit piece that starts off a cell boundary and crosses it, and
    # another multi-unit piece in the same tile
    multi = [(a, b) for a, b in zip(starts, ends)
             if a // S_SPLIT != (b - 1) // S_SPLIT
             and a // T_TILE == (b - 1) // T_TILE]
    assert any(a % S_SPLIT for a, _ in multi)
    tiles = [a // T_TILE for a, _ in multi]
    assert any(tiles.count(t) >= 2 for t in tiles)


# ---------------------------------------------------------------------------
# the oracles against fm_ref and the CPU model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", fo.KS)
def test_oracles_match_fm_ref(K):
    for c in fo.row_cases(K) + [fo.float_row_case(K)]:
        ref = _fw(c)
        pred, sumVX = fm_ref.fm_forward_ref(c["row_ptr"], c["fids"],
                                            c["vals"], c["W"], c["V"])
        sv32 = ref["sumVX"][0].float()
        gw64, gv64, gvb = fo.fm_emit_ref(c["row_ptr"], c["fids"], c["vals"],
                                         c["V"], sv32, c["dpred"])
        totW, totV, tb = fo.fid_totals(c["fids"], gw64, gv64, c["F"],
                                       None if c["exact"] else gvb)
        gW, gV = fm_ref.fm_backward_ref(c["row_ptr"], c["fids"], c["vals"],
                                        c["V"], sv32, c["dpred"])
        live = torch.unique(c["fids"].long())
        if c["exact"]:
            fo.check_value("pred", pred, ref["pred"][0])
            fo.check_value("sumVX", sumVX, ref["sumVX"][0])
            fo.check_value("gW", gW[live], totW[live])
            fo.check_value("gV", gV[live], totV[live])
        else:
            ko.check_bound("pred", pred, *ref["pred"])
            ko.check_bound("sumVX", sumVX, *ref["sumVX"])
            ko.check_bound("gW", gW[live], totW[live], tb[0][live])
            ko.check_bound("gV", gV[live], totV[live], tb[1][live])
        assert torch.equal(fo.words_to_fids(fo.fid_words(c["fids"],
                                                         c["F"])), live)


def test_loss_oracle_matches_fm_ref():
    s = fo.loss_sweep()
    ref = fo.logloss_ref(s["z"], s["y"], s["scale"])
    loss, dpred = fm_ref.logloss_grad_ref(s["z"], s["y"], s["scale"])
    ko.check_bound("loss", loss, *ref["loss"])
    ko.check_bound("dpred", dpred, *ref["dpred"])
    # the sweep's rows make the forward produce z exactly
    V = torch.zeros(s["z"].numel() + 1, 4)
    fw = fo.fm_forward_ref(s["row_ptr"], s["fids"], s["vals"], s["W"], V)
    assert torch.equal(fw["pred"][0], s["z"].double())


def test_oracles_match_cpu_train_step():
    """One CPU FMModel.train_step on an exact case: pred is exact, so the
    model's loss lies within the loss bound of the oracle's, and after one
    Adagrad step from zero state (l2 = 0) nW = gW^2 with gW = sum d x: its
    root lies within the propagated dpred bound of the oracle's |gW|, and
    the rows with state are exactly the oracle's fid set."""
    K = 8
    c = fo.row_case(K, [3, 0, 9, 17, 1, 39], 11)
    c["V"] = c["V"] * 0.25          # keep pred inside the sweep's range
    c["W"] = c["W"] * 0.25
    F, B = c["F"], c["B"]
    live = torch.unique(c["fids"].long())
    m = FMModel(FMHyper(num_features=F, k=K, optimizer="adagrad", l2=0.0),
                device="cpu")
    m.W.copy_(torch.nan_to_num(c["W"]))
    m.V.copy_(torch.nan_to_num(c["V"]))
    loss = m.train_step(c["row_ptr"], c["fids"], c["vals"], c["label"])
    ref = _fw(c)
    z = ref["pred"][0]
    assert torch.equal(z.float().double(), z)
    ll = fo.logloss_ref(z.float(), c["label"], 1.0 / B)
    ko.check_bound("loss", loss, *ll["loss"])
    d, db = ll["dpred"]
    row, _, _ = ko.rows_pos(c["row_ptr"])
    x = c["vals"].double()
    z1 = lambda: torch.zeros(F, dtype=torch.float64)  # noqa: E731
    f = c["fids"].long()
    gW = z1().index_add_(0, f, d[row] * x)
    mag = z1().index_add_(0, f, (d[row] * x).abs())
    cnt = z1().index_add_(0, f, torch.ones_like(x))
    # err(d) x per entry, the sum rule, and the square / root roundings
    eg = z1().index_add_(0, f, db[row] * x) + (cnt + 3) * ko.U23 * mag
    ko.check_bound("sqrt nW", m.nW.sqrt()[live], gW.abs()[live], eg[live])
    assert torch.equal((m.nW > 0).nonzero().flatten(), live)


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_opt_step_matches_fm_ref(mode):
    K, F = 8, 64
    g = torch.Generator().manual_seed(mode)
    st = fo.int_state(F, K, mode, mode != 1)
    st = {k: v + 0.25 * torch.rand(v.shape, generator=g) for k, v in
          st.items()}
    gW, gV = torch.randn(F, generator=g), torch.randn(F, K, generator=g)
    ref = fo.opt_step_ref(st, gW, gV, mode)
    r = {k: v.clone() for k, v in st.items()}
    u = torch.arange(F, dtype=torch.int32)
    if mode == 1:
        fm_ref.adagrad_apply_ref(u, r["W"], r["V"], r["nW"], r["nV"],
                                 gW.clone(), gV.clone(), **fo.ADAGRAD)
    else:
        if mode == 3:
            r["zV"] = torch.zeros(F, K)
        fm_ref.ftrl_apply_ref(u, r["W"], r["V"], r["zW"], r["nW"], r["zV"],
                              r["nV"], gW.clone(), gV.clone(), **fo.FTRL,
                              v_adagrad=mode == 3,
                              v_lr=fo.V_ADAGRAD["lr"],
                              v_eps=fo.V_ADAGRAD["eps"],
                              v_l2=fo.V_ADAGRAD["l2"])
    for k in ref:
        # the fp32 torch path rounds like the kernel; allow its own roundings
        # the same bound again
        ko.check_bound(k, r[k], ref[k][0], 2 * ref[k][1] + ko.U23 *
                       ref[k][0].abs())


# ---------------------------------------------------------------------------
# wrong references
# ---------------------------------------------------------------------------
ROW_MUTANTS = ("droplast", "drop4G", "nohalf", "lin_all", "droplane", "noG")


@pytest.mark.parametrize("K", fo.KS)
def test_row_mutants_are_caught(K):
    """exact set: some element of some case differs; float set: outside the
    bound (x of the last and the 4G-th entry is boosted by FLOAT_BOOST, a
    power of two found here, until every one of them is)"""
    G = 64 // K
    cases = fo.row_cases(K)
    fc = fo.float_row_case(K)
    right = [_fw(c) for c in cases]
    fright = _fw(fc)
    for mu in ROW_MUTANTS:
        if mu == "noG" and G == 1:
            continue   # one feature group: there is no 1/G to omit
        keys = ("pred",) if mu in ("nohalf", "lin_all", "noG") else \
            ("pred", "sumVX")
        for key in keys:
            hit = any(ko.differs(_fw(c, mu)[key][0], r[key][0])
                      for c, r in zip(cases, right))
            assert hit, (K, mu, key)
            wrong = _fw(fc, mu)[key][0]
            assert ko.differs(wrong, fright[key][0], fright[key][1]), \
                (K, mu, key, "float")
    # the emit's self term, and the two permutations
    hit = fhit = False
    for c in cases + [fc]:
        sv32 = _fw(c)["sumVX"][0].float()
        a = fo.fm_emit_ref(c["row_ptr"], c["fids"], c["vals"], c["V"], sv32,
                           c["dpred"])
        b = fo.fm_emit_ref(c["row_ptr"], c["fids"], c["vals"], c["V"], sv32,
                           c["dpred"], "noself")
        if c["exact"]:
            hit |= ko.differs(a[1], b[1])
        else:
            fhit = ko.differs(a[1], b[1], a[2])
    assert hit and fhit
    c = cases[0]
    sv32 = _fw(c)["sumVX"][0].float()
    _, gv, _ = fo.fm_emit_ref(c["row_ptr"], c["fids"], c["vals"], c["V"],
                              sv32, c["dpred"])
    perm = torch.randperm(gv.shape[0],
                          generator=torch.Generator().manual_seed(K))
    assert ko.differs(gv[perm], gv), "pos ignored"


@pytest.mark.parametrize("K", fo.KS)
def test_run_mutants_are_caught(K):
    """perm ignored, last entry of a run dropped, first entry after a
    chunk / sub-chunk / entries-per-wave boundary dropped, and a run whose
    head lies in the previous unit taken as owned: each changes a total of
    the GPU test's own apply cases"""
    G = 64 // K
    for chunk in fo.APPLY_CHUNKS:
        kind, unit = fo.apply_units(K, chunk)
        c = fo.apply_case(K, chunk, 100 * K + 1)
        right = fo.apply_totals(c)
        units = [unit] + ([(unit + G - 1) // G] if kind == "walk" else [])
        muts = [("noperm", None), ("droplast", None)]
        muts += [(m, u) for u in units for m in ("dropfirst", "head_owned")]
        for mu, u in muts:
            wrong = fo.apply_totals(c, mu, u)
            assert ko.differs(wrong[0], right[0]) or \
                ko.differs(wrong[1], right[1]), (K, chunk, mu, u)
    # cap and tile boundaries on the segment inputs
    for cap, runs in ((32, fo.segment_runs(32)),
                      (T_TILE, fo.tile_runs(32, T_TILE, S_SPLIT))):
        c = fo.record_case(K, runs, 600 * K + cap)
        st = fo.int_state(c["F"], K, 9 * K + cap, False)
        gw, gv = fo.record_gradients(c, st["V"])
        cc = dict(c, gw_sorted=gw, gv_sorted=gv, gw=gw, gv=gv)
        right = fo.apply_totals(cc)
        for mu in ("dropfirst", "droplast"):
            wrong = fo.apply_totals(cc, mu, cap)
            assert ko.differs(wrong[1], right[1]) or \
                ko.differs(wrong[0], right[0]), (K, cap, mu)


@pytest.mark.parametrize("K", (4, 64))
def test_spill_mutants_are_caught(K):
    """a spilled run also updated in place leaves state that differs from
    the untouched state by more than the step's own bound; a spilled fid
    listed twice breaks the distinctness the GPU test asserts"""
    cap = 32
    c = fo.record_case(K, fo.segment_runs(cap), 600 * K + cap)
    for mode in (1, 2, 3):
        st = fo.int_state(c["F"], K, 9 * K + cap, mode != 1)
        gw, gv = fo.record_gradients(c, st["V"])
        totW, totV, _ = fo.fid_totals(c["sorted_fids"], gw, gv, c["F"])
        ref = fo.opt_step_ref(st, totW, totV, mode)
        pred = fo.spill_set(c["sorted_fids"], cap)
        assert pred.numel() >= 3
        for k in ref:
            assert ko.differs(ref[k][0][pred], st[k][pred]), (K, mode, k)
    twice = torch.cat([pred, pred[:1]])
    assert twice.unique().numel() != twice.numel()
    # the prediction itself: a run spills iff a multiple of cap is strictly
    # inside it
    fid, a, b = fo.run_bounds(c["sorted_fids"])
    brute = [int(f) for f, s, e in zip(fid, a, b)
             if any(s < m < e for m in range(0, int(e) + cap, cap))]
    assert brute == pred.tolist()


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_optimizer_mutants_are_caught(mode):
    """eps outside the root and l2 omitted leave the bound on the sparse
    apply's inputs (gradients of 1e-4); '<' for '<=' at the l1 edge flips
    the sign bit of w at g = +-l1 from zero state"""
    K = 8
    c = fo.sparse_case(K, 33, 5, mode != 1)
    st = c["state"]
    right = fo.opt_step_ref(st, c["gradW"], c["gradV"], mode)
    live = c["list"].long()
    if mode != 2:
        key = "W" if mode == 1 else "V"
        for mu in ("eps_out", "nol2"):
            wrong = fo.opt_step_ref(st, c["gradW"], c["gradV"], 1, mu) \
                if mode == 1 else \
                {"V": ko.adagrad_ref(st["V"], c["gradV"], st["nV"],
                                     **fo.V_ADAGRAD, mutant=mu)["W"]}
            assert ko.differs(wrong[key][0][live], right[key][0][live],
                              right[key][1][live]), (mode, mu)
    if mode != 1:
        wrong = fo.opt_step_ref(st, c["gradW"], c["gradV"], mode, "lt")
        e = live[:2]
        a, b = right["W"][0][e].float(), wrong["W"][0][e].float()
        assert (a == 0).all() and (b == 0).all()
        assert not torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_loss_mutants_are_caught():
    s = fo.loss_sweep()
    right = fo.logloss_ref(s["z"], s["y"], s["scale"])
    w = fo.logloss_ref(s["z"], s["y"], s["scale"], "noscale")
    assert ko.differs(w["dpred"][0], right["dpred"][0], right["dpred"][1])
    w = fo.logloss_ref(s["z"], s["y"], s["scale"], "clamped_loss")
    assert ko.differs(w["loss"][0], right["loss"][0], right["loss"][1])
