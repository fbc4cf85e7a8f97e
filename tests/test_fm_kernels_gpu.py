"""Parity tests for the FM kernels (fm_kernels.hip) against the float64
oracles of ``fm_oracles.py``.

Main set: small-integer inputs on which every FM quantity except the loss
is exact in fp32 in any summation, atomic or tiling order (the rule and its
magnitude conditions are stated in ``fm_oracles.py`` and asserted for every
case), so the comparisons are bit or value equality. A float set per K keeps
real rounding in view under derived bounds; the optimizers are held to
``adagrad_ref`` / ``ftrl_ref`` applied once to the exact total gradient; the
loss is swept over exact arguments. Shapes follow the kernels' loops (row
lengths around G = 64/K and the four-trip unroll, runs around the walk's
chunk, sub-chunk and batch, the scans' entries per wave, the pieces' cap,
the tile and its split), not the workload. ``test_fm_oracles.py`` shows on
the CPU that the wrong references listed in docs/TESTING.md differ on these
same inputs. The binding checks are exercised at the end: every bad argument
raises before anything is launched.
"""

import numpy as np
import pytest
import torch

import fm_oracles as fo
import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def view_on_gpu(t, fill):
    """t as a view inside a longer device buffer filled with `fill`"""
    buf, o = fo.padded(t, fill)
    return buf.to(DEV)[o:o + t.numel()]


def up_row(c):
    """Upload a row case: fids / vals are views; the ints around fids name
    fid F-1 (NaN rows of W and V), the floats around vals are NaN"""
    return {"row_ptr": c["row_ptr"].to(DEV),
            "fids": view_on_gpu(c["fids"], c["F"] - 1),
            "vals": view_on_gpu(c["vals"], NAN),
            "W": c["W"].to(DEV), "V": c["V"].to(DEV),
            "dpred": c["dpred"].to(DEV), "label": c["label"].to(DEV)}


def poison_i32(shape):
    p = torch.full(shape, -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    del p


def slabs(F, K):
    return (torch.zeros(F, device=DEV), torch.zeros(F, K, device=DEV),
            torch.zeros((F + 63) // 64, dtype=torch.int64, device=DEV))


def run_forward(g, B, K):
    ko.poison((B,), torch.float32, DEV)
    ko.poison((B, K), torch.float32, DEV)
    return ops().fm_forward(g["row_ptr"], g["fids"], g["vals"], g["W"],
                            g["V"])


def run_emit(g, sumVX, nnz, K, pos=None):
    ko.poison((nnz,), torch.float32, DEV)
    ko.poison((nnz, K), torch.float32, DEV)
    return ops().fm_backward_emit(g["row_ptr"], g["fids"], g["vals"],
                                  g["V"], sumVX, g["dpred"], pos)


def check_rows(name, out, ref, rows):
    """check_bound of (ref64, bound) on the given rows only"""
    r, b = ref
    if rows.numel():
        ko.check_bound(name, out.detach().cpu()[rows], r[rows], b[rows])


def check_rows_bits(name, out, expect, rows):
    ko.check_bits(name, out.detach().cpu()[rows], expect[rows])


def others(F, fids):
    m = torch.ones(F, dtype=torch.bool)
    m[fids] = False
    return m.nonzero().flatten()


# ---------------------------------------------------------------------------
# row kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", fo.KS)
def test_forward_exact(K):
    """pred and sumVX bit for bit; fm_forward_train's sumVX is fm_forward's,
    its loss / dpred are logloss_grad of fm_forward's pred, its records are
    {row, bits of x}"""
    for i, c in enumerate(fo.row_cases(K)):
        fo.assert_exact(c)
        g = up_row(c)
        B, nnz = c["B"], c["fids"].numel()
        ref = fo.fm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"],
                                c["V"])
        pred, sumVX = run_forward(g, B, K)
        name = f"K{K}.case{i}"
        ko.check_bits(name + ".pred", pred, fo.exact32(ref["pred"][0]))
        ko.check_bits(name + ".sumVX", sumVX, fo.exact32(ref["sumVX"][0]))

        scale = 1.0 / 8
        for _ in range(2):
            ko.poison((B,), torch.float32, DEV)
        ko.poison((B, K), torch.float32, DEV)
        poison_i32((nnz, 2))
        loss, dpred, sumVX2, rec = ops().fm_forward_train(
            g["row_ptr"], g["fids"], g["vals"], g["W"], g["V"], g["label"],
            scale, None)
        for _ in range(2):
            ko.poison((B,), torch.float32, DEV)
        loss1, dpred1 = ops().logloss_grad(pred, g["label"], scale)
        ko.check_bits(name + ".train.sumVX", sumVX2, sumVX.cpu())
        ko.check_bits(name + ".train.loss", loss, loss1.cpu())
        ko.check_bits(name + ".train.dpred", dpred, dpred1.cpu())
        row, _, _ = ko.rows_pos(c["row_ptr"])
        rec_ref = torch.stack([row.to(torch.int32),
                               c["vals"].view(torch.int32)], 1)
        ko.check_bits(name + ".train.rec", rec, rec_ref)


@pytest.mark.parametrize("K", fo.KS)
def test_backward_and_emit_exact(K):
    """fm_backward: exact slab totals, the bitmap is the batch's fid set, a
    second call doubles the totals. fm_backward_emit: gw bit for bit, gv by
    value (d < 0 times a zero bracket is -0); pos = a permutation's inverse
    gives the plain emit permuted, bit for bit."""
    for i, c in enumerate(fo.row_cases(K)):
        g = up_row(c)
        F, nnz = c["F"], c["fids"].numel()
        name = f"K{K}.case{i}"
        sv32 = fo.case_sumvx32(c)
        sumVX = sv32.to(DEV)
        gw64, gv64, _ = fo.fm_emit_ref(c["row_ptr"], c["fids"], c["vals"],
                                       c["V"], sv32, c["dpred"])
        totW, totV, _ = fo.fid_totals(c["fids"], gw64, gv64, F)
        words = fo.fid_words(c["fids"], F)

        gradW, gradV, touched = slabs(F, K)
        for rep in (1, 2):
            ops().fm_backward(g["row_ptr"], g["fids"], g["vals"], g["V"],
                              sumVX, g["dpred"], gradW, gradV, touched)
            # accumulators start at +0: a reference -0 is folded (exact32)
            ko.check_bits(f"{name}.gradW x{rep}", gradW,
                          fo.exact32(rep * totW))
            ko.check_bits(f"{name}.gradV x{rep}", gradV,
                          fo.exact32(rep * totV))
            assert torch.equal(touched.cpu(), words), name

        gw, gv = run_emit(g, sumVX, nnz, K)
        ko.check_bits(name + ".gw", gw, gw64.float())
        fo.check_value(name + ".gv", gv, gv64)
        gen = torch.Generator().manual_seed(K + i)
        perm = torch.randperm(nnz, generator=gen).to(torch.int32)
        pos = ops().inv_perm_i32(perm.to(DEV)) if nnz else \
            torch.zeros(0, dtype=torch.int32, device=DEV)
        gw2, gv2 = run_emit(g, sumVX, nnz, K, pos)
        ko.check_bits(name + ".gw[pos]", gw2[pos.long()], gw.cpu())
        ko.check_bits(name + ".gv[pos]", gv2[pos.long()], gv.cpu())


@pytest.mark.parametrize("K", fo.KS)
def test_row_kernels_empty_batch(K):
    """B = 0 returns empty tensors and launches nothing; the checked launch
    that follows reports nothing"""
    c = fo.row_case(K, [], 1)
    g = up_row(c)
    pred, sumVX = ops().fm_forward(g["row_ptr"], g["fids"], g["vals"],
                                   g["W"], g["V"])
    assert pred.shape == (0,) and sumVX.shape == (0, K)
    out = ops().fm_forward_train(g["row_ptr"], g["fids"], g["vals"], g["W"],
                                 g["V"], g["label"], 1.0, None)
    assert [tuple(t.shape) for t in out] == [(0,), (0,), (0, K), (0, 2)]
    loss, dpred = ops().logloss_grad(pred, g["label"], 1.0)
    assert loss.numel() == 0 and dpred.numel() == 0
    gw, gv = ops().fm_backward_emit(g["row_ptr"], g["fids"], g["vals"],
                                    g["V"], sumVX, g["dpred"], None)
    assert gw.shape == (0,) and gv.shape == (0, K)
    gradW, gradV, touched = slabs(c["F"], K)
    ops().fm_backward(g["row_ptr"], g["fids"], g["vals"], g["V"], sumVX,
                      g["dpred"], gradW, gradV, touched)
    assert not gradW.any() and not gradV.any() and not touched.any()
    c1 = fo.row_case(K, [3], 2)
    g1 = up_row(c1)
    run_forward(g1, 1, K)
    torch.cuda.synchronize()


@pytest.mark.parametrize("K", fo.KS)
def test_row_kernels_float(K):
    """Real rounding under the derived bounds: forward, emit, and the
    totals of the atomic backward and of the default sorted apply"""
    c = fo.float_row_case(K)
    g = up_row(c)
    B, F, nnz = c["B"], c["F"], c["fids"].numel()
    ref = fo.fm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"],
                            c["V"])
    pred, sumVX = run_forward(g, B, K)
    ko.check_bound(f"fm.float.K{K}.pred", pred, *ref["pred"])
    ko.check_bound(f"fm.float.K{K}.sumVX", sumVX, *ref["sumVX"])

    sv32 = ref["sumVX"][0].float()
    gw64, gv64, gvb = fo.fm_emit_ref(c["row_ptr"], c["fids"], c["vals"],
                                     c["V"], sv32, c["dpred"])
    gw, gv = run_emit(g, sv32.to(DEV), nnz, K)
    row, _, _ = ko.rows_pos(c["row_ptr"])
    ko.check_bits(f"fm.float.K{K}.gw", gw, c["dpred"][row] * c["vals"])
    ko.check_bound(f"fm.float.K{K}.gv", gv, gv64, gvb)

    totW, totV, (bW, bV) = fo.fid_totals(c["fids"], gw64, gv64, F, gvb)
    gradW, gradV, touched = slabs(F, K)
    ops().fm_backward(g["row_ptr"], g["fids"], g["vals"], g["V"],
                      sv32.to(DEV), g["dpred"], gradW, gradV, touched)
    ko.check_bound(f"fm.float.K{K}.gradW", gradW, totW, bW)
    ko.check_bound(f"fm.float.K{K}.gradV", gradV, totV, bV)

    # the sorted apply sums the emitted fp32 values: sum rule alone
    sf, perm = torch.sort(c["fids"], stable=True)
    tW, tV, (sW, sV) = fo.fid_totals(c["fids"], gw.cpu(), gv.cpu(), F,
                                     torch.zeros(nnz, K,
                                                 dtype=torch.float64))
    gradW, gradV, touched = slabs(F, K)
    ops().fm_sorted_apply(sf.to(DEV), perm.to(torch.int32).to(DEV), gw, gv,
                          gradW, gradV, touched, 0)
    # gw is exact here (already rounded): only the sum rule remains
    ko.check_bound(f"fm.float.K{K}.apply.gradW", gradW, tW, sW)
    ko.check_bound(f"fm.float.K{K}.apply.gradV", gradV, tV, sV)
    assert torch.equal(touched.cpu(), fo.fid_words(c["fids"], F))


def test_loss_sweep():
    """z = -17 .. 17 in steps of 1/4 and +-20, y in {0, 1}: logloss_grad
    and fm_forward_train agree bit for bit (the forward sees one-entry rows
    with W = z, x = 1, V = 0) and both stay inside the loss / dpred bounds"""
    s = fo.loss_sweep()
    B, K = s["z"].numel(), 4
    z, y = s["z"].to(DEV), s["y"].to(DEV)
    for _ in range(2):
        ko.poison((B,), torch.float32, DEV)
    loss, dpred = ops().logloss_grad(z, y, s["scale"])
    ref = fo.logloss_ref(s["z"], s["y"], s["scale"])
    ko.check_bound("fm.loss.loss", loss, *ref["loss"])
    ko.check_bound("fm.loss.dpred", dpred, *ref["dpred"])
    dev = (loss.cpu().double() - ref["loss"][0]).abs()
    print(f"FM_LOSS worst |loss - loss64| = {float(dev.max()):.6g} at z = "
          f"{float(s['z'][dev.argmax()])}")

    V = torch.zeros(B + 1, K)
    V[B] = NAN
    for _ in range(2):
        ko.poison((B,), torch.float32, DEV)
    ko.poison((B, K), torch.float32, DEV)
    poison_i32((B, 2))
    loss2, dpred2, sumVX, _ = ops().fm_forward_train(
        s["row_ptr"].to(DEV), view_on_gpu(s["fids"], B),
        view_on_gpu(s["vals"], NAN), s["W"].to(DEV), V.to(DEV), y,
        s["scale"], None)
    ko.check_bits("fm.loss.train.loss", loss2, loss.cpu())
    ko.check_bits("fm.loss.train.dpred", dpred2, dpred.cpu())
    ko.check_bits("fm.loss.train.sumVX", sumVX, torch.zeros(B, K))


# ---------------------------------------------------------------------------
# sorted apply, slab mode
# ---------------------------------------------------------------------------
def run_apply(c, chunk):
    K, F = c["K"], c["F"]
    gradW, gradV, touched = slabs(F, K)
    perm = None if c["perm"] is None else c["perm"].to(DEV)
    ops().fm_sorted_apply(view_on_gpu(c["sorted_fids"], F - 1), perm,
                          c["gw"].to(DEV), c["gv"].to(DEV), gradW, gradV,
                          touched, chunk)
    return gradW, gradV, touched


@pytest.mark.parametrize("K", fo.KS)
def test_sorted_apply_slab_exact(K):
    """Every chunk mode on hand-built integer gradients behind the route's
    run list (with and without perm) and the small nnz: totals bit for bit
    on zeroed slabs (an owned run is stored, an unowned one added: either
    way the slab holds the total and nothing else is written), bitmap = fid
    set. chunk = -1 at K = 32 / 64 takes the walk and is held to the same."""
    for chunk in fo.APPLY_CHUNKS:
        cases = [fo.apply_case(K, chunk, 100 * K + 1, with_perm=True),
                 fo.apply_case(K, chunk, 100 * K + 2, with_perm=False)]
        for j, nnz in enumerate(fo.apply_nnz_cases(K, chunk)):
            cases.append(fo.apply_case(K, chunk, 100 * K + 10 + j, nnz=nnz,
                                       with_perm=bool(j % 2)))
        for i, c in enumerate(cases):
            name = f"apply.K{K}.chunk{chunk}.case{i}"
            fo.assert_exact_totals(c["sorted_fids"], c["gw_sorted"],
                                   c["gv_sorted"], c["F"], 1.0)
            totW, totV = fo.apply_totals(c)
            gradW, gradV, touched = run_apply(c, chunk)
            ko.check_bits(name + ".gradW", gradW, fo.exact32(totW))
            ko.check_bits(name + ".gradV", gradV, fo.exact32(totV))
            assert torch.equal(touched.cpu(),
                               fo.fid_words(c["sorted_fids"], c["F"])), name


# ---------------------------------------------------------------------------
# fused walk and the sparse optimizers behind it
# ---------------------------------------------------------------------------
def up_state(st):
    return {k: v.to(DEV) for k, v in st.items()}


def sparse_apply(opt_mode, uniq, count, g, gradW, gradV):
    if opt_mode == 1:
        ops().fm_adagrad_apply(uniq, count, g["W"], g["V"], g["nW"],
                               g["nV"], gradW, gradV, fo.ADAGRAD["lr"],
                               fo.ADAGRAD["eps"], fo.ADAGRAD["l2"])
    else:
        ops().fm_ftrl_apply(uniq, count, g["W"], g["V"], g["zW"], g["nW"],
                            g.get("zV"), g["nV"], gradW, gradV,
                            fo.FTRL["alpha"], fo.FTRL["beta"], fo.FTRL["l1"],
                            fo.FTRL["l2"], 1 if opt_mode == 3 else 0,
                            fo.V_ADAGRAD["lr"], fo.V_ADAGRAD["eps"],
                            fo.V_ADAGRAD["l2"])


def check_state(name, g, st, ref, stepped, kept):
    """rows `stepped`: one optimizer step within the oracle's bounds; rows
    `kept`: bit-identical to the uploaded state"""
    for k in st:
        if k not in ref:   # zV under Adagrad on V: nothing may write it
            ko.check_bits(f"{name}.{k}.unused", g[k], st[k])
            continue
        check_rows(f"{name}.{k}", g[k], ref[k], stepped)
        check_rows_bits(f"{name}.{k}.kept", g[k], st[k], kept)


def check_ftrl_edges(name, g, c, opt_mode):
    """from zero state z' = g exactly; the four gradients inside or on the
    dead zone give w = +0, bit for bit"""
    e = c["edge_fids"]
    edge = fo.ftrl_edge_gradients()
    ko.check_bits(name + ".edge.zW", g["zW"].cpu()[e], edge)
    ko.check_bits(name + ".edge.W", g["W"].cpu()[e[:4]], torch.zeros(4))
    assert (g["W"].cpu()[e[4:]] != 0).all(), name
    if opt_mode == 2:
        K = c["K"]
        ko.check_bits(name + ".edge.zV", g["zV"].cpu()[e],
                      edge.unsqueeze(1).expand(6, K).contiguous())
        ko.check_bits(name + ".edge.V", g["V"].cpu()[e[:4]],
                      torch.zeros(4, K))


@pytest.mark.parametrize("opt_mode", (1, 2, 3))
@pytest.mark.parametrize("K", fo.KS)
def test_fused_walk(K, opt_mode):
    """fm_sorted_apply_fused without assuming its chunk: every fid of the
    batch is either reported (bit set, state untouched, slab rows = exact
    total) or updated in place (bit clear, slab rows +0, one optimizer step
    on the exact total); both occur. bitmap_compact + the sparse apply then
    bring every fid to the oracle step and leave the slabs +0."""
    c = fo.fused_case(K, 300 * K + opt_mode, opt_mode)
    F, st = c["F"], c["state"]
    name = f"fused.K{K}.mode{opt_mode}"
    totW, totV = fo.apply_totals(c)
    ref = fo.opt_step_ref(st, totW, totV, opt_mode)
    g = up_state(st)
    gradW, gradV, touched = slabs(F, K)
    ops().fm_sorted_apply_fused(
        view_on_gpu(c["sorted_fids"], F - 1), c["perm"].to(DEV),
        c["gw"].to(DEV), c["gv"].to(DEV), gradW, gradV, touched, g["W"],
        g["V"], g["nW"], g["nV"], g.get("zW"), g.get("zV"), opt_mode,
        *fo.opt_args(opt_mode))
    batch = torch.unique(c["sorted_fids"].long())
    reported = fo.words_to_fids(touched)
    assert np.isin(reported.numpy(), batch.numpy()).all(), name
    inplace = batch[~np.isin(batch.numpy(), reported.numpy())]
    assert reported.numel() > 0 and inplace.numel() > 0, name
    check_state(name, g, st, ref, inplace,
                torch.cat([reported, others(F, batch)]))
    zW, zV = torch.zeros(F), torch.zeros(F, K)
    keep0 = others(F, reported)
    check_rows_bits(name + ".gradW", gradW, fo.exact32(totW), reported)
    check_rows_bits(name + ".gradV", gradV, fo.exact32(totV), reported)
    check_rows_bits(name + ".gradW.zero", gradW, zW, keep0)
    check_rows_bits(name + ".gradV.zero", gradV, zV, keep0)
    if opt_mode != 1:
        check_ftrl_edges(name, g, c, opt_mode)

    uniq = torch.full((F,), F - 1, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops().bitmap_compact(touched, uniq, count)
    assert int(count) == reported.numel() and not touched.any()
    sparse_apply(opt_mode, uniq, count, g, gradW, gradV)
    check_state(name + ".after", g, st, ref, batch, others(F, batch))
    ko.check_bits(name + ".after.gradW", gradW, zW)
    ko.check_bits(name + ".after.gradV", gradV, zV)


@pytest.mark.parametrize("opt_mode", (1, 2, 3))
@pytest.mark.parametrize("K", fo.KS)
def test_sparse_apply(K, opt_mode):
    """fm_adagrad_apply / fm_ftrl_apply (both v_adagrad values) over lists
    around the 256 / K rows of a block: listed rows take one step and their
    slab rows become +0; rows behind `count`, rows behind the list view
    (count above its length is clamped) and every other row and slab entry
    stay bit-identical."""
    rpb = 256 // K
    for n in (1, 3, rpb - 1, rpb, rpb + 1, 257):
        for over in (0, -1, 7):
            if n + over < 1:
                continue
            c = fo.sparse_case(K, n, 1000 * K + 10 * n + over, opt_mode != 1)
            F, st = c["F"], c["state"]
            if opt_mode == 1:
                st = {k: v for k, v in st.items() if k[0] != "z"}
            name = f"sparse.K{K}.mode{opt_mode}.n{n}.over{over}"
            g = up_state(st)
            gradW, gradV = c["gradW"].to(DEV), c["gradV"].to(DEV)
            buf = torch.cat([c["list"], c["tail"]]).to(DEV)
            uniq = buf[:n]
            count = torch.tensor([n + over], dtype=torch.int32, device=DEV)
            sparse_apply(opt_mode, uniq, count, g, gradW, gradV)
            live = c["list"].long()[:min(n, n + over)]
            ref = fo.opt_step_ref(st, c["gradW"], c["gradV"], opt_mode)
            rest = others(F, live)
            check_state(name, g, st, ref, live, rest)
            check_rows_bits(name + ".gradW", gradW, torch.zeros(F), live)
            check_rows_bits(name + ".gradV", gradV, torch.zeros(F, K), live)
            check_rows_bits(name + ".gradW.rest", gradW, c["gradW"], rest)
            check_rows_bits(name + ".gradV.rest", gradV, c["gradV"], rest)
            if opt_mode != 1 and n >= 6 and over >= 0:
                e = c["list"].long()[:6]
                edge = fo.ftrl_edge_gradients()
                ko.check_bits(name + ".edge.zW", g["zW"].cpu()[e], edge)
                ko.check_bits(name + ".edge.W", g["W"].cpu()[e[:4]],
                              torch.zeros(4))


# ---------------------------------------------------------------------------
# list-fed and tile-local segment reduces
# ---------------------------------------------------------------------------
SENT = -7


def spill_buffers(n, start=0):
    """(buffer, view of n slots, counter): the view lies inside a longer
    buffer of sentinels"""
    buf = torch.full((n + 2 * fo.PAD,), SENT, dtype=torch.int32, device=DEV)
    cnt = torch.full((1,), start, dtype=torch.int32, device=DEV)
    return buf, buf[fo.PAD:fo.PAD + n], cnt


def check_spill(name, buf, n, cnt, pred, start=0, short=False):
    """the list holds the predicted spill set once each, from slot `start`;
    nothing outside [start, start + count) of the view is written"""
    total = int(cnt) - start
    assert total == pred.numel(), (name, total, pred.numel())
    b = buf.cpu()
    view = b[fo.PAD:fo.PAD + n]
    wrote = min(total, n - start)
    got = view[start:start + wrote].long()
    assert got.unique().numel() == wrote, name + ": fid listed twice"
    if short:
        assert np.isin(got.numpy(), pred.numpy()).all(), name
    else:
        assert torch.equal(got.sort().values, pred), name
    assert (view[:start] == SENT).all() and \
        (view[start + wrote:] == SENT).all(), name
    assert (b[:fo.PAD] == SENT).all() and (b[fo.PAD + n:] == SENT).all(), \
        name + ": wrote outside the spill list"


def check_segment(name, c, g, st, gradW, gradV, totW, totV, pred, opt_mode):
    """spilled fids: state untouched, slab rows = exact total; every other
    fid of the batch: one optimizer step, slab rows +0; the rest of the
    table untouched"""
    F, K = c["F"], c["K"]
    ref = fo.opt_step_ref(st, totW, totV, opt_mode)
    batch = torch.unique(c["sorted_fids"].long())
    inplace = batch[~np.isin(batch.numpy(), pred.numpy())]
    check_state(name, g, st, ref, inplace,
                torch.cat([pred, others(F, batch)]))
    check_rows_bits(name + ".gradW", gradW, fo.exact32(totW), pred)
    check_rows_bits(name + ".gradV", gradV, fo.exact32(totV), pred)
    keep0 = others(F, pred)
    check_rows_bits(name + ".gradW.zero", gradW, torch.zeros(F), keep0)
    check_rows_bits(name + ".gradV.zero", gradV, torch.zeros(F, K), keep0)
    return inplace


def emit_case(K, runs, seed, with_perm):
    """apply_case-shaped hand-built integer gradients behind a run list"""
    c = fo.apply_case(K, 0, seed, nnz=1, with_perm=with_perm)
    sf, F = fo.runs_stream(runs, seed)
    n = sf.numel()
    gen = torch.Generator().manual_seed(seed + 5)
    gw_s = torch.randint(-3, 4, (n,), generator=gen).float()
    gv_s = torch.randint(-3, 4, (n, K), generator=gen).float()
    c.update(sorted_fids=sf, F=F, gw_sorted=gw_s, gv_sorted=gv_s, gw=gw_s,
             gv=gv_s, perm=None)
    if with_perm:
        perm = torch.randperm(n, generator=gen).to(torch.int32)
        gw, gv = torch.empty(n), torch.empty(n, K)
        gw[perm.long()] = gw_s
        gv[perm.long()] = gv_s
        c.update(perm=perm, gw=gw, gv=gv)
    return c


def run_segment_emit(c, st, cap, opt_mode, spill_len):
    K, F = c["K"], c["F"]
    g = up_state(st)
    gradW, gradV, _ = slabs(F, K)
    sf = view_on_gpu(c["sorted_fids"], F - 1)
    buf, spill, cnt = spill_buffers(spill_len)
    piece_start, n_pieces = ops().segment_worklist(sf, cap, None)
    perm = None if c["perm"] is None else c["perm"].to(DEV)
    ops().fm_segment_apply(sf, perm, piece_start, n_pieces, c["gw"].to(DEV),
                           c["gv"].to(DEV), gradW, gradV, spill, cnt, g["W"],
                           g["V"], g["nW"], g["nV"], g.get("zW"),
                           g.get("zV"), opt_mode, *fo.opt_args(opt_mode))
    return g, gradW, gradV, buf, cnt


def run_segment_rec(c, st, cap, opt_mode, spill_len, tile=False, start=0):
    K, F = c["K"], c["F"]
    g = up_state(st)
    gradW, gradV, _ = slabs(F, K)
    sf = view_on_gpu(c["sorted_fids"], F - 1)
    buf, spill, cnt = spill_buffers(spill_len, start)
    rec, sumVX, dpred = (c[k].to(DEV) for k in ("rec", "sumVX", "dpred"))
    tail = (gradW, gradV, spill, cnt, g["W"], g["V"], g["nW"], g["nV"],
            g.get("zW"), g.get("zV"), opt_mode) + fo.opt_args(opt_mode)
    if tile:
        ops().fm_segment_tile_rec(sf, rec, sumVX, dpred, cap, *tail)
    else:
        piece_start, n_pieces = ops().segment_worklist(sf, cap, None)
        ops().fm_segment_apply_rec(sf, rec, sumVX, dpred, piece_start,
                                   n_pieces, *tail)
    return g, gradW, gradV, buf, cnt


def rec_totals(c, st):
    gw, gv = fo.record_gradients(c, st["V"])
    fo.assert_exact_totals(c["sorted_fids"], gw, gv, c["F"], 2.0 ** -c["s"])
    totW, totV, _ = fo.fid_totals(c["sorted_fids"], gw, gv, c["F"])
    return totW, totV


@pytest.mark.parametrize("K", fo.KS)
def test_segment_list_fed(K):
    """fm_segment_apply (with and without perm) and fm_segment_apply_rec at
    cap 1, 2, 32, 256: the spill list is exactly the runs with a multiple
    of cap strictly inside; those keep their state and get exact slab
    totals, every other run is one optimizer step in place. A spill list
    shorter than the spilled set is not overrun and the count stays true."""
    for ci, cap in enumerate((1, 2, 32, 256)):
        opt_mode = 1 + (ci + K // 8) % 3
        ftrl = opt_mode != 1
        runs = fo.segment_runs(cap)
        for v, with_perm in enumerate((True, False)):
            c = emit_case(K, runs, 500 * K + 10 * cap + v, with_perm)
            name = f"segment.K{K}.cap{cap}.perm{int(with_perm)}"
            fo.assert_exact_totals(c["sorted_fids"], c["gw_sorted"],
                                   c["gv_sorted"], c["F"], 1.0)
            st = fo.int_state(c["F"], K, 7 * K + cap, ftrl)
            pred = fo.spill_set(c["sorted_fids"], cap)
            totW, totV = fo.apply_totals(c)
            g, gradW, gradV, buf, cnt = run_segment_emit(
                c, st, cap, opt_mode, pred.numel() + 3)
            check_spill(name, buf, pred.numel() + 3, cnt, pred)
            inplace = check_segment(name, c, g, st, gradW, gradV, totW,
                                    totV, pred, opt_mode)
            assert pred.numel() > 0 and inplace.numel() > 0, name

        c = fo.record_case(K, runs, 600 * K + cap, s=2 + ci)
        name = f"segment_rec.K{K}.cap{cap}"
        st = fo.int_state(c["F"], K, 9 * K + cap, ftrl)
        pred = fo.spill_set(c["sorted_fids"], cap)
        totW, totV = rec_totals(c, st)
        g, gradW, gradV, buf, cnt = run_segment_rec(
            c, st, cap, opt_mode, pred.numel() + 3)
        check_spill(name, buf, pred.numel() + 3, cnt, pred)
        check_segment(name, c, g, st, gradW, gradV, totW, totV, pred,
                      opt_mode)

        # a list two short of the spilled set
        short = pred.numel() - 2
        assert short >= 1
        g, gradW, gradV, buf, cnt = run_segment_rec(c, st, cap, opt_mode,
                                                    short)
        check_spill(name + ".short", buf, short, cnt, pred, short=True)
        check_segment(name + ".short", c, g, st, gradW, gradV, totW, totV,
                      pred, opt_mode)


def test_segment_stride_loop_k64():
    """2 * 8 * CUs * 4 + 5 runs of one entry at K = 64: more pieces than
    twice any grid the launcher can pick (8 blocks of 4 waves per CU fill
    its 32 wave slots), so every wave makes a second and some a third trip
    of the stride loop with its two-ahead prefetch"""
    K, cap, opt_mode = 64, 256, 3
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    runs = [1] * (2 * 8 * cus * 4 + 5)
    pred = torch.zeros(0, dtype=torch.int64)
    c = emit_case(K, runs, 64064, True)
    st = fo.int_state(c["F"], K, 64065, True)
    totW, totV = fo.apply_totals(c)
    g, gradW, gradV, buf, cnt = run_segment_emit(c, st, cap, opt_mode, 4)
    check_spill("stride.emit", buf, 4, cnt, pred)
    check_segment("stride.emit", c, g, st, gradW, gradV, totW, totV, pred,
                  opt_mode)
    c = fo.record_case(K, runs, 64066)
    st = fo.int_state(c["F"], K, 64067, True)
    totW, totV = rec_totals(c, st)
    g, gradW, gradV, buf, cnt = run_segment_rec(c, st, cap, opt_mode, 4)
    check_spill("stride.rec", buf, 4, cnt, pred)
    check_segment("stride.rec", c, g, st, gradW, gradV, totW, totV, pred,
                  opt_mode)


@pytest.mark.parametrize("K", fo.KS)
def test_segment_tile(K):
    """fm_segment_tile_rec with the tile and split read from the extension,
    cap in {1, 32, 64, T}: the spill prediction and per-fid conditions of
    the list-fed reduce; the counter starts from the value passed; the
    list-fed recompute reduce reaches bit-identical state on every fid that
    does not spill."""
    T, S = ops().fm_segment_tile(), ops().fm_segment_split()
    START = 5
    for ci, cap in enumerate((1, 32, 64, T)):
        opt_mode = 1 + (ci + K // 4) % 3
        ftrl = opt_mode != 1
        lists = [fo.tile_runs(cap, T, S)]
        for nnz in (1, T - 1, T, T + 1, 2 * T + 3):
            runs, left = [], nnz
            while left > 0:
                runs.append(min(left, 1 + (len(runs) * 7) % 5))
                left -= runs[-1]
            lists.append(runs)
        for li, runs in enumerate(lists):
            c = fo.record_case(K, runs, 700 * K + 10 * cap + li, s=1 + ci)
            name = f"tile.K{K}.cap{cap}.list{li}"
            st = fo.int_state(c["F"], K, 11 * K + cap + li, ftrl)
            pred = fo.spill_set(c["sorted_fids"], cap)
            totW, totV = rec_totals(c, st)
            n = START + pred.numel() + 3
            g, gradW, gradV, buf, cnt = run_segment_rec(
                c, st, cap, opt_mode, n, tile=True, start=START)
            check_spill(name, buf, n, cnt, pred, start=START)
            inplace = check_segment(name, c, g, st, gradW, gradV, totW,
                                    totV, pred, opt_mode)
            if li == 0:
                assert pred.numel() > 0 and inplace.numel() > 0, name
            g2, _, _, _, _ = run_segment_rec(c, st, cap, opt_mode, n)
            for k in st:
                check_rows_bits(f"{name}.{k}.list_fed", g[k], g2[k].cpu(),
                                inplace)


# ---------------------------------------------------------------------------
# sort
# ---------------------------------------------------------------------------
def test_sort_ids_is_the_stable_sort():
    """the permutation is torch.sort(stable=True)'s, not just a valid one"""
    from lightctr_amd.ops._extension import sort_ids

    gen = torch.Generator().manual_seed(5)
    for n in (1, 2, 255, 256, 257, 4097):
        for upper in (2, 7, 1000, 1 << 24):
            fids = torch.randint(0, upper, (n,), generator=gen,
                                 dtype=torch.int32)
            s, p = sort_ids(fids.to(DEV), upper)
            rs, rp = torch.sort(fids, stable=True)
            assert torch.equal(s.cpu(), rs), (n, upper)
            assert torch.equal(p.cpu().long(), rp), (n, upper)


# ---------------------------------------------------------------------------
# binding checks: every bad argument raises before anything is launched
# ---------------------------------------------------------------------------
def _bad_variants(t):
    """(label, tensor) mutations a binding must reject"""
    out = [("cpu", t.cpu())]
    if t.is_floating_point():
        out.append(("dtype", t.double()))
    elif t.dtype == torch.int32:
        out.append(("dtype", t.long()))
    else:
        out.append(("dtype", t.to(torch.int32)))
    if t.numel() >= 1:
        out.append(("short", t.flatten()[:-1]))
    big = torch.cat([t.flatten(), t.flatten()])[::2]
    if not big.is_contiguous():    # one element is contiguous at any stride
        out.append(("strided", big))
    return out


def _raises_for_each(fn, args, names, valid=()):
    """fn(**args) passes; with any named argument mutated it raises.
    `valid` names the (argument, mutation) pairs that are still a valid
    call, such as a shorter fid list: those are not made."""
    fn(**{k: (v.clone() if torch.is_tensor(v) else v)
          for k, v in args.items()})
    torch.cuda.synchronize()
    for nm in names:
        for label, bad in _bad_variants(args[nm]):
            if (nm, label) in valid:
                continue
            a = dict(args)
            a[nm] = bad
            try:
                fn(**a)
            except RuntimeError:
                continue
            pytest.fail(f"{nm} ({label}) was accepted")


def _small(K=8, B=3):
    c = fo.row_case(K, [2, 0, 3][:B], 42)
    g = torch.Generator().manual_seed(1)
    F = c["F"]
    d = {k: c[k].to(DEV) for k in ("row_ptr", "fids", "vals", "dpred",
                                    "label")}
    d["W"] = torch.randn(F, generator=g).to(DEV)
    d["V"] = torch.randn(F, K, generator=g).to(DEV)
    d["sumVX"] = torch.zeros(B, K, device=DEV)
    return c, d


def _apply_args(K=8):
    c = fo.apply_case(K, 0, 77, nnz=9, with_perm=True)
    F = c["F"]
    gradW, gradV, touched = slabs(F, K)
    a = dict(sorted_fids=c["sorted_fids"].to(DEV), perm=c["perm"].to(DEV),
             gw=c["gw"].to(DEV), gv=c["gv"].to(DEV), gradW=gradW,
             gradV=gradV, touched=touched)
    return c, a


def test_checks_k_outside_dispatch_set():
    """K = 5 (and a V that is not 2-D) is an exception in every FM binding,
    not an abort of the process"""
    o = ops()
    for K in (5, None):
        c, d = _small()
        F, B, nnz = c["F"], c["B"], c["fids"].numel()
        V = torch.zeros(F, 5, device=DEV) if K == 5 else \
            torch.zeros(F, 2, 4, device=DEV)
        Kb = 5 if K == 5 else 8
        slabW = torch.zeros(F, device=DEV)
        slabV = torch.zeros_like(V)
        touched = torch.zeros((F + 63) // 64, dtype=torch.int64, device=DEV)
        sv = torch.zeros(B, Kb, device=DEV)
        csr = (d["row_ptr"], d["fids"], d["vals"])
        i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)  # noqa
        calls = [
            lambda: o.fm_forward(*csr, d["W"], V),
            lambda: o.fm_forward_train(*csr, d["W"], V, d["label"], 1.0,
                                       None),
            lambda: o.fm_backward(*csr, V, sv, d["dpred"], slabW, slabV,
                                  touched),
            lambda: o.fm_backward_emit(*csr, V, sv, d["dpred"], None),
            lambda: o.fm_sorted_apply(d["fids"], None,
                                      torch.zeros(nnz, device=DEV),
                                      torch.zeros(nnz, Kb, device=DEV),
                                      slabW, slabV, touched, 0),
            lambda: o.fm_sorted_apply_fused(
                d["fids"], None, torch.zeros(nnz, device=DEV),
                torch.zeros(nnz, Kb, device=DEV), slabW, slabV, touched,
                d["W"], V, slabW.clone(), slabV.clone(), None, None, 1,
                0.1, 1e-8, 0.0, 0.0),
            lambda: o.fm_adagrad_apply(i32(2), i32(1), d["W"], V,
                                       slabW.clone(), slabV.clone(), slabW,
                                       slabV, 0.1, 1e-8, 0.0),
            lambda: o.fm_ftrl_apply(i32(2), i32(1), d["W"], V, slabW.clone(),
                                    slabW.clone(), slabV.clone(),
                                    slabV.clone(), slabW, slabV, 0.1, 1.0,
                                    0.01, 0.0),
            lambda: o.fm_segment_apply(
                d["fids"], None, i32(nnz), i32(1),
                torch.zeros(nnz, device=DEV),
                torch.zeros(nnz, Kb, device=DEV), slabW, slabV, i32(4),
                i32(1), d["W"], V, slabW.clone(), slabV.clone(), None, None,
                1, 0.1, 1e-8, 0.0, 0.0),
            lambda: o.fm_segment_apply_rec(
                d["fids"], torch.zeros(nnz, 2, dtype=torch.int32,
                                       device=DEV), sv, d["dpred"], i32(nnz),
                i32(1), slabW, slabV, i32(4), i32(1), d["W"], V,
                slabW.clone(), slabV.clone(), None, None, 1, 0.1, 1e-8, 0.0,
                0.0),
            lambda: o.fm_segment_tile_rec(
                d["fids"], torch.zeros(nnz, 2, dtype=torch.int32,
                                       device=DEV), sv, d["dpred"], 32,
                slabW, slabV, i32(4), i32(1), d["W"], V, slabW.clone(),
                slabV.clone(), None, None, 1, 0.1, 1e-8, 0.0, 0.0),
        ]
        for call in calls:
            with pytest.raises(RuntimeError):
                call()
    torch.cuda.synchronize()


def test_checks_row_kernels():
    o = ops()
    c, d = _small()

    def emit(row_ptr, fids, vals, V, sumVX, dpred, pos):
        return o.fm_backward_emit(row_ptr, fids, vals, V, sumVX, dpred, pos)

    nnz = c["fids"].numel()
    args = dict(row_ptr=d["row_ptr"], fids=d["fids"], vals=d["vals"],
                V=d["V"], sumVX=d["sumVX"], dpred=d["dpred"],
                pos=torch.arange(nnz, dtype=torch.int32, device=DEV))
    _raises_for_each(emit, args, ("row_ptr", "fids", "vals", "V", "sumVX",
                                  "dpred", "pos"))
    csr = (d["row_ptr"], d["fids"], d["vals"])
    empty_rp = torch.zeros(0, dtype=torch.int32, device=DEV)
    bad = [
        lambda: o.fm_forward(d["row_ptr"], d["fids"], d["vals"][:-1],
                             d["W"], d["V"]),
        lambda: o.fm_forward(d["row_ptr"], d["fids"][:-1], d["vals"],
                             d["W"], d["V"]),
        lambda: o.fm_forward(*csr, d["W"][:-1], d["V"]),
        lambda: o.fm_forward(empty_rp, d["fids"], d["vals"], d["W"],
                             d["V"]),
        lambda: o.fm_forward_train(*csr, d["W"], d["V"], d["label"][:-1],
                                   1.0, None),
        lambda: o.logloss_grad(d["dpred"], d["label"][:-1], 1.0),
        lambda: o.fm_backward_emit(empty_rp, d["fids"], d["vals"], d["V"],
                                   d["sumVX"], d["dpred"], None),
    ]
    F, K = c["F"], c["K"]
    gradW, gradV, touched = slabs(F, K)
    bad += [
        lambda: o.fm_backward(*csr, d["V"], d["sumVX"], d["dpred"], gradW,
                              gradV, touched[:-1]),
        lambda: o.fm_backward(*csr, d["V"], d["sumVX"], d["dpred"], gradW,
                              gradV, touched.to(torch.int32)),
        lambda: o.fm_backward(*csr, d["V"], d["sumVX"], d["dpred"],
                              gradW[:-1], gradV, touched),
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()


def test_checks_sorted_apply():
    o = ops()
    c, a = _apply_args()
    names = ("sorted_fids", "gw", "gv", "gradW", "gradV", "touched")

    def slab(**kw):
        return o.fm_sorted_apply(chunk=0, **kw)

    _raises_for_each(slab, a, names)
    for bad_perm in (a["perm"].cpu(), a["perm"][:-1], a["perm"].float()):
        with pytest.raises(RuntimeError):
            slab(**dict(a, perm=bad_perm))
    for chunk in (-5, -100):
        with pytest.raises(RuntimeError):
            o.fm_sorted_apply(chunk=chunk, **a)

    F, K = c["F"], c["K"]
    st = up_state(fo.int_state(F, K, 3, True))

    def fused(**kw):
        return o.fm_sorted_apply_fused(opt_mode=2, p0=0.15, p1=1.0, p2=0.01,
                                       p3=1e-4, **kw)

    fa = dict(a, **st)
    _raises_for_each(fused, fa, names + ("W", "V", "nW", "nV", "zW", "zV"))
    with pytest.raises(RuntimeError):    # FTRL on V needs zV
        fused(**dict(fa, zV=None))
    with pytest.raises(RuntimeError):
        fused(**dict(fa, zW=None))
    with pytest.raises(RuntimeError):
        o.fm_sorted_apply_fused(opt_mode=4, p0=0.1, p1=1.0, p2=0.0, p3=0.0,
                                **fa)
    torch.cuda.synchronize()


def test_checks_sparse_apply():
    o = ops()
    F, K = 70, 8
    st = up_state(fo.int_state(F, K, 4, True))
    gradW, gradV, _ = slabs(F, K)
    base = dict(uniq=torch.tensor([0, 5, 69], dtype=torch.int32,
                                  device=DEV),
                count=torch.tensor([3], dtype=torch.int32, device=DEV),
                gradW=gradW, gradV=gradV)

    def ada(uniq, count, W, V, nW, nV, gradW, gradV):
        return o.fm_adagrad_apply(uniq, count, W, V, nW, nV, gradW, gradV,
                                  0.01, 1e-8, 0.0)

    aa = dict(base, **{k: st[k] for k in ("W", "V", "nW", "nV")})
    _raises_for_each(ada, aa, ("uniq", "W", "V", "nW", "nV", "gradW",
                               "gradV"), valid=(("uniq", "short"),))
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    for bad in (empty, base["count"].cpu(), base["count"].long()):
        with pytest.raises(RuntimeError):
            ada(**dict(aa, count=bad))

    def ftrl(uniq, count, W, V, zW, nW, zV, nV, gradW, gradV, v_adagrad=0):
        return o.fm_ftrl_apply(uniq, count, W, V, zW, nW, zV, nV, gradW,
                               gradV, 0.15, 1.0, 0.01, 1e-4, v_adagrad)

    fa = dict(base, **st)
    _raises_for_each(ftrl, fa, ("uniq", "W", "V", "zW", "nW", "zV", "nV",
                                "gradW", "gradV"),
                     valid=(("uniq", "short"),))
    for bad in (empty, base["count"].cpu(), base["count"].long()):
        with pytest.raises(RuntimeError):
            ftrl(**dict(fa, count=bad))
    with pytest.raises(RuntimeError):     # FTRL on V needs zV
        ftrl(**dict(fa, zV=None))
    ftrl(**dict(fa, zV=None, v_adagrad=1))   # Adagrad on V does not
    torch.cuda.synchronize()


def test_empty_inputs_launch_nothing():
    """an empty fid list, an empty sorted stream: no launch (a grid of 0
    blocks is a launch error), state untouched, and the checked launch that
    follows reports nothing"""
    o = ops()
    F, K = 70, 8
    st0 = fo.int_state(F, K, 6, True)
    st = up_state(st0)
    gradW, gradV, touched = slabs(F, K)
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    o.fm_adagrad_apply(empty, count, st["W"], st["V"], st["nW"], st["nV"],
                       gradW, gradV, 0.01, 1e-8, 0.0)
    o.fm_ftrl_apply(empty, count, st["W"], st["V"], st["zW"], st["nW"],
                    st["zV"], st["nV"], gradW, gradV, 0.15, 1.0, 0.01, 1e-4)
    ef = torch.zeros(0, device=DEV)
    o.fm_sorted_apply(empty, None, ef, torch.zeros(0, K, device=DEV), gradW,
                      gradV, touched, 0)
    o.fm_sorted_apply(empty, empty, ef, torch.zeros(0, K, device=DEV),
                      gradW, gradV, touched, -1)
    o.fm_sorted_apply_fused(empty, None, ef, torch.zeros(0, K, device=DEV),
                            gradW, gradV, touched, st["W"], st["V"],
                            st["nW"], st["nV"], st["zW"], st["zV"], 2, 0.15,
                            1.0, 0.01, 1e-4)
    for k in st0:
        ko.check_bits("empty." + k, st[k], st0[k])
    assert not touched.any() and not gradW.any() and not gradV.any()
    # a checked launch after them
    one = torch.tensor([3], dtype=torch.int32, device=DEV)
    count.fill_(1)
    o.fm_adagrad_apply(one, count, st["W"], st["V"], st["nW"], st["nV"],
                       gradW, gradV, 0.01, 1e-8, 0.0)
    torch.cuda.synchronize()
