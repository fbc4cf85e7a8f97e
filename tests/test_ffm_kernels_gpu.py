"""Parity tests for the field-aware kernels (ffm_kernels.hip) against the
float64 oracles of ``ffm_oracles.py``.

Main set: inputs on which fp32, bf16 and fp16 arithmetic is exact (the
rule and its magnitude conditions are stated in ``ffm_oracles.py`` and
asserted for every case), so every comparison is bit or value equality and
no summation or atomic order can excuse a difference. A small float set
keeps real rounding in view under derived bounds; the fused optimizer is
held to ``adagrad_ref`` / ``ftrl_ref`` applied once to the exact total
gradient. ``test_ffm_oracles.py`` shows on the CPU that the wrong
references listed in docs/TESTING.md differ on these same inputs.
"""

import pytest
import torch

import ffm_oracles as fo
import kernel_oracles as ko
from lightctr_amd.models.ffm import FFMHyper, FFMModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
CSR = ("row_ptr", "fields", "fids", "vals")
ADA = dict(lr=0.05, eps=1e-8, l2=1e-5)


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def csr(c):
    return tuple(c[k] for k in CSR)


def gcsr(c):
    return tuple(c[k].to(DEV) for k in CSR)


def slabs(F, D):
    return (torch.zeros(F, device=DEV), torch.zeros(F, D, device=DEV),
            torch.zeros((F + 63) // 64, dtype=torch.int64, device=DEV))


def check_slabs(name, gradW, gradV, touched, ref, fids, F):
    """totals bit for bit (rows of fids outside the batch are +0 in the
    oracle too) and exactly the batch's bits in the bitmap"""
    refW, refV, magW, magV = ref
    fo.assert_exact_fp32(name + ".gradW", magW)
    fo.assert_exact_fp32(name + ".gradV", magV)
    ko.check_bits(name + ".gradW", gradW, refW.float())
    ko.check_bits(name + ".gradV", gradV.view(F, -1), refV.float())
    assert torch.equal(touched.cpu(), fo.touched_words(fids, F)), name


def poison_i32(n):
    """ko.poison for an int32 output: -1 where a kernel writes nothing"""
    p = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    del p


def shape_kind_params(row_emit):
    return [pytest.param(K, shape, kind, id=f"K{K}-{shape}-{kind}")
            for K in fo.KS for shape in fo.shape_names(K, row_emit)
            for kind in fo.ROW_KINDS]


# ---------------------------------------------------------------------------
# forward and the three fp32 backward variants, exact set
# ---------------------------------------------------------------------------
def run_backward_variants(name, c, ref):
    o = ops()
    F, nf, K = c["V"].shape
    g = gcsr(c)
    V, d = c["V"].to(DEV), c["dpred"].to(DEV)
    sf, pm = (t.to(DEV) for t in fo.sort_entries(c["fids"]))
    nnz = c["fids"].numel()

    gradW, gradV, touched = slabs(F, nf * K)
    o.ffm_backward(*g, V, d, gradW, gradV.view(F, nf, K), touched)
    check_slabs(name + ".atomic", gradW, gradV, touched, ref, c["fids"], F)

    poison_i32(nnz)
    roe = o.row_index(g[0], nnz)
    gradW, gradV, touched = slabs(F, nf * K)
    o.ffm_sorted_backward(sf, pm, roe, *g, V, d, gradW,
                          gradV.view(F, nf, K), touched)
    check_slabs(name + ".sorted", gradW, gradV, touched, ref, c["fids"], F)

    ko.poison((nnz,), torch.float32, DEV)
    ko.poison((nnz, nf * K), torch.float32, DEV)
    gw, gblocks = o.ffm_block_emit(roe, *g, V, d)
    gradW, gradV, touched = slabs(F, nf * K)
    o.ffm_blocks_apply(sf, pm, gblocks, gw, gradW, gradV, touched)
    check_slabs(name + ".blocks", gradW, gradV, touched, ref, c["fids"], F)


@pytest.mark.parametrize("K,shape,kind", shape_kind_params(False))
def test_forward_and_fp32_backwards_exact(K, shape, kind):
    """ffm_forward / ffm_forward_pp (two bindings of one kernel,
    ffm_forward_pp_kernel; each has its own argument checks) on fp32 and
    bf16 V, then ffm_backward, ffm_sorted_backward and ffm_block_emit +
    ffm_blocks_apply: bit-exact predictions, totals and bitmap."""
    o = ops()
    for c in fo.exact_cases(K, shape, kind):
        pred, mag, _ = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"])
        fo.assert_exact_fp32("forward", mag)
        g, W = gcsr(c), c["W"].to(DEV)
        B = len(pred)
        for V in (c["V"].to(DEV), c["V"].to(DEV).to(BF)):
            for fn in (o.ffm_forward, o.ffm_forward_pp):
                ko.poison((B,), torch.float32, DEV)
                ko.check_bits("forward", fn(*g, W, V), pred.float())
        run_backward_variants("bwd", c, fo.ffm_backward_totals_ref(c))


def test_forward_long_row():
    """n = 1000 at K = 4: 499,500 pairs, the sqrt + fix-up of tri_decode at
    a large n, and many trips of the 2-deep pair pipeline (its edges, 64
    and 128 pairs, lie between the rows of 11 / 12 and 16 / 17 entries that
    every exact case holds)"""
    c = fo.long_row_case()
    pred, mag, _ = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"])
    fo.assert_exact_fp32("forward n=1000", mag)
    g, W = gcsr(c), c["W"].to(DEV)
    for V in (c["V"].to(DEV), c["V"].to(DEV).to(BF)):
        for fn in (ops().ffm_forward, ops().ffm_forward_pp):
            ko.check_bits("forward n=1000", fn(*g, W, V), pred.float())


# ---------------------------------------------------------------------------
# ffm_row_emit and the emit -> sort -> apply chain, exact set
# ---------------------------------------------------------------------------
def emit_oracle(c):
    """per-entry blocks and their totals, with the exactness conditions"""
    F, nf, K = c["V"].shape
    nnz = c["fids"].numel()
    gw64, blocks, mag, npart, _ = fo.ffm_entry_blocks_ref(
        *csr(c), c["V"], c["dpred"])
    fo.assert_exact_fp16("emit", blocks, c["scale"])
    fo.assert_exact_fp32("emit", mag * c["scale"])
    sf, pm = fo.sort_entries(c["fids"])
    tot = fo.ffm_totals_ref(sf, pm, blocks.reshape(nnz, -1), gw64, F)
    magV = fo.ffm_totals_ref(sf, pm, mag.reshape(nnz, -1), gw64, F)[1]
    return gw64, blocks, npart, (tot[0], tot[1], tot[2], magV), (sf, pm)


def run_emit_and_chain(name, c, v_bf16, oracle=None):
    """emit right after poisoning both output shapes; gw and every block
    element exact; unfed slots +0 bit for bit; then the f16 apply."""
    o = ops()
    F, nf, K = c["V"].shape
    D, scale = nf * K, c["scale"]
    nnz = c["fids"].numel()
    gw64, blocks, npart, totals, order = oracle or emit_oracle(c)
    g = gcsr(c)
    V = c["V"].to(DEV).to(BF) if v_bf16 else c["V"].to(DEV)
    d = c["dpred"].to(DEV)
    ko.poison((nnz,), torch.float32, DEV)
    ko.poison((nnz, D), torch.float16, DEV)
    gw, gblocks = o.ffm_row_emit(*g, V, d, scale=scale)
    assert gblocks.dtype == torch.float16
    ko.check_bits(name + ".gw", gw, gw64.float())
    fo.check_equal(name + ".gblocks", gblocks,
                   (blocks * scale).reshape(nnz, D).to(torch.float16))
    unfed = (npart == 0).unsqueeze(-1).expand(nnz, nf, K).reshape(nnz, D)
    got = gblocks.cpu()[unfed]
    ko.check_bits(name + ".unfed", got, torch.zeros_like(got))
    # chain: fid sort, then the f16 segment reduce into zeroed slabs
    sf, pm = (t.to(DEV) for t in order)
    gradW, gradV, touched = slabs(F, D)
    o.ffm_blocks_apply_f16(sf, pm, gblocks, gw, gradW, gradV, touched,
                           inv_scale=1.0 / scale)
    check_slabs(name + ".chain", gradW, gradV, touched, totals, c["fids"], F)
    return npart


@pytest.mark.parametrize("K,shape,kind", shape_kind_params(True))
def test_row_emit_and_chain_exact(K, shape, kind):
    one_entry = False
    for scale in fo.SCALES:
        for c in fo.exact_cases(K, shape, kind, scale=scale):
            oracle = emit_oracle(c)
            for v_bf16 in (False, True):
                npart = run_emit_and_chain(
                    f"emit.s{int(scale)}.{'bf16' if v_bf16 else 'fp32'}",
                    c, v_bf16, oracle)
            counts = (c["row_ptr"][1:] - c["row_ptr"][:-1])
            one_entry |= bool((counts == 1).any())
            # a one-entry row's block has no partner at all
            first = c["row_ptr"][:-1][counts == 1].long()
            assert (npart[first] == 0).all()
    assert one_entry


@pytest.mark.parametrize("K", fo.KS)
@pytest.mark.parametrize("B", fo.BATCHES)
def test_row_emit_batches(K, B):
    """1, 3, 4, 5 and 9 rows (the forward puts 4 rows in a block, the emit
    one), row kinds cycling, empty rows inside"""
    c = fo.batch_case(K, B)
    pred, mag, _ = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"])
    fo.assert_exact_fp32("forward", mag)
    ko.check_bits("forward", ops().ffm_forward(*gcsr(c), c["W"].to(DEV),
                                               c["V"].to(DEV)), pred.float())
    oracle = emit_oracle(c)
    for v_bf16 in (False, True):
        run_emit_and_chain(f"emit.B{B}", c, v_bf16, oracle)
    run_backward_variants(f"bwd.B{B}", c, oracle[3])


# ---------------------------------------------------------------------------
# ffm_blocks_apply_f16 on hand-built blocks: slab mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("D", fo.APPLY_DS)
@pytest.mark.parametrize("runs", list(fo.RUNS))
def test_apply_f16_slab_exact(D, runs):
    """opt_mode 0: gradW / gradV bit-exact on zeroed slabs, the bitmap
    holds exactly the unique fids, rows of other fids stay +0"""
    a = fo.apply_inputs(D, runs)
    F = a["F"]
    refW, refV, magW, magV = fo.ffm_totals_ref(
        a["sorted_fids"], a["perm"], a["gblocks"], a["gw"], F,
        a["inv_scale"])
    gradW, gradV, touched = slabs(F, D)
    ops().ffm_blocks_apply_f16(
        a["sorted_fids"].to(DEV), a["perm"].to(DEV), a["gblocks"].to(DEV),
        a["gw"].to(DEV), gradW, gradV, touched, inv_scale=a["inv_scale"])
    check_slabs("apply_f16", gradW, gradV, touched,
                (refW, refV, magW, magV / a["inv_scale"]),
                a["sorted_fids"], F)


# ---------------------------------------------------------------------------
# ffm_blocks_apply_f16 with the optimizer fused into interior runs
# ---------------------------------------------------------------------------
STATE = ("W", "V", "nW", "nV", "zW", "gradW", "gradV")


def fused_state(F, D, seed):
    g = torch.Generator().manual_seed(seed)
    return {"W": torch.randn(F, generator=g) * 0.1,
            "V": torch.randn(F, D, generator=g) * 0.1,
            "nW": torch.rand(F, generator=g),
            "nV": torch.rand(F, D, generator=g),
            "zW": torch.randn(F, generator=g) * 0.1,
            "gradW": torch.zeros(F), "gradV": torch.zeros(F, D)}


def snapshot(gpu):
    return {k: t.cpu().clone() for k, t in gpu.items()}


def full(shape, rows, val):
    t = torch.zeros(shape, dtype=torch.float64)
    t[rows] = val
    return t


def fused_oracle(before, uniq, totW, totV, mode):
    """{state name: (ref64 [F, ...], bound)} after one optimizer step on
    the rows `uniq` with the exact total gradient; other rows unchanged"""
    rV = ko.adagrad_ref(before["V"][uniq], totV[uniq], before["nV"][uniq],
                        **ADA)
    out = {"V": rV["W"], "nV": rV["n"]}
    if mode == 1:
        rW = ko.adagrad_ref(before["W"][uniq], totW[uniq],
                            before["nW"][uniq], **ADA)
        out.update(W=rW["W"], nW=rW["n"])
    else:
        rW = ko.ftrl_ref(before["W"][uniq], before["zW"][uniq],
                         before["nW"][uniq], totW[uniq], **ko.FTRL)
        out.update(W=rW["w"], zW=rW["z"], nW=rW["n"])
    res = {}
    for k, (ref, bound) in out.items():
        r = before[k].double().clone()
        r[uniq] = ref
        res[k] = (r, full(r.shape, uniq, bound))
    return res


@pytest.mark.parametrize("D", fo.FUSED_DS)
@pytest.mark.parametrize("mirror", [False, True], ids=["nomirror", "Vh"])
@pytest.mark.parametrize("mode", [1, 3], ids=["adagrad", "ftrlW"])
def test_apply_f16_fused(D, mirror, mode):
    """opt_mode 1 / 3 on the run lists of the slab test. The chunk size is
    not assumed: per unique fid exactly one of
      (a) bitmap bit set: state bitwise unchanged, slab = exact total;
      (b) bit clear: slab exactly +0, state = one optimizer step on the
          exact total within the short-chain bound, Vh = bf16(V) bitwise
    must hold, both must occur, other fids stay bitwise unchanged. Then the
    model's tail (bitmap_compact + sparse apply) must bring every unique
    fid to the oracle and leave the slabs all zero."""
    o = ops()
    seen = set()
    for runs in fo.RUNS:
        a = fo.apply_inputs(D, runs)
        F = a["F"]
        nnz = a["sorted_fids"].numel()
        totW, totV, _, _ = fo.ffm_totals_ref(
            a["sorted_fids"], a["perm"], a["gblocks"], a["gw"], F,
            a["inv_scale"])
        uniq = torch.unique(a["sorted_fids"].long())
        gpu = {k: t.to(DEV) for k, t in
               fused_state(F, D, 100 * D + 10 * mode + mirror).items()}
        if mirror:
            gpu["Vh"] = gpu["V"].to(BF)
        touched = torch.zeros((F + 63) // 64, dtype=torch.int64, device=DEV)
        before = snapshot(gpu)
        ref = fused_oracle(before, uniq, totW, totV, mode)
        wp = ((ADA["lr"], ADA["eps"], ADA["l2"], 0.0) if mode == 1 else
              tuple(ko.FTRL[k] for k in ("alpha", "beta", "l1", "l2")))
        o.ffm_blocks_apply_f16(
            a["sorted_fids"].to(DEV), a["perm"].to(DEV),
            a["gblocks"].to(DEV), a["gw"].to(DEV), gpu["gradW"],
            gpu["gradV"], touched, inv_scale=a["inv_scale"], opt_mode=mode,
            V=gpu["V"], W=gpu["W"], nW=gpu["nW"],
            zW=gpu["zW"] if mode == 3 else None, nV=gpu["nV"],
            Vh=gpu.get("Vh"), p0=wp[0], p1=wp[1], p2=wp[2], p3=wp[3],
            q0=ADA["lr"], q1=ADA["eps"], q2=ADA["l2"])
        after = snapshot(gpu)
        tw = touched.cpu()
        bit = torch.tensor([fo.bit_is_set(tw, int(f)) for f in uniq])
        seen |= set(bit.tolist())
        kept, done = uniq[bit], uniq[~bit]
        # no bit outside the batch
        assert torch.equal(tw, fo.touched_words(kept, F))
        # (a) and the fids outside the batch: state bitwise unchanged
        same = torch.ones(F, dtype=torch.bool)
        same[done] = False
        for k in after:
            if k not in ("gradW", "gradV"):
                ko.check_bits(f"fused.same.{k}", after[k][same],
                              before[k][same])
        # slabs: exact totals under (a), +0 everywhere else
        expW, expV = torch.zeros(F), torch.zeros(F, D)
        expW[kept] = totW[kept].float()
        expV[kept] = totV[kept].float()
        ko.check_bits("fused.gradW", after["gradW"], expW)
        ko.check_bits("fused.gradV", after["gradV"], expV)
        if mode == 1:
            ko.check_bits("fused.zW", after["zW"], before["zW"])
        # (b): one optimizer step on the exact total
        for k, (r, b) in ref.items():
            ko.check_bound(f"fused.{k}", after[k][done], r[done], b[done])
        if mirror:
            ko.check_bits("fused.Vh", after["Vh"][done],
                          after["V"][done].to(BF))
        # the model's tail
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        ubuf = torch.zeros(F, dtype=torch.int32, device=DEV)
        o.bitmap_compact(touched, ubuf, count)
        live = ubuf[: min(F, nnz)]
        if mode == 1:
            o.sparse_adagrad_apply(live, count, gpu["W"], gpu["V"],
                                   gpu["nW"], gpu["nV"], gpu["gradW"],
                                   gpu["gradV"], ADA["lr"], ADA["eps"],
                                   ADA["l2"], gpu.get("Vh"))
        else:
            zV = torch.zeros(F, D, device=DEV)
            o.sparse_ftrl_apply(live, count, gpu["W"], gpu["V"], gpu["zW"],
                                gpu["nW"], zV, gpu["nV"], gpu["gradW"],
                                gpu["gradV"], ko.FTRL["alpha"],
                                ko.FTRL["beta"], ko.FTRL["l1"],
                                ko.FTRL["l2"], 1, ADA["lr"], ADA["eps"],
                                ADA["l2"], gpu.get("Vh"))
        assert int(count.item()) == kept.numel()
        final = snapshot(gpu)
        for k, (r, b) in ref.items():
            ko.check_bound(f"fused.tail.{k}", final[k], r, b)
        if mirror:
            ko.check_bits("fused.tail.Vh", final["Vh"][uniq],
                          final["V"][uniq].to(BF))
        ko.check_bits("fused.tail.gradW", final["gradW"], torch.zeros(F))
        ko.check_bits("fused.tail.gradV", final["gradV"],
                      torch.zeros(F, D))
    assert seen == {True, False}


# ---------------------------------------------------------------------------
# chunk edges of the sorted walk (32) and the fp32 block apply (64)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,nf", [(K, fo.SHAPES[K]["q1"]) for K in fo.KS]
                         + [(16, 65), (64, 80)])
def test_backward_variants_run_edges(K, nf):
    """a CSR whose fid-sorted order has runs of 31, 1, 32, 33, 31, 70, 2:
    runs that end on, start on and span the 32-entry chunks of the sorted
    walk. nfields = 65, K = 16 is D = 1040, past the f16 apply's cap.
    nfields = 80, K = 64 asks for 83,200 bytes of dynamic LDS in the sorted
    walk and the block emit and 81,920 in the fp32 block apply: above
    64 KB, inside the 160 KB a gfx950 block can get."""
    c = fo.csr_from_runs(fo.SORTED_RUNS, nf, K, seed=1000 * nf + K,
                         F=256 if nf * K > 2048 else fo.F_TABLE)
    run_backward_variants("runs", c, fo.ffm_backward_totals_ref(c))


def test_row_index():
    lengths = [0, 1, 63, 64, 65, 0, 130, 0]
    row_ptr, _, _ = ko.make_csr(lengths)
    row, _, _ = ko.rows_pos(row_ptr)
    nnz = int(row_ptr[-1])
    rp = row_ptr.to(DEV)
    poison_i32(nnz)
    out = ops().row_index(rp, nnz)
    assert torch.equal(out.cpu(), row.to(torch.int32))


# ---------------------------------------------------------------------------
# float set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", fo.KS)
def test_float_set(K):
    """random V ~ 0.1 N(0,1), x in [0.5, 1.5]: the forward under the sum
    rule, the row emit under the bound derived in ffm_oracles.row_emit_bound
    (scale 1 and 128), fp32 and bf16 V"""
    o = ops()
    c = fo.float_emit_case(K)
    F, nf, _ = c["V"].shape
    nnz = c["fids"].numel()
    g, W, d = gcsr(c), c["W"].to(DEV), c["dpred"].to(DEV)
    for v_bf16 in (False, True):
        Vg = c["V"].to(DEV).to(BF) if v_bf16 else c["V"].to(DEV)
        Vc = Vg.float().cpu()
        tag = "bf16" if v_bf16 else "fp32"
        pred, mag, nterms = fo.ffm_forward_ref64(*csr(c), c["W"], Vc)
        ko.check_bound(f"ffm_forward.{tag}", o.ffm_forward(*g, W, Vg), pred,
                       nterms * ko.U23 * mag)
        gw64, blocks, bmag, npart, cmag = fo.ffm_entry_blocks_ref(
            *csr(c), Vc, c["dpred"])
        for scale in (1.0, 128.0):
            ko.poison((nnz,), torch.float32, DEV)
            ko.poison((nnz, nf * K), torch.float16, DEV)
            gw, gblocks = o.ffm_row_emit(*g, Vg, d, scale=scale)
            ko.check_bits("ffm_row_emit.gw", gw,
                          c["dpred"][ko.rows_pos(c["row_ptr"])[0]]
                          * c["vals"])
            ko.check_bound(
                f"ffm_row_emit.{tag}.s{int(scale)}",
                gblocks.double() / scale, blocks.reshape(nnz, -1),
                fo.row_emit_bound(bmag, npart, cmag, scale, not v_bf16))


# ---------------------------------------------------------------------------
# what the bindings refuse
# ---------------------------------------------------------------------------
def tiny(nf, K, F=16):
    """a valid two-row CSR on an all-zero [F, nf, K] table"""
    row_ptr, fields, fids, vals = fo.make_ffm_csr(
        [[(1, 0, 1.0), (2, nf - 1, 1.0)], [(3, 0, 1.0)]])
    return {"g": tuple(t.to(DEV) for t in (row_ptr, fields, fids, vals)),
            "W": torch.zeros(F, device=DEV),
            "V": torch.zeros(F, nf, K, device=DEV),
            "d": torch.ones(2, device=DEV), "F": F,
            "sf": torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV),
            "pm": torch.tensor([0, 1, 2], dtype=torch.int32, device=DEV),
            "roe": torch.tensor([0, 0, 1], dtype=torch.int32, device=DEV)}


def each_v_binding(t):
    """every FFM binding that dispatches on V's K"""
    o = ops()
    F, nf, K = t["V"].shape
    gradW, gradV, touched = slabs(F, nf * K)
    gV3 = gradV.view(F, nf, K)
    yield lambda: o.ffm_forward(*t["g"], t["W"], t["V"])
    yield lambda: o.ffm_forward_pp(*t["g"], t["W"], t["V"])
    yield lambda: o.ffm_row_emit(*t["g"], t["V"], t["d"])
    yield lambda: o.ffm_backward(*t["g"], t["V"], t["d"], gradW, gV3,
                                 touched)
    yield lambda: o.ffm_sorted_backward(t["sf"], t["pm"], t["roe"], *t["g"],
                                        t["V"], t["d"], gradW, gV3, touched)
    yield lambda: o.ffm_block_emit(t["roe"], *t["g"], t["V"], t["d"])


def test_bindings_raise_on_unsupported_k():
    for call in each_v_binding(tiny(3, 5)):
        with pytest.raises(RuntimeError, match="4, 8, 16, 32, 64"):
            call()


@pytest.mark.parametrize("D,width,msg", [(6, 6, "unsupported"),
                                         (1028, 1028, "unsupported"),
                                         (8, 12, "width")])
def test_apply_f16_raises_on_bad_width(D, width, msg):
    t = tiny(1, 4)
    gradW, gradV, touched = slabs(t["F"], D)
    gblocks = torch.zeros(3, width, dtype=torch.float16, device=DEV)
    with pytest.raises(RuntimeError, match=msg):
        ops().ffm_blocks_apply_f16(t["sf"], t["pm"], gblocks,
                                   torch.zeros(3, device=DEV), gradW, gradV,
                                   touched)
    torch.cuda.synchronize()
    assert not gradV.any()


def test_lds_over_request_is_refused():
    """ffm_sorted_backward and ffm_block_emit ask for 16 nfields (K+1)
    bytes of dynamic LDS, ffm_blocks_apply for 16 D. The first shape past
    the device's per-block limit (at K = 64 that is nfields = 158 on a
    160 KB device) makes each binding raise before any launch, and the
    model refuses the pair at construction."""
    o = ops()
    limit = o.ffm_max_lds_per_block()
    assert limit >= (64 << 10)
    nf = limit // (16 * 65) + 1
    assert o.ffm_block_lds_bytes(nf, 64) > limit
    assert o.ffm_block_lds_bytes(nf - 1, 64) <= limit
    t = tiny(nf, 64)
    gradW, gradV, touched = slabs(t["F"], nf * 64)
    with pytest.raises(RuntimeError, match="LDS"):
        o.ffm_sorted_backward(t["sf"], t["pm"], t["roe"], *t["g"], t["V"],
                              t["d"], gradW, gradV.view(t["F"], nf, 64),
                              touched)
    with pytest.raises(RuntimeError, match="LDS"):
        o.ffm_block_emit(t["roe"], *t["g"], t["V"], t["d"])
    D = limit // 16 + 1
    with pytest.raises(RuntimeError, match="LDS"):
        o.ffm_blocks_apply(t["sf"], t["pm"], torch.zeros(3, D, device=DEV),
                           torch.zeros(3, device=DEV), gradW,
                           torch.zeros(t["F"], D, device=DEV), touched)
    with pytest.raises(ValueError, match="LDS"):
        FFMModel(FFMHyper(num_features=16, num_fields=nf, k=64), device=DEV)
    torch.cuda.synchronize()
    assert not gradV.any() and not gradW.any() and not touched.any()


def test_model_trains_on_the_largest_issue_shape():
    """num_fields = 80, k = 64 selects the sorted walk with 83,200 bytes of
    LDS per block, above 64 KB and inside the device's limit: the step must
    move W and V of every feature of the batch (the kernels' numbers at
    this shape are held exactly in test_backward_variants_run_edges)."""
    F, nf, B = 256, 80, 8
    m = FFMModel(FFMHyper(num_features=F, num_fields=nf, k=64), device=DEV)
    assert m.backward_mode == "sorted"
    g = torch.Generator().manual_seed(80064)
    fields = torch.arange(nf, dtype=torch.int32).repeat(B).to(DEV)
    fids = torch.randint(0, F, (B * nf,), generator=g,
                         dtype=torch.int32).to(DEV)
    vals = torch.ones(B * nf, device=DEV)
    row_ptr = (torch.arange(B + 1, dtype=torch.int32) * nf).to(DEV)
    labels = (torch.rand(B, generator=g) > 0.5).float().to(DEV)
    W0, V0 = m.W.clone(), m.V.clone()
    loss = m.train_step(row_ptr, fields, fids, vals, labels)
    assert torch.isfinite(loss).all() and torch.isfinite(m.V).all()
    live = torch.unique(fids).long()
    assert (m.W[live] != W0[live]).all()
    assert (m.V[live] != V0[live]).any(dim=(1, 2)).all()
