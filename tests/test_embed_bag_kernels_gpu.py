"""Parity tests for the field-addressed embedding-bag kernels
(embed_bag_kernels.hip) against the float64 oracles of
``embed_bag_oracles.py``.

Main set: small-integer inputs on which every quantity is reproduced exactly
(conditions stated and asserted in ``embed_bag_oracles``), so the comparisons
are bit or value equality: against the oracle, against the position kernels
on the rows where the two layouts coincide, between the fused DeepFM pair and
the composed bindings, and under a permutation of the entries of every row.
Rows with and without a shared slot take the staged and the direct path of
the forward; both are in every batch. A float case per K keeps real rounding
in view under derived bounds and checks that two launches agree bit for bit.
``test_embed_bag_oracles.py`` shows on the CPU that the wrong references
listed in docs/TESTING.md differ on these same inputs.
"""

import pytest
import torch

import embed_bag_oracles as bo
import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def view_on_gpu(t, fill):
    buf, o = bo.padded(t, fill)
    return buf.to(DEV)[o:o + t.numel()]


def up(c):
    """Upload a case: fields / fids / vals are views; the ints around fids
    name fid F-1 (NaN rows of W and E), the fields around the view name slot
    0 and the floats around vals are NaN, so an entry read past either end of
    a row's range lands in the outputs as NaN"""
    return {"row_ptr": c["row_ptr"].to(DEV),
            "fields": view_on_gpu(c["fields"], 0),
            "fids": view_on_gpu(c["fids"], c["F"] - 1),
            "vals": view_on_gpu(c["vals"], NAN),
            "W": c["W"].to(DEV), "E": c["E"].to(DEV),
            "dpred": c["dpred"].to(DEV), "dDeep": c["dDeep"].to(DEV)}


def bag_forward(g, c, pooling):
    ko.poison((c["B"], c["nf"] * c["K"]), torch.bfloat16, DEV)
    return ops().embed_bag_forward(g["row_ptr"], g["fields"], g["fids"],
                                   g["vals"], g["E"], c["nf"], pooling)


def fused_forward(g, c, pooling):
    B, K, nf = c["B"], c["K"], c["nf"]
    ko.poison((B,), torch.float32, DEV)
    ko.poison((B, K), torch.float32, DEV)
    ko.poison((B, nf * K), torch.bfloat16, DEV)
    return ops().deepfm_bag_forward(g["row_ptr"], g["fields"], g["fids"],
                                    g["vals"], g["W"], g["E"], nf, pooling)


def bag_emit(g, c, pooling):
    nnz, K = c["fids"].numel(), c["K"]
    ko.poison((nnz,), torch.float32, DEV)
    ko.poison((nnz, K), torch.float32, DEV)
    return ops().embed_bag_backward_emit(
        g["row_ptr"], g["fields"], g["vals"], g["dDeep"], g["dpred"],
        c["nf"], K, pooling)


def fused_emit(g, c, sumVX, pooling, dpred=None):
    nnz, K = c["fids"].numel(), c["K"]
    ko.poison((nnz,), torch.float32, DEV)
    ko.poison((nnz, K), torch.float32, DEV)
    return ops().deepfm_bag_backward_emit(
        g["row_ptr"], g["fields"], g["fids"], g["vals"], g["E"], sumVX,
        g["dDeep"], g["dpred"] if dpred is None else dpred, c["nf"],
        pooling)


def fargs(c):
    return (c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"], c["nf"])


def fm_ref(c):
    return bo.do.deepfm_forward_ref(c["row_ptr"], c["fids"], c["vals"],
                                    c["W"], c["E"], c["nf"])


@pytest.mark.parametrize("nf", bo.NFS)
@pytest.mark.parametrize("K", bo.KS)
def test_forward_exact(K, nf):
    """Concat, fm and sumVX bit for bit against the oracle, empty slots +0,
    and the fused forward bit for bit against fm_forward +
    embed_bag_forward"""
    for i, c in enumerate(bo.exact_cases(K, nf)):
        bo.assert_exact(c)
        g = up(c)
        ref = fm_ref(c)
        for pooling in bo.POOLINGS:
            name = f"K{K}.nf{nf}.case{i}.pool{pooling}"
            want = bo.concat_expect(*fargs(c), pooling)
            deep = bag_forward(g, c, pooling)
            ko.check_bits(name + ".concat", deep, want)
            _, _, cnt = bo.concat_ref(*fargs(c), pooling)
            empty = (cnt == 0).view(c["B"], nf, 1).expand(-1, -1, K)
            bits = deep.cpu().view(torch.int16).view(c["B"], nf, K)
            assert bool((bits[empty] == 0).all()), name + ": empty slot"
            fm, sumVX, deep2 = fused_forward(g, c, pooling)
            ko.check_bits(name + ".fm", fm, ref["fm"][0].float() + 0.0)
            ko.check_bits(name + ".sumVX", sumVX,
                          ref["sumVX"][0].float() + 0.0)
            ko.check_bits(name + ".fused concat", deep2, want)
            # composed: fm_forward beside the bag
            ko.poison((c["B"],), torch.float32, DEV)
            ko.poison((c["B"], K), torch.float32, DEV)
            pred2, sumVX2 = ops().fm_forward(g["row_ptr"], g["fids"],
                                             g["vals"], g["W"], g["E"])
            ko.check_bits(name + ".fm vs fm_forward", fm, pred2.cpu())
            ko.check_bits(name + ".sumVX vs fm_forward", sumVX, sumVX2.cpu())
            ko.check_bits(name + ".concat vs embed_bag", deep2, deep.cpu())


@pytest.mark.parametrize("nf", bo.NFS)
@pytest.mark.parametrize("K", bo.KS)
def test_emit_exact(K, nf):
    """gw bit for bit, gv by value against the oracle; the fused emit bit
    for bit against fm_backward_emit + embed_bag_backward_emit summed, under
    both poolings (Dm = fl(D inv); d (s - e x) = t is exact and x is 1 or 2,
    so Dm x and t x are exact and fl(Dm x + t x) = fl(Dm + t) x: one
    rounding either way); entries outside [0, nf) get the pure FM emit"""
    for i, c in enumerate(bo.exact_cases(K, nf)):
        g = up(c)
        nnz = c["fids"].numel()
        sv32 = bo.case_sumvx32(c)
        sumVX = sv32.to(DEV)
        ko.poison((nnz,), torch.float32, DEV)
        ko.poison((nnz, K), torch.float32, DEV)
        gw_fm, gv_fm = ops().fm_backward_emit(
            g["row_ptr"], g["fids"], g["vals"], g["E"], sumVX, g["dpred"],
            None)
        for pooling in bo.POOLINGS:
            name = f"K{K}.nf{nf}.case{i}.pool{pooling}"
            gw64, gv64, _ = bo.embed_bag_emit_ref(
                c["row_ptr"], c["fields"], c["vals"], c["dDeep"], c["dwide"],
                nf, K, pooling)
            gw_b, gv_b = bag_emit(g, c, pooling)
            ko.check_bits(name + ".bag gw", gw_b, gw64.float())
            bo.check_value(name + ".bag gv", gv_b, gv64)
            gw64, gv64, _ = bo.deepfm_bag_emit_ref(
                c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"],
                sv32, c["dDeep"], c["dpred"], nf, pooling)
            gw, gv = fused_emit(g, c, sumVX, pooling)
            ko.check_bits(name + ".gw", gw, gw64.float())
            bo.check_value(name + ".gv", gv, gv64)
            ko.check_bits(name + ".gw vs fm_backward_emit", gw, gw_fm.cpu())
            ko.check_bits(name + ".gv vs composed", gv,
                          (gv_fm + gv_b).cpu())
            f = c["fields"]
            out = (f < 0) | (f >= nf)
            assert torch.equal(gv.cpu()[out], gv_fm.cpu()[out]), name
            assert bool((gv_b.cpu()[out] == 0).all()), name
            # d = 0: the fused emit is the bag emit
            zero = torch.zeros_like(g["dpred"])
            _, gv0 = fused_emit(g, c, sumVX, pooling, dpred=zero)
            assert torch.equal(gv0.cpu() + 0.0, gv_b.cpu() + 0.0), name


@pytest.mark.parametrize("nf", bo.NFS)
@pytest.mark.parametrize("K", bo.KS)
def test_position_equivalence(K, nf):
    """Rows whose fields are 0..len-1 in order, len <= nf, sum pooling, no
    zero product (``position_cases`` keeps zeros out of E, so no -0 product
    meets a +0 accumulator): all four kernels are bit-equal to embed_gather,
    embed_backward_emit, deepfm_forward and deepfm_backward_emit"""
    for i, c in enumerate(bo.position_cases(K, nf)):
        g = up(c)
        name = f"K{K}.nf{nf}.case{i}"
        nnz = c["fids"].numel()
        sumVX = bo.case_sumvx32(c).to(DEV)
        deep = bag_forward(g, c, 0)
        fm, s, deep2 = fused_forward(g, c, 0)
        ko.poison((c["B"], nf * K), torch.bfloat16, DEV)
        want = ops().embed_gather(g["row_ptr"], g["fids"], g["vals"],
                                  g["E"], nf)
        ko.check_bits(name + ".embed_gather", deep, want.cpu())
        fm0, s0, deep0 = ops().deepfm_forward(g["row_ptr"], g["fids"],
                                              g["vals"], g["W"], g["E"], nf)
        ko.check_bits(name + ".deepfm_forward fm", fm, fm0.cpu())
        ko.check_bits(name + ".deepfm_forward sumVX", s, s0.cpu())
        ko.check_bits(name + ".deepfm_forward concat", deep2, deep0.cpu())
        gw, gv = bag_emit(g, c, 0)
        ko.poison((nnz,), torch.float32, DEV)
        ko.poison((nnz, K), torch.float32, DEV)
        gw0, gv0 = ops().embed_backward_emit(g["row_ptr"], g["vals"],
                                             g["dDeep"], g["dpred"], nf, K)
        ko.check_bits(name + ".embed_backward_emit gw", gw, gw0.cpu())
        ko.check_bits(name + ".embed_backward_emit gv", gv, gv0.cpu())
        gw, gv = fused_emit(g, c, sumVX, 0)
        ko.poison((nnz,), torch.float32, DEV)
        ko.poison((nnz, K), torch.float32, DEV)
        gw0, gv0 = ops().deepfm_backward_emit(
            g["row_ptr"], g["fids"], g["vals"], g["E"], sumVX, g["dDeep"],
            g["dpred"], nf)
        ko.check_bits(name + ".deepfm_backward_emit gw", gw, gw0.cpu())
        ko.check_bits(name + ".deepfm_backward_emit gv", gv, gv0.cpu())


@pytest.mark.parametrize("K", bo.KS)
def test_permutation_invariance(K):
    """Permuting the entries inside every row leaves concat, fm and sumVX
    bit-equal on the exact set and permutes gw and gv; the position kernels
    do change on the same permuted input, which keeps this test honest"""
    position_moved = 0
    for nf in bo.NFS:
        for i, c in enumerate(bo.exact_cases(K, nf)):
            cp, perm = bo.permuted(c, 31 + i)
            g, gp = up(c), up(cp)
            sumVX = bo.case_sumvx32(c).to(DEV)
            for pooling in bo.POOLINGS:
                name = f"K{K}.nf{nf}.case{i}.pool{pooling}"
                fm, s, deep = fused_forward(g, c, pooling)
                fm_p, s_p, deep_p = fused_forward(gp, cp, pooling)
                ko.check_bits(name + ".concat", deep_p, deep.cpu())
                ko.check_bits(name + ".fm", fm_p, fm.cpu())
                ko.check_bits(name + ".sumVX", s_p, s.cpu())
                ko.check_bits(name + ".bag concat",
                              bag_forward(gp, cp, pooling),
                              bag_forward(g, c, pooling).cpu())
                gw, gv = fused_emit(g, c, sumVX, pooling)
                gw_p, gv_p = fused_emit(gp, cp, sumVX, pooling)
                ko.check_bits(name + ".gw", gw_p, gw.cpu()[perm])
                assert torch.equal(gv_p.cpu() + 0.0, gv.cpu()[perm] + 0.0)
                gw, gv = bag_emit(g, c, pooling)
                gw_p, gv_p = bag_emit(gp, cp, pooling)
                ko.check_bits(name + ".bag gw", gw_p, gw.cpu()[perm])
                ko.check_bits(name + ".bag gv", gv_p, gv.cpu()[perm])
            a = ops().embed_gather(g["row_ptr"], g["fids"], g["vals"],
                                   g["E"], nf)
            b = ops().embed_gather(gp["row_ptr"], gp["fids"], gp["vals"],
                                   gp["E"], nf)
            position_moved += int(not torch.equal(a.cpu().view(torch.int16),
                                                  b.cpu().view(torch.int16)))
    assert position_moved >= 1


@pytest.mark.parametrize("K", bo.KS)
def test_float_set(K):
    """Real rounding: concat, sumVX, fm and gv inside their derived bounds,
    gw bit for bit; two launches of every kernel are bit-equal"""
    c = bo.float_case(K)
    g = up(c)
    nf = c["nf"]
    ref = fm_ref(c)
    sv32 = ref["sumVX"][0].float()
    sumVX = sv32.to(DEV)
    row, _, _ = ko.rows_pos(c["row_ptr"])
    for pooling in bo.POOLINGS:
        name = f"K{K}.pool{pooling}"
        val, bound, _ = bo.concat_ref(*fargs(c), pooling)
        fm, s, deep = fused_forward(g, c, pooling)
        ko.check_bound(name + ".concat", deep.float(), val, bound)
        ko.check_bound(name + ".sumVX", s, *ref["sumVX"])
        ko.check_bound(name + ".fm", fm, *ref["fm"])
        deep_b = bag_forward(g, c, pooling)
        ko.check_bits(name + ".bag concat", deep_b, deep.cpu())
        fm2, s2, deep2 = fused_forward(g, c, pooling)
        ko.check_bits(name + ".fm again", fm2, fm.cpu())
        ko.check_bits(name + ".sumVX again", s2, s.cpu())
        ko.check_bits(name + ".concat again", deep2, deep.cpu())
        ko.check_bits(name + ".bag again", bag_forward(g, c, pooling),
                      deep_b.cpu())

        gw64, gv64, gb = bo.deepfm_bag_emit_ref(
            c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"], sv32,
            c["dDeep"], c["dpred"], nf, pooling)
        gw, gv = fused_emit(g, c, sumVX, pooling)
        ko.check_bits(name + ".gw", gw, c["dpred"][row] * c["vals"])
        ko.check_bound(name + ".gv", gv, gv64, gb)
        gw2, gv2 = fused_emit(g, c, sumVX, pooling)
        ko.check_bits(name + ".gw again", gw2, gw.cpu())
        ko.check_bits(name + ".gv again", gv2, gv.cpu())
        gw64, gv64, gb = bo.embed_bag_emit_ref(
            c["row_ptr"], c["fields"], c["vals"], c["dDeep"], c["dwide"],
            nf, K, pooling)
        gw, gv = bag_emit(g, c, pooling)
        ko.check_bits(name + ".bag gw", gw, c["dwide"][row] * c["vals"])
        ko.check_bound(name + ".bag gv", gv, gv64, gb)
        gw2, gv2 = bag_emit(g, c, pooling)
        ko.check_bits(name + ".bag gv again", gv2, gv.cpu())


@pytest.mark.parametrize("K", bo.KS)
def test_empty_batch(K):
    """B = 0 returns empty tensors and launches nothing; the checked launch
    that follows reports nothing"""
    c = bo.case(K, [], 5, 1)
    g = up(c)
    for pooling in bo.POOLINGS:
        deep = ops().embed_bag_forward(g["row_ptr"], g["fields"], g["fids"],
                                       g["vals"], g["E"], 5, pooling)
        assert deep.shape == (0, 5 * K) and deep.dtype == torch.bfloat16
        fm, sumVX, deep = ops().deepfm_bag_forward(
            g["row_ptr"], g["fields"], g["fids"], g["vals"], g["W"], g["E"],
            5, pooling)
        assert fm.shape == (0,) and sumVX.shape == (0, K)
        assert deep.shape == (0, 5 * K)
        gw, gv = ops().deepfm_bag_backward_emit(
            g["row_ptr"], g["fields"], g["fids"], g["vals"], g["E"], sumVX,
            g["dDeep"], g["dpred"], 5, pooling)
        assert gw.shape == (0,) and gv.shape == (0, K)
        gw, gv = ops().embed_bag_backward_emit(
            g["row_ptr"], g["fields"], g["vals"], g["dDeep"], g["dpred"], 5,
            K, pooling)
        assert gw.shape == (0,) and gv.shape == (0, K)
        c1 = bo.case(K, [[1, 1, 4]], 5, 2)
        ko.check_bits("after empty", bag_forward(up(c1), c1, pooling),
                      bo.concat_expect(*fargs(c1), pooling))


# ---------------------------------------------------------------------------
# argument checks: every bad argument raises before anything is launched,
# and a good call follows each
# ---------------------------------------------------------------------------
def test_binding_checks():
    K, nf = 4, 3
    c = bo.case(K, [[0, 2, 2], [], [1, 5]], nf, 77)
    g = up(c)
    sumVX = bo.case_sumvx32(c).to(DEV)
    B, F = c["B"], c["F"]
    gen = torch.Generator().manual_seed(78)
    E5 = torch.randn(F, 5, generator=gen).to(DEV)
    base = dict(row_ptr=g["row_ptr"], fields=g["fields"], fids=g["fids"],
                vals=g["vals"], W=g["W"], E=g["E"], sumVX=sumVX,
                dDeep=g["dDeep"], dpred=g["dpred"], nf=nf, K=K, pooling=1)

    def bag_fwd(a):
        return ops().embed_bag_forward(a["row_ptr"], a["fields"], a["fids"],
                                       a["vals"], a["E"], a["nf"],
                                       a["pooling"])

    def bag_bwd(a):
        return ops().embed_bag_backward_emit(
            a["row_ptr"], a["fields"], a["vals"], a["dDeep"], a["dpred"],
            a["nf"], a["K"], a["pooling"])

    def fus_fwd(a):
        return ops().deepfm_bag_forward(
            a["row_ptr"], a["fields"], a["fids"], a["vals"], a["W"], a["E"],
            a["nf"], a["pooling"])

    def fus_bwd(a):
        return ops().deepfm_bag_backward_emit(
            a["row_ptr"], a["fields"], a["fids"], a["vals"], a["E"],
            a["sumVX"], a["dDeep"], a["dpred"], a["nf"], a["pooling"])

    want = bo.concat_expect(*fargs(c), 1)
    gw_want = (c["dpred"][ko.rows_pos(c["row_ptr"])[0]] * c["vals"])

    def good():
        ko.poison((B, nf * K), torch.bfloat16, DEV)
        ko.check_bits("good.bag", bag_fwd(base), want)
        ko.check_bits("good.fused", fus_fwd(base)[2], want)
        ko.check_bits("good.bag gw", bag_bwd(base)[0], gw_want)
        ko.check_bits("good.fused gw", fus_bwd(base)[0], gw_want)

    good()
    # for every op: fields, pooling, nf, and the LDS limit (not launched)
    nf_big = bo.nf_past_lds(K)
    assert bo.lds_bytes(nf_big, K) > bo.LDS_LIMIT
    big_dDeep = torch.zeros(B, nf_big * K, device=DEV)
    common = [
        dict(fields=g["fields"].long()),                   # dtype
        dict(fields=g["fields"][:-1]),                     # length
        dict(fields=g["fields"].cpu()),                    # device
        dict(fields=torch.stack([g["fields"]] * 2, 1)[:, 0]),  # contiguity
        dict(pooling=2), dict(pooling=-1),
        dict(nf=0),
        dict(nf=nf_big, dDeep=big_dDeep),                  # past the LDS
        dict(row_ptr=g["row_ptr"][:0]),
        dict(row_ptr=g["row_ptr"].long()),
        dict(vals=g["vals"][:-1]),
        dict(vals=g["vals"].double()),
    ]
    for fn in (bag_fwd, bag_bwd, fus_fwd, fus_bwd):
        for kw in common:
            with pytest.raises(RuntimeError):
                fn({**base, **kw})
            good()
    with pytest.raises(RuntimeError, match="needs .* bytes of LDS"):
        bag_fwd({**base, "nf": nf_big})
    good()

    with_e = [
        dict(E=E5), dict(E=g["E"].flatten()), dict(E=g["E"].double()),
        dict(E=g["E"].cpu()), dict(E=g["E"].t().contiguous().t()),
        dict(fids=g["fids"].long()), dict(fids=g["fids"].cpu()),
    ]
    for fn in (bag_fwd, fus_fwd, fus_bwd):
        for kw in with_e:
            with pytest.raises(RuntimeError):
                fn({**base, **kw})
            good()
    for kw in (dict(W=g["W"][:-1]), dict(W=g["W"].double())):
        with pytest.raises(RuntimeError):
            fus_fwd({**base, **kw})
        good()
    bad_emit = [
        dict(dDeep=g["dDeep"].flatten()),                  # not [B, nf*K]
        dict(dDeep=g["dDeep"][:, :-1].contiguous()),
        dict(dDeep=g["dDeep"][:, :-1]),                    # contiguity
        dict(dDeep=g["dDeep"].double()),
        dict(dpred=g["dpred"][:-1]),                       # not [B]
        dict(dpred=g["dpred"].unsqueeze(1)),
        dict(dpred=g["dpred"].cpu()),
        dict(nf=nf + 1),                                   # dDeep mismatch
    ]
    for fn in (bag_bwd, fus_bwd):
        for kw in bad_emit:
            with pytest.raises(RuntimeError):
                fn({**base, **kw})
            good()
    for kw in (dict(sumVX=sumVX.flatten()), dict(sumVX=sumVX[:-1]),
               dict(sumVX=sumVX.double()), dict(sumVX=sumVX.cpu())):
        with pytest.raises(RuntimeError):
            fus_bwd({**base, **kw})
        good()
    with pytest.raises(RuntimeError, match="K must be one of"):
        bag_bwd({**base, "K": 5})
    good()
