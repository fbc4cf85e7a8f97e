"""CPU checks of the float64 oracles in ``kernel_oracles.py`` and of the
bounds the GPU parity tests assert.

Self-consistency: each oracle agrees with the project's fp32 CPU path
(`WideDeepModel._gather_cpu`, the `NFMModel` CPU branch,
`DenseLayer.backward_cpu`, the CPU branch of `apply_grads`, `fm_ref.*`)
within the bound it hands to the GPU tests.

Mutation sensitivity: on the GPU tests' own inputs, a deliberately wrong
reference differs from the right one by more than the bound in at least
one element. A bound that hid one of these mistakes would make its GPU
test meaningless; the cure is different inputs, never a different bound.
"""

import pytest
import torch

import kernel_oracles as ko
from lightctr_amd.models.mlp import DenseLayer
from lightctr_amd.models.nfm import NFMHyper, NFMModel
from lightctr_amd.models.wide_deep import WideDeepHyper, WideDeepModel
from lightctr_amd.ops import fm_ref

BF = torch.bfloat16


def inside(name, out, ref64, bound):
    """the fp32 CPU path sits within the bound of the float64 oracle"""
    err = (out.double().reshape(ref64.shape) - ref64).abs()
    assert (err <= bound.reshape(ref64.shape)).all(), \
        (name, float(err.max()), float(bound.max()))


# ---------------------------------------------------------------------------
# self-consistency with the project's CPU paths
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", ko.EMBED_KS)
@pytest.mark.parametrize("nf", [1, 5, 39])
def test_gather_oracle_equals_gather_cpu(K, nf):
    for lengths, seed in ko.length_cases(K):
        d = ko.embed_inputs(K, lengths, seed)
        model = WideDeepModel(WideDeepHyper(num_features=ko.F_TABLE,
                                            num_fields=nf, k=K, hidden=(4,)))
        model.E.copy_(d["E"])
        cpu = model._gather_cpu(d["row_ptr"], d["fids"], d["vals"])
        ko.check_bits("gather_cpu", cpu.to(BF), ko.embed_gather_expect(
            d["row_ptr"], d["fids"], d["vals"], d["E"], nf))


@pytest.mark.parametrize("K", ko.EMBED_KS)
def test_nfm_oracles_match_nfm_cpu_branch(K):
    for ls, seed, dup in ko.nfm_cases(K, base=1000):
        d = ko.embed_inputs(K, ls, seed, dup_row=dup)
        model = NFMModel(NFMHyper(num_features=ko.F_TABLE, k=K, hidden=(4,)))
        model.W.copy_(d["W"])
        model.V.copy_(d["E"])
        _, (wide, sumVX, vec) = model._forward_cpu(
            d["row_ptr"], d["fids"], d["vals"], train=False)
        ref = ko.nfm_forward_ref(d["row_ptr"], d["fids"], d["vals"], d["W"],
                                 d["E"])
        inside("wide", wide, *ref["wide"])
        inside("sumVX", sumVX, *ref["sumVX"])
        inside("vec", vec, *ref["vec"])
        w_ref, w_bound = ko.wide_forward_ref(d["row_ptr"], d["fids"],
                                             d["vals"], d["W"])
        inside("wide_forward", wide, w_ref, w_bound)
        # backward: the expression of NFMModel.train_step's CPU branch
        row, _, _ = ko.rows_pos(d["row_ptr"])
        x = d["vals"].unsqueeze(1)
        sv = ref["sumVX"][0].float()
        gv32 = (sv[row] - d["E"][d["fids"].long()] * x) * x * d["dvec"][row]
        gw, gv, bound = ko.nfm_backward_emit_ref(
            d["row_ptr"], d["fids"], d["vals"], d["E"], sv, d["dvec"],
            d["dwide"])
        inside("nfm gv", gv32, gv, bound)
        assert torch.equal(gw, d["dwide"][row] * d["vals"])


@pytest.mark.parametrize("act", ["none", "relu", "sigmoid"])
def test_act_and_colsum_oracles_match_backward_cpu(act):
    g = torch.Generator().manual_seed(3)
    la = DenseLayer(7, 5, act=act, device="cpu")
    x = torch.randn(129, 7, generator=g)
    la.forward(x, train=True)
    dy = torch.randn(129, 5, generator=g)
    la.backward(dy)
    act_id = {"none": 0, "relu": 1, "sigmoid": 2}[act]
    ref, bound = ko.act_backward_ref(dy, la._y, act_id)
    if bound is None:
        dZ = ref
    else:
        dZ = (dy * la._y * (1 - la._y))
        inside("act sigmoid", dZ, ref, bound)
    db_ref, db_bound = ko.colsum_ref(dZ)
    inside("colsum", la._db, db_ref, db_bound)


@pytest.mark.parametrize("opt", ["adam", "adagrad"])
@pytest.mark.parametrize("l2", [0.0, 1e-3])
def test_dense_optimizer_oracles_match_apply_grads_cpu(opt, l2):
    """two steps of DenseLayer.apply_grads on the CPU against the oracle
    fed the state before each step. Adagrad sits inside the oracle's
    bound; the CPU Adam forms its constants in float64, so it is held to
    the bound plus that known relative difference (1e-4 covers it; a
    misplaced eps or a missing correction is percents)."""
    la = DenseLayer(17, 16, act="none", optimizer=opt, lr=1e-2, l2=l2)
    for step in (1, 2):
        W0, grad = ko.dense_inputs((16, 17), 1.0, seed=step)
        if step == 1:
            la.W.copy_(W0)
        la._dW, la._db = grad, torch.zeros(16)
        before = la.W.clone()
        if opt == "adam":
            m0, v0 = la.m.clone(), la.v.clone()
            ref = ko.adam_ref(before, grad, m0, v0, 1e-2, la.beta1, la.beta2,
                              la.eps, step, l2)
            la.apply_grads()
            # the CPU branch holds the betas as Python doubles, so its
            # (1 - beta2) is fp32(0.001) where the kernel's is
            # 1 - fp32(0.999): 4.7e-5 apart, as are the bias corrections
            inside("m", la.m, ref["m"][0],
                   ref["m"][1] + 1e-4 * ref["m"][0].abs())
            inside("v", la.v, ref["v"][0],
                   ref["v"][1] + 1e-4 * ref["v"][0].abs())
            slack = 1e-4 * (ref["W"][0] - before.double()).abs()
            inside("W", la.W, ref["W"][0], ref["W"][1] + slack)
        else:
            n0 = la.n.clone()
            ref = ko.adagrad_ref(before, grad, n0, 1e-2, la.eps, l2)
            la.apply_grads()
            inside("n", la.n, *ref["n"])
            inside("W", la.W, *ref["W"])


def test_adam_bias_correction_is_formed_in_fp32():
    bc1, bc2 = ko.adam_bias_corrections(0.9, 0.999, 1)
    assert bc2 != 1 - 0.999
    assert abs(bc2 / (1 - 0.999) - 1) > 1e-5  # the fp32 rounding of 0.999
    assert abs(bc1 / (1 - 0.9) - 1) < 1e-6


@pytest.mark.parametrize("D", [4, 6])
def test_sparse_oracles_equal_fm_ref_in_float64(D):
    """kernel_oracles' elementwise Adagrad / FTRL are fm_ref's arithmetic:
    same float64 values to a few ulp of float64"""
    for rnd, v_adagrad in ((0, True), (1, False)):
        st = ko.sparse_inputs(D, seed=D + rnd, ftrl=True)
        st["nW"] += 0.3 * rnd
        st["nV"] += 0.3 * rnd
        live = st["uniq"][:ko.SPARSE_NLIVE]
        lv = live.long()
        ref = {k: st[k].double().clone()
               for k in ("W", "V", "zW", "nW", "zV", "nV", "gradW", "gradV")}
        hy = [ko.f32(ko.FTRL[k]) for k in ("alpha", "beta", "l1", "l2")]
        fm_ref.ftrl_apply_ref(live, ref["W"], ref["V"], ref["zW"], ref["nW"],
                              ref["zV"], ref["nV"], ref["gradW"],
                              ref["gradV"], *hy, v_adagrad=v_adagrad,
                              v_lr=ko.f32(0.05), v_eps=ko.f32(1e-8),
                              v_l2=ko.f32(1e-5))
        mine = ko.ftrl_ref(st["W"][lv], st["zW"][lv], st["nW"][lv],
                           st["gradW"][lv], **ko.FTRL)
        for k, n in (("w", "W"), ("z", "zW"), ("n", "nW")):
            assert torch.allclose(mine[k][0], ref[n][lv], rtol=1e-13, atol=0)
        if v_adagrad:
            mv = ko.adagrad_ref(st["V"][lv], st["gradV"][lv], st["nV"][lv],
                                0.05, 1e-8, 1e-5)
            assert torch.allclose(mv["W"][0], ref["V"][lv], rtol=1e-13)
            assert torch.allclose(mv["n"][0], ref["nV"][lv], rtol=1e-13)
        else:
            mv = ko.ftrl_ref(st["V"][lv], st["zV"][lv], st["nV"][lv],
                             st["gradV"][lv], **ko.FTRL)
            assert torch.allclose(mv["w"][0], ref["V"][lv], rtol=1e-13)
            assert torch.allclose(mv["z"][0], ref["zV"][lv], rtol=1e-13)
        # fm_ref run in fp32 stays within the float64 oracle's bound
        st32 = {k: st[k].clone() for k in ref}
        fm_ref.ftrl_apply_ref(live, st32["W"], st32["V"], st32["zW"],
                              st32["nW"], st32["zV"], st32["nV"],
                              st32["gradW"], st32["gradV"], *hy,
                              v_adagrad=v_adagrad, v_lr=ko.f32(0.05),
                              v_eps=ko.f32(1e-8), v_l2=ko.f32(1e-5))
        inside("ftrl W fp32", st32["W"][lv], *mine["w"])
        inside("ftrl zW fp32", st32["zW"][lv], *mine["z"])
        if v_adagrad:
            inside("adagrad V fp32", st32["V"][lv], *mv["W"])
        else:
            inside("ftrl V fp32", st32["V"][lv], *mv["w"])


# ---------------------------------------------------------------------------
# mutation sensitivity on the GPU tests' inputs
# ---------------------------------------------------------------------------
def _longest(lengths):
    return lengths.index(max(lengths))


def test_mutant_wide_forward_drops_last_entry():
    for lengths, seed in ko.length_cases(4, wide=True):
        d = ko.embed_inputs(4, lengths, seed)
        ref, bound = ko.wide_forward_ref(d["row_ptr"], d["fids"], d["vals"],
                                         d["W"])
        rows = [r for r, n in enumerate(lengths) if n > 0]
        hit = 0
        for r in rows:
            mut, _ = ko.wide_forward_ref(
                *ko.drop_last_entry(d["row_ptr"], d["fids"], d["vals"], r),
                d["W"])
            hit += ko.differs(mut, ref, bound)
        assert hit >= 1 and hit >= len(rows) - 1, (hit, len(rows))


@pytest.mark.parametrize("K", ko.EMBED_KS)
@pytest.mark.parametrize("nf", [1, 5, 39])
def test_mutants_embed_gather(K, nf):
    """bit-exact outputs: any difference counts. 'pos+1' reads the next
    entry; 'nopad' leaves short rows' padding unwritten; dropping a row's
    last entry shows wherever that entry lies below nf."""
    seen_pad = 0
    for lengths, seed in ko.length_cases(K):
        d = ko.embed_inputs(K, lengths, seed)
        a = (d["row_ptr"], d["fids"], d["vals"], d["E"], nf)
        ref = ko.embed_gather_expect(*a)
        if sum(lengths) > 1:
            assert ko.differs(ko.embed_gather_expect(*a, mutant="pos+1"), ref)
        if any(n < nf for n in lengths):
            seen_pad += 1
            assert ko.differs(ko.embed_gather_expect(*a, mutant="nopad"), ref)
        r = _longest(lengths)
        if 0 < lengths[r] <= nf:
            cut = ko.drop_last_entry(d["row_ptr"], d["fids"], d["vals"], r)
            assert ko.differs(ko.embed_gather_expect(*cut, d["E"], nf), ref)
    assert seen_pad or nf == 1


@pytest.mark.parametrize("K", ko.EMBED_KS)
@pytest.mark.parametrize("nf", [1, 5, 39])
def test_mutant_embed_backward_emit_reads_next_position(K, nf):
    for lengths, seed in ko.length_cases(K):
        d = ko.embed_inputs(K, lengths, seed, nf=nf)
        a = (d["row_ptr"], d["vals"], d["dOut"], d["dwide"], nf, K)
        _, gv = ko.embed_backward_emit_expect(*a)
        _, gv_m = ko.embed_backward_emit_expect(*a, mutant="pos+1")
        if sum(lengths) > 0:
            assert ko.differs(gv_m, gv)


@pytest.mark.parametrize("K", ko.EMBED_KS)
def test_mutants_nfm(K):
    """dropping the last entry of the longest row moves wide, sumVX and vec
    past their bounds; omitting the -v x self term moves gv past its."""
    for ls, seed, dup in ko.nfm_cases(K, base=1000):
        d = ko.embed_inputs(K, ls, seed, dup_row=dup)
        ref = ko.nfm_forward_ref(d["row_ptr"], d["fids"], d["vals"], d["W"],
                                 d["E"])
        r = _longest(ls)
        mut = ko.nfm_forward_ref(
            *ko.drop_last_entry(d["row_ptr"], d["fids"], d["vals"], r),
            d["W"], d["E"])
        for k in ("wide", "sumVX"):
            assert ko.differs(mut[k][0], ref[k][0], ref[k][1]), k
        if ls[r] >= 2:  # a one-entry row's vec is 0 with or without it
            assert ko.differs(mut["vec"][0], ref["vec"][0], ref["vec"][1])
    for ls, seed, dup in ko.nfm_cases(K, base=2000):
        d = ko.embed_inputs(K, ls, seed, dup_row=dup)
        fwd = ko.nfm_forward_ref(d["row_ptr"], d["fids"], d["vals"], d["W"],
                                 d["E"])
        a = (d["row_ptr"], d["fids"], d["vals"], d["E"],
             fwd["sumVX"][0].float(), d["dvec"], d["dwide"])
        _, gv, bound = ko.nfm_backward_emit_ref(*a)
        _, gv_m, _ = ko.nfm_backward_emit_ref(*a, mutant="noself")
        assert ko.differs(gv_m, gv, bound)


def test_mutant_relu_ge():
    for n in (1, 255, 256, 257, 1025):
        g = torch.Generator().manual_seed(40 + n + 1)
        dY = torch.randn(n, generator=g)
        Y = torch.randn(n, generator=g)
        Y[0] = 0.0
        dY[0] = 1.5
        ref, _ = ko.act_backward_ref(dY, Y, 1)
        assert ko.differs(ko.act_backward_ref(dY, Y, 1, mutant="ge")[0], ref)


def test_mutant_colsum_drops_last_row():
    for N in (2, 255, 256, 257, 624):
        for M in (1, 3, 4, 5, 127, 128, 129, 385, 1000):
            dZ = ko.unit_matrix(M, N, seed=M * 7 + N)
            ref, bound = ko.colsum_ref(dZ)
            mut, _ = ko.colsum_ref(dZ, mutant="droprow")
            assert bool(((mut - ref).abs() > bound).all()), (M, N)
    for M in (1, 63, 64, 65, 131072, 131073):
        dZ = ko.unit_matrix(M, 1, seed=M,
                            last_row_scale=ko.colsum_flat_scale(M))
        ref, bound = ko.colsum_ref(dZ)
        mut, _ = ko.colsum_ref(dZ, mutant="droprow")
        assert ko.differs(mut, ref, bound), M


@pytest.mark.parametrize("shape", ko.DENSE_SHAPES + [(17,)], ids=str)
def test_mutants_dense_adam(shape):
    """eps moved inside the square root and the omitted bias correction
    show at both gradient scales; the omitted l2 wherever l2 != 0."""
    seed = 31 * sum(shape) + len(shape)
    for scale in (1.0, 1e-6):
        W, grad = ko.dense_inputs(shape, scale, seed=seed)
        z = torch.zeros_like(W)
        for step in (1, 2, 1000):
            ref = ko.adam_ref(W, grad, z, z, step=step, l2=1e-3, **ko.ADAM)
            muts = ["nol2", "nobc"] + (["eps_in"] if scale < 1 else [])
            for mutant in muts:
                mut = ko.adam_ref(W, grad, z, z, step=step, l2=1e-3,
                                  mutant=mutant, **ko.ADAM)
                hit = any(ko.differs(mut[k][0], ref[k][0], ref[k][1])
                          for k in ("W", "m", "v"))
                assert hit, (mutant, scale, step)


@pytest.mark.parametrize("shape", ko.DENSE_SHAPES + [(17,)], ids=str)
def test_mutants_dense_adagrad(shape):
    seed = 31 * sum(shape) + len(shape) + 1
    for scale in (1.0, 1e-4):
        W, grad = ko.dense_inputs(shape, scale, seed=seed)
        z = torch.zeros_like(W)
        ref = ko.adagrad_ref(W, grad, z, l2=1e-3, **ko.ADAGRAD)
        muts = ["nol2"] + (["eps_out"] if scale < 1 else [])
        for mutant in muts:
            mut = ko.adagrad_ref(W, grad, z, l2=1e-3, mutant=mutant,
                                 **ko.ADAGRAD)
            hit = any(ko.differs(mut[k][0], ref[k][0], ref[k][1])
                      for k in ("W", "n"))
            assert hit, (mutant, scale)


def test_mutant_transposed_mirror_swapped_strides():
    """visible on every shape with more than one row and column; for
    [n,1], [1,n] and [1,1] the transpose is the same flat buffer"""
    for shape in ko.DENSE_SHAPES:
        W, _ = ko.dense_inputs(shape, 1.0, seed=1)
        good = ko.transposed_mirror(W)
        bad = ko.transposed_mirror(W, mutant="swapped")
        assert ko.differs(good.float(), bad.float()) == (min(shape) > 1)
    assert sum(min(s) > 1 and s[0] != s[1] for s in ko.DENSE_SHAPES) >= 3


def test_mutant_gemm_drops_last_k():
    """on the fast-path tests' own operands, losing the last k exceeds the
    bound in every output element (pre-activation), and after the sigmoid
    and relu epilogues in at least one"""
    for M in (1, 3, 4, 5, 257):
        for K in (1, 63, 64, 65, 130):
            for act in (0, 1, 2):
                X = ko.bf16_values((M, K), seed=M * 131 + K)
                w = ko.bf16_values((1, K), seed=K, signed=act != 0,
                                   scale=1.0 if act == 0 else 2.0 / K)
                bias = torch.tensor([0.375])
                s, sb = ko.gemm_sum_ref(X, w)
                sm, _ = ko.gemm_sum_ref(X, w, mutant="dropk")
                ref, bound = ko.gemm_epilogue_ref(s, sb, bias, act)
                mut, _ = ko.gemm_epilogue_ref(sm, sb, bias, act)
                assert ko.differs(mut, ref, bound), (M, K, act)
    for N in (2, 255, 256, 257):
        for K in (1, 3, 4, 5, 127, 128, 129, 1000):
            dZ = ko.bf16_values((K, 1), seed=K * 3 + N)
            X = ko.bf16_values((K, N), seed=K * 5 + N)
            ref, bound = ko.gemm_sum_ref(dZ.t(), X.t())
            mut, _ = ko.gemm_sum_ref(dZ.t(), X.t(), mutant="dropk")
            assert bool(((mut - ref).abs() > bound).all()), (N, K)
    for M, N, K in ((63, 65, 8192), (64, 15, 8193), (3, 5, 16384),
                    (2, 2048, 8192)):
        dZ = ko.unit_matrix(K, M, seed=K + M, last_row_scale=16.0)
        X = ko.unit_matrix(K, N, seed=K + N + 1, last_row_scale=16.0)
        dZ, X = dZ.to(BF).float(), X.to(BF).float()
        ref, bound = ko.gemm_sum_ref(dZ.t(), X.t())
        mut, _ = ko.gemm_sum_ref(dZ.t(), X.t(), mutant="dropk")
        assert bool(((mut - ref).abs() > bound).all()), (M, N, K)


@pytest.mark.parametrize("D", [4, 6])
def test_mutant_ftrl_strict_inequality(D):
    """at |z'| == l1 both branches are numerically 0; '<' computes
    -(l1 - l1)/den = -0.0 where '<=' stores +0.0, which is why the GPU
    test compares the dead zone bit for bit"""
    st = ko.sparse_inputs(D, seed=D + 7, ftrl=True)
    lv = st["uniq"][:ko.SPARSE_NLIVE].long()
    a = (st["W"][lv], st["zW"][lv], st["nW"][lv], st["gradW"][lv])
    good = ko.ftrl_ref(*a, **ko.FTRL)["w"][0].float()
    bad = ko.ftrl_ref(*a, mutant="lt", **ko.FTRL)["w"][0].float()
    assert torch.equal(good, bad)  # numerically identical ...
    gb, bb = good.view(torch.int32), bad.view(torch.int32)
    assert (gb[:4] == 0).all()
    assert (bb[:2] != 0).all() and (bb[2:4] == 0).all()  # ... not bitwise
    # the rows just outside move by far more than the bound
    ref = ko.ftrl_ref(*a, **ko.FTRL)["w"]
    assert (ref[0][4:6].abs() > 100 * ref[1][4:6]).all()


@pytest.mark.parametrize("D", [4, 6])
def test_mutants_sparse_adagrad(D):
    st = ko.sparse_inputs(D, seed=D)
    lv = st["uniq"][:ko.SPARSE_NLIVE].long()
    a = (st["V"][lv], st["gradV"][lv], st["nV"][lv], 0.05, 1e-8)
    ref = ko.adagrad_ref(*a, 1e-5)
    mut = ko.adagrad_ref(*a, 1e-5, mutant="nol2")
    # from n = 0 the first update is lr * sign(g) whatever l2 adds to g;
    # the accumulator n' = g^2 is what shows it
    assert ko.differs(mut["n"][0], ref["n"][0], ref["n"][1])
