"""CPU checks of ``embed_bag_oracles``: the oracles agree with the definition
written as a plain loop on every exact case, the exactness conditions hold,
and every wrong reference of docs/TESTING.md differs on those same cases, so
a kernel that passes ``test_embed_bag_kernels_gpu.py`` is none of them:

* the position layout;
* sum instead of mean;
* mean by the sum of x;
* out-of-range fields clamped instead of skipped;
* an empty slot left unwritten.
"""

import pytest
import torch

import embed_bag_oracles as bo
import kernel_oracles as ko


def _args(c):
    return (c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"], c["nf"])


@pytest.mark.parametrize("nf", bo.NFS)
@pytest.mark.parametrize("K", bo.KS)
def test_oracle_is_the_loop(K, nf):
    for c in bo.exact_cases(K, nf) + bo.position_cases(K, nf):
        bo.assert_exact(c)
        for pooling in bo.POOLINGS:
            val, _, _ = bo.concat_ref(*_args(c), pooling)
            assert torch.equal(val, bo.concat_loop(*_args(c), pooling))


@pytest.mark.parametrize("nf", bo.NFS)
@pytest.mark.parametrize("K", bo.KS)
def test_emit_oracles_are_the_loop(K, nf):
    """both emit oracles against the definition written as a plain loop, on
    every exact case and both poolings; and the argument the GPU test leans
    on for fused == composed under mean as well: fl(D inv) x and
    d (s - e x) x are exact there, and their fp32 sum is the fused gv"""
    for c in bo.exact_cases(K, nf) + bo.position_cases(K, nf):
        sv = bo.case_sumvx32(c)
        for pooling in bo.POOLINGS:
            gw, gv_e, gv_d = bo.emit_loops(
                c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"], sv,
                c["dDeep"], c["dpred"], nf, pooling)
            w, e, _ = bo.embed_bag_emit_ref(
                c["row_ptr"], c["fields"], c["vals"], c["dDeep"], c["dwide"],
                nf, K, pooling)
            assert torch.equal(w, gw) and torch.equal(e, gv_e)
            w, d, _ = bo.deepfm_bag_emit_ref(
                c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"], sv,
                c["dDeep"], c["dpred"], nf, pooling)
            assert torch.equal(w, gw) and torch.equal(d, gv_d)
            # composed: the FM emit (exact) + the bag emit (exact), one add
            row, _, _ = ko.rows_pos(c["row_ptr"])
            x = c["vals"].double().unsqueeze(1)
            fm = c["dpred"].double()[row].unsqueeze(1) * (
                sv.double()[row] - c["E"].double()[c["fids"].long()] * x) * x
            assert torch.equal(fm.float().double(), fm)
            assert torch.equal(e.float().double(), e)
            assert torch.equal((fm + e).float().double(), d)


def test_mean_counts_beyond_powers_of_two():
    """the exact cases hold slots of 3, 5 and 7 entries, whose reciprocal
    rounds, and the expected value is fp32(S) * fp32(1/cnt) rounded once to
    fp32 and then to bf16"""
    c = bo.exact_cases(16, 5)[4]
    _, _, cnt = bo.concat_ref(*_args(c), 1)
    assert {3, 5, 7} <= set(cnt.tolist())
    inv = bo.inv32(cnt, 1)
    assert float(inv[cnt == 3][0]) == float(torch.tensor(1.0) / 3)
    S, _, _ = bo.bag_sums64(*_args(c))
    want = (S.float() * inv.unsqueeze(1)).to(torch.bfloat16)
    got = bo.concat_expect(*_args(c), 1)
    ko.check_bits("mean", got, (want.float() + 0.0).to(torch.bfloat16)
                  .view(got.shape))


MUTANTS = ("position", "sum", "mean_x", "clamp", "nopad")


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("nf", bo.NFS)
@pytest.mark.parametrize("K", bo.KS)
def test_wrong_references_differ(K, nf, mutant):
    """each wrong concat differs from the oracle on the exact set, in the
    bf16 values the GPU test compares"""
    pooling = 1 if mutant in ("sum", "mean_x") else 0
    hit = 0
    for c in bo.exact_cases(K, nf):
        good = bo.concat_expect(*_args(c), pooling)
        bad = bo.concat_expect(*_args(c), pooling, mutant=mutant)
        hit += ko.differs(good.float(), bad.float())
    assert hit >= 1, mutant


@pytest.mark.parametrize("mutant", ("position", "sum", "clamp"))
@pytest.mark.parametrize("K", (4, 16, 64))
def test_wrong_emits_differ(K, mutant):
    pooling = 1 if mutant == "sum" else 0
    hit = 0
    for c in bo.exact_cases(K, 5):
        sv = bo.case_sumvx32(c)
        a = (c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"], sv,
             c["dDeep"], c["dpred"], 5, pooling)
        hit += ko.differs(bo.deepfm_bag_emit_ref(*a)[1],
                          bo.deepfm_bag_emit_ref(*a, mutant=mutant)[1])
        b = (c["row_ptr"], c["fields"], c["vals"], c["dDeep"], c["dwide"],
             5, K, pooling)
        hit += ko.differs(bo.embed_bag_emit_ref(*b)[1],
                          bo.embed_bag_emit_ref(*b, mutant=mutant)[1])
    assert hit >= 2, mutant


@pytest.mark.parametrize("K", (4, 16, 64))
def test_position_cases_are_the_position_layout(K):
    """on the equivalence inputs the field oracle with sum pooling is the
    position oracle of kernel_oracles / deepfm_oracles, and no product is
    zero"""
    import deepfm_oracles as do

    for nf in bo.NFS:
        for c in bo.position_cases(K, nf):
            want = do.concat_expect(c["row_ptr"], c["fids"], c["vals"],
                                    c["E"], nf)
            ko.check_bits("concat", bo.concat_expect(*_args(c), 0), want)
            assert bool((c["E"][c["fids"].long()] != 0).all())
            sv = bo.case_sumvx32(c)
            _, gv, _ = bo.deepfm_bag_emit_ref(
                c["row_ptr"], c["fields"], c["fids"], c["vals"], c["E"], sv,
                c["dDeep"], c["dpred"], nf, 0)
            _, gv0, _ = do.deepfm_emit_ref(
                c["row_ptr"], c["fids"], c["vals"], c["E"], sv, c["dDeep"],
                c["dpred"], nf)
            assert torch.equal(gv, gv0)


def test_emit_is_the_autograd_gradient():
    """gv of the embed emit is d(sum concat * dOut)/dE per entry, in
    float64, for both pooling modes"""
    c = bo.float_case(8)
    nf, K = c["nf"], 8
    for pooling in bo.POOLINGS:
        row, inn, flat, cnt = bo.slots(c["row_ptr"], c["fields"], nf)
        inv = bo.inv32(cnt, pooling).double()
        P = (c["E"].double()[c["fids"].long()]
             * c["vals"].double().unsqueeze(1)).requires_grad_(True)
        S = torch.zeros(c["B"] * nf, K, dtype=torch.float64).index_add(
            0, flat[inn], P[inn])
        loss = (S * inv.unsqueeze(1)
                * c["dDeep"].double().view(c["B"] * nf, K)).sum()
        (gP,) = torch.autograd.grad(loss, P)
        _, gv, bound = bo.embed_bag_emit_ref(
            c["row_ptr"], c["fields"], c["vals"], c["dDeep"], c["dwide"],
            nf, K, pooling)
        err = (gv - gP * c["vals"].double().unsqueeze(1)).abs()
        assert bool((err <= bound + 1e-300).all())


def test_lds_rule():
    assert bo.lds_bytes(39, 16) == 16 * 39 * 17
    for K in bo.KS:
        nf = bo.nf_past_lds(K)
        assert bo.lds_bytes(nf, K) > bo.LDS_LIMIT >= bo.lds_bytes(nf - 1, K)
