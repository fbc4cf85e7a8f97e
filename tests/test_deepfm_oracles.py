"""CPU checks of ``deepfm_oracles``: the oracles equal the model's fp32 CPU
path (exactly on the exact set, inside the bounds on the float set), the
exactness assertion rejects an oversized case, the analytic per-entry
gradients add up to float64 autograd's, and every wrong reference listed in
docs/TESTING.md differs on the exact inputs of ``test_deepfm_kernels_gpu.py``
and leaves the bound on its float inputs.
"""

import pytest
import torch

import deepfm_oracles as do
import kernel_oracles as ko
from lightctr_amd.models.deepfm import DeepFMHyper, DeepFMModel


def cpu_model(c):
    m = DeepFMModel(DeepFMHyper(num_features=c["F"], num_fields=c["nf"],
                                k=c["K"], hidden=(8,)), device="cpu")
    m.W.copy_(c["W"])
    m.E.copy_(c["E"])
    return m


def fwd_ref(c, mutant=None):
    return do.deepfm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"],
                                 c["E"], c["nf"], mutant=mutant)


def emit_ref(c, sv32, mutant=None):
    return do.deepfm_emit_ref(c["row_ptr"], c["fids"], c["vals"], c["E"],
                              sv32, c["dDeep"], c["dpred"], c["nf"],
                              mutant=mutant)


@pytest.mark.parametrize("K", do.KS)
def test_oracles_equal_cpu_path_exact(K):
    for i, c in enumerate(do.exact_cases(K)):
        do.assert_exact(c)
        m = cpu_model(c)
        ref = fwd_ref(c)
        fm, sumVX, deep = m._fm_gather_cpu(c["row_ptr"], c["fids"],
                                           c["vals"])
        name = f"K{K}.nf{c['nf']}.case{i}"
        assert torch.equal(fm.double(), ref["fm"][0]), name
        assert torch.equal(sumVX.double(), ref["sumVX"][0]), name
        ko.check_bits(name + ".concat", deep.to(torch.bfloat16),
                      ref["concat"])
        sv32 = ref["sumVX"][0].float()
        gw64, gv64, _ = emit_ref(c, sv32)
        gw, gv = m._emit_cpu(c["row_ptr"], c["fids"], c["vals"], sv32,
                             c["dDeep"], c["dpred"])
        assert torch.equal(gw.double(), gw64), name
        assert torch.equal(gv.double(), gv64), name


@pytest.mark.parametrize("K", do.KS)
def test_oracles_equal_cpu_path_float(K):
    c = do.float_case(K)
    m = cpu_model(c)
    ref = fwd_ref(c)
    fm, sumVX, deep = m._fm_gather_cpu(c["row_ptr"], c["fids"], c["vals"])
    ko.check_bound(f"K{K}.sumVX", sumVX, *ref["sumVX"])
    ko.check_bound(f"K{K}.fm", fm, *ref["fm"])
    ko.check_bits(f"K{K}.concat", deep.to(torch.bfloat16), ref["concat"])
    sv32 = ref["sumVX"][0].float()
    gw64, gv64, bound = emit_ref(c, sv32)
    gw, gv = m._emit_cpu(c["row_ptr"], c["fids"], c["vals"], sv32,
                         c["dDeep"], c["dpred"])
    row, _, _ = ko.rows_pos(c["row_ptr"])
    ko.check_bits(f"K{K}.gw", gw, c["dpred"][row] * c["vals"])
    ko.check_bound(f"K{K}.gv", gv, gv64, bound)


def test_assert_exact_rejects_oversized():
    """a thousand entries of E = 2, x = 2 at K = 64: s_k = 4000 and
    sum_k s_k^2 = 2^30"""
    c = do.case(64, [1000], 3, 5)
    c["E"][:-1] = 2.0
    c["vals"][:] = 2.0
    with pytest.raises(AssertionError):
        do.assert_exact(c)
    # and a gradient past 2^24 units
    c = do.case(4, [3], 4, 5, s=3)
    c["dDeep"][:] = 2.0 ** 22
    with pytest.raises(AssertionError):
        do.assert_exact(c)


@pytest.mark.parametrize("K,nf", [(4, 5), (16, 39), (64, 1)])
def test_emit_totals_equal_autograd(K, nf):
    """per-fid totals of the analytic (gw, gv) against float64 autograd of
    the float64 forward composed with a small float64 MLP and the logistic
    loss, 1e-10 relative"""
    c = do.case(K, [0, 3, 45, 1, 0, 39, 7], 500 + K, nf, exact=False)
    F, B = c["F"], c["B"]
    g = torch.Generator().manual_seed(9)
    W = c["W"].double()
    E = c["E"].double()
    W[F - 1] = 0.0
    E[F - 1] = 0.0
    W.requires_grad_(True)
    E.requires_grad_(True)
    W1 = torch.randn(nf * K, 6, generator=g, dtype=torch.float64)
    b1 = torch.randn(6, generator=g, dtype=torch.float64)
    W2 = torch.randn(6, generator=g, dtype=torch.float64)
    y = torch.randint(0, 2, (B,), generator=g).double()
    wide, s, q, deep = do.forward64(c["row_ptr"], c["fids"], c["vals"], W, E,
                                    nf)
    fm = wide + 0.5 * (s * s - q).sum(1)
    score = fm + torch.tanh(deep @ W1 + b1) @ W2
    loss = torch.nn.functional.binary_cross_entropy_with_logits(
        score, y, reduction="sum") / B
    d, D = torch.autograd.grad(loss, (score, deep), retain_graph=True)
    gW, gE = torch.autograd.grad(loss, (W, E))
    gw, gv, _ = do.deepfm_emit_ref(c["row_ptr"], c["fids"], c["vals"],
                                   E.detach(), s.detach(), D, d, nf)
    f = c["fids"].long()
    totW = torch.zeros(F, dtype=torch.float64).index_add_(0, f, gw)
    totE = torch.zeros(F, K, dtype=torch.float64).index_add_(0, f, gv)
    assert float((totW - gW).abs().max()) <= 1e-10 * float(gW.abs().max())
    assert float((totE - gE).abs().max()) <= 1e-10 * float(gE.abs().max())


FWD_MUTANTS = ("droplast", "drop4G", "nohalf", "fm_nf", "nopad", "wide_all")
EMIT_MUTANTS = ("noself", "pos+1", "past_nf", "D_after")


def _fwd_differs(a, b, bounds=None):
    """any of fm, sumVX, concat differs (beyond its bound, if given; the
    concat is bit-exact either way)"""
    out = False
    for k in ("fm", "sumVX"):
        out |= ko.differs(a[k][0], b[k][0],
                          None if bounds is None else b[k][1])
    return out | ko.differs(a["concat"].float(), b["concat"].float())


@pytest.mark.parametrize("K", do.KS)
@pytest.mark.parametrize("mutant", FWD_MUTANTS)
def test_wrong_forward_references_are_caught(K, mutant):
    """last entry of a row dropped; entry at 4G dropped; the 1/2 omitted;
    entries past nf dropped from the FM term; padding not written; wide
    summed from every lane"""
    hit = any(_fwd_differs(fwd_ref(c, mutant), fwd_ref(c))
              for c in do.exact_cases(K))
    assert hit, "exact set"
    c = do.float_case(K)
    assert _fwd_differs(fwd_ref(c, mutant), fwd_ref(c), bounds=True), \
        "float set"


@pytest.mark.parametrize("K", do.KS)
@pytest.mark.parametrize("mutant", EMIT_MUTANTS)
def test_wrong_emit_references_are_caught(K, mutant):
    """-v x self term omitted; pos+1 read for pos in dDeep; entries past nf
    given a D; D added after the multiply by x"""
    hit = False
    for c in do.exact_cases(K):
        sv32 = do.case_sumvx32(c)
        hit |= ko.differs(emit_ref(c, sv32, mutant)[1], emit_ref(c, sv32)[1])
    assert hit, "exact set"
    c = do.float_case(K)
    sv32 = do.case_sumvx32(c)
    _, gv, bound = emit_ref(c, sv32)
    assert ko.differs(emit_ref(c, sv32, mutant)[1], gv, bound), "float set"
