"""Parity tests for the DeepFM kernels (deepfm_kernels.hip) against the
float64 oracles of ``deepfm_oracles.py``.

Main set: small-integer inputs on which every quantity is exact in fp32 in
any summation order (conditions stated and asserted in ``deepfm_oracles``),
so the comparisons are bit or value equality, against the oracle and against
the composed bindings the fused kernels replace (``fm_forward`` +
``embed_gather``, ``fm_backward_emit`` + ``embed_backward_emit``). A float
case per K keeps real rounding in view under derived bounds. Shapes follow
the loops: row lengths around G = 64/K and the four-trip unroll, 39, 130,
1000; nf = 1, 5, 39 (rows shorter than, equal to and longer than nf);
batches of 1, 3, 4, 5, 9 rows around the four rows of a block; empty rows
first, last, in the middle and adjacent; one fid twice in a row.
``test_deepfm_oracles.py`` shows on the CPU that the wrong references listed
in docs/TESTING.md differ on these same inputs.
"""

import pytest
import torch

import deepfm_oracles as do
import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def view_on_gpu(t, fill):
    """t as a view inside a longer device buffer filled with `fill`"""
    buf, o = do.padded(t, fill)
    return buf.to(DEV)[o:o + t.numel()]


def up(c):
    """Upload a case: fids / vals are views; the ints around fids name fid
    F-1 (NaN rows of W and E), the floats around vals are NaN"""
    return {"row_ptr": c["row_ptr"].to(DEV),
            "fids": view_on_gpu(c["fids"], c["F"] - 1),
            "vals": view_on_gpu(c["vals"], NAN),
            "W": c["W"].to(DEV), "E": c["E"].to(DEV),
            "dpred": c["dpred"].to(DEV), "dDeep": c["dDeep"].to(DEV)}


def run_forward(g, c):
    B, K, nf = c["B"], c["K"], c["nf"]
    ko.poison((B,), torch.float32, DEV)
    ko.poison((B, K), torch.float32, DEV)
    ko.poison((B, nf * K), torch.bfloat16, DEV)
    return ops().deepfm_forward(g["row_ptr"], g["fids"], g["vals"], g["W"],
                                g["E"], nf)


def run_emit(g, c, sumVX, dDeep=None, dpred=None):
    nnz, K = c["fids"].numel(), c["K"]
    ko.poison((nnz,), torch.float32, DEV)
    ko.poison((nnz, K), torch.float32, DEV)
    return ops().deepfm_backward_emit(
        g["row_ptr"], g["fids"], g["vals"], g["E"], sumVX,
        g["dDeep"] if dDeep is None else dDeep,
        g["dpred"] if dpred is None else dpred, c["nf"])


def fwd_ref(c):
    return do.deepfm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"],
                                 c["E"], c["nf"])


def emit_ref(c, sv32):
    return do.deepfm_emit_ref(c["row_ptr"], c["fids"], c["vals"], c["E"],
                              sv32, c["dDeep"], c["dpred"], c["nf"])


@pytest.mark.parametrize("K", do.KS)
def test_forward_exact(K):
    """fm, sumVX and the concat bit for bit against the oracle, and bit for
    bit against fm_forward / embed_gather on the same inputs"""
    for i, c in enumerate(do.exact_cases(K)):
        do.assert_exact(c)
        g = up(c)
        name = f"K{K}.nf{c['nf']}.case{i}"
        ref = fwd_ref(c)
        fm, sumVX, deep = run_forward(g, c)
        ko.check_bits(name + ".fm", fm, ref["fm"][0].float() + 0.0)
        ko.check_bits(name + ".sumVX", sumVX, ref["sumVX"][0].float() + 0.0)
        ko.check_bits(name + ".concat", deep, ref["concat"])
        # the composed bindings
        ko.poison((c["B"],), torch.float32, DEV)
        ko.poison((c["B"], K), torch.float32, DEV)
        pred2, sumVX2 = ops().fm_forward(g["row_ptr"], g["fids"], g["vals"],
                                         g["W"], g["E"])
        ko.poison((c["B"], c["nf"] * K), torch.bfloat16, DEV)
        deep2 = ops().embed_gather(g["row_ptr"], g["fids"], g["vals"],
                                   g["E"], c["nf"])
        ko.check_bits(name + ".fm vs fm_forward", fm, pred2.cpu())
        ko.check_bits(name + ".sumVX vs fm_forward", sumVX, sumVX2.cpu())
        ko.check_bits(name + ".concat vs embed_gather", deep, deep2.cpu())


@pytest.mark.parametrize("K", do.KS)
def test_emit_exact(K):
    """gw bit for bit, gv by value against the oracle; both bit for bit
    against fm_backward_emit + embed_backward_emit summed; gv at pos >= nf is
    the pure FM emit; with d = 0, gv is embed_backward_emit's output"""
    for i, c in enumerate(do.exact_cases(K)):
        g = up(c)
        name = f"K{K}.nf{c['nf']}.case{i}"
        nnz, nf = c["fids"].numel(), c["nf"]
        sv32 = do.case_sumvx32(c)
        sumVX = sv32.to(DEV)
        gw64, gv64, _ = emit_ref(c, sv32)
        gw, gv = run_emit(g, c, sumVX)
        ko.check_bits(name + ".gw", gw, gw64.float())
        do.check_value(name + ".gv", gv, gv64)

        ko.poison((nnz,), torch.float32, DEV)
        ko.poison((nnz, K), torch.float32, DEV)
        gw_fm, gv_fm = ops().fm_backward_emit(
            g["row_ptr"], g["fids"], g["vals"], g["E"], sumVX, g["dpred"],
            None)
        ko.poison((nnz,), torch.float32, DEV)
        ko.poison((nnz, K), torch.float32, DEV)
        _, gv_em = ops().embed_backward_emit(
            g["row_ptr"], g["vals"], g["dDeep"], g["dpred"], nf, K)
        ko.check_bits(name + ".gw vs fm_backward_emit", gw, gw_fm.cpu())
        ko.check_bits(name + ".gv vs composed", gv, (gv_fm + gv_em).cpu())
        _, pos, _ = ko.rows_pos(c["row_ptr"])
        past = pos >= nf
        assert torch.equal(gv.cpu()[past], gv_fm.cpu()[past]), name

        zero = torch.zeros_like(g["dpred"])
        gw0, gv0 = run_emit(g, c, sumVX, dpred=zero)
        assert torch.equal(gv0.cpu(), gv_em.cpu()), name
        assert torch.equal(gw0.cpu(), torch.zeros(nnz)), name


@pytest.mark.parametrize("K", do.KS)
def test_float_set(K):
    """sumVX, fm and gv inside their derived bounds; gw and the concat bit
    for bit"""
    c = do.float_case(K)
    g = up(c)
    ref = fwd_ref(c)
    fm, sumVX, deep = run_forward(g, c)
    ko.check_bound(f"K{K}.sumVX", sumVX, *ref["sumVX"])
    ko.check_bound(f"K{K}.fm", fm, *ref["fm"])
    ko.check_bits(f"K{K}.concat", deep, ref["concat"])
    sv32 = ref["sumVX"][0].float()
    gw64, gv64, bound = emit_ref(c, sv32)
    gw, gv = run_emit(g, c, sv32.to(DEV))
    row, _, _ = ko.rows_pos(c["row_ptr"])
    ko.check_bits(f"K{K}.gw", gw, c["dpred"][row] * c["vals"])
    ko.check_bound(f"K{K}.gv", gv, gv64, bound)


@pytest.mark.parametrize("K", do.KS)
def test_empty_batch(K):
    """B = 0 returns empty tensors and launches nothing; the checked launch
    that follows reports nothing"""
    c = do.case(K, [], 1, 5)
    g = up(c)
    fm, sumVX, deep = ops().deepfm_forward(g["row_ptr"], g["fids"],
                                           g["vals"], g["W"], g["E"], 5)
    assert fm.shape == (0,) and sumVX.shape == (0, K)
    assert deep.shape == (0, 5 * K) and deep.dtype == torch.bfloat16
    gw, gv = ops().deepfm_backward_emit(g["row_ptr"], g["fids"], g["vals"],
                                        g["E"], sumVX, g["dDeep"],
                                        g["dpred"], 5)
    assert gw.shape == (0,) and gv.shape == (0, K)
    c1 = do.case(K, [2], 2, 5)
    fm1, _, _ = run_forward(up(c1), c1)
    ko.check_bits("after empty", fm1, fwd_ref(c1)["fm"][0].float() + 0.0)


# ---------------------------------------------------------------------------
# argument checks: every bad argument raises before anything is launched,
# and a good call follows each
# ---------------------------------------------------------------------------
def _good(c, g, sumVX):
    fm, s, _ = run_forward(g, c)
    ko.check_bits("good.fm", fm, fwd_ref(c)["fm"][0].float() + 0.0)
    gw, _ = run_emit(g, c, sumVX)
    ko.check_bits("good.gw", gw, emit_ref(c, sumVX.cpu())[0].float())


def test_binding_checks():
    K, nf = 4, 2
    c = do.case(K, [3, 0, 2], 77, nf)
    g = up(c)
    sumVX = do.case_sumvx32(c).to(DEV)
    B, nnz, F = c["B"], c["fids"].numel(), c["F"]
    gen = torch.Generator().manual_seed(78)
    E5 = torch.randn(F, 5, generator=gen).to(DEV)

    def fwd(**kw):
        a = dict(row_ptr=g["row_ptr"], fids=g["fids"], vals=g["vals"],
                 W=g["W"], E=g["E"], nf=nf)
        a.update(kw)
        return ops().deepfm_forward(a["row_ptr"], a["fids"], a["vals"],
                                    a["W"], a["E"], a["nf"])

    def emit(**kw):
        a = dict(row_ptr=g["row_ptr"], fids=g["fids"], vals=g["vals"],
                 E=g["E"], sumVX=sumVX, dDeep=g["dDeep"], dpred=g["dpred"],
                 nf=nf)
        a.update(kw)
        return ops().deepfm_backward_emit(
            a["row_ptr"], a["fids"], a["vals"], a["E"], a["sumVX"],
            a["dDeep"], a["dpred"], a["nf"])

    with pytest.raises(RuntimeError, match="K must be one of"):
        fwd(E=E5)
    _good(c, g, sumVX)
    with pytest.raises(RuntimeError, match="K must be one of"):
        emit(E=E5, sumVX=torch.zeros(B, 5, device=DEV),
             dDeep=torch.zeros(B, nf * 5, device=DEV))
    _good(c, g, sumVX)

    bad_fwd = [
        dict(E=g["E"].flatten()),                          # not 2-D
        dict(E=g["E"].double()),                           # dtype
        dict(E=g["E"].cpu()),                              # device
        dict(E=g["E"].t().contiguous().t()),               # contiguity
        dict(W=g["W"][:-1]),                               # numel != F
        dict(W=g["W"].double()),
        dict(vals=g["vals"][:-1]),                         # lengths
        dict(fids=g["fids"].long()),
        dict(fids=g["fids"].cpu()),
        dict(vals=g["vals"].double()),
        dict(row_ptr=g["row_ptr"][:0]),                    # empty row_ptr
        dict(row_ptr=g["row_ptr"].long()),
        dict(nf=0),
    ]
    for kw in bad_fwd:
        with pytest.raises(RuntimeError):
            fwd(**kw)
        _good(c, g, sumVX)

    bad_emit = [
        dict(sumVX=sumVX.flatten()),                       # not [B, K]
        dict(sumVX=sumVX[:-1]),
        dict(sumVX=torch.zeros(B, 2 * K, device=DEV)),
        dict(sumVX=sumVX.double()),
        dict(sumVX=sumVX.cpu()),
        dict(dDeep=g["dDeep"].flatten()),                  # not [B, nf*K]
        dict(dDeep=g["dDeep"][:, :-1].contiguous()),
        dict(dDeep=g["dDeep"][:, :-1]),                    # contiguity
        dict(dDeep=g["dDeep"].double()),
        dict(dpred=g["dpred"][:-1]),                       # not [B]
        dict(dpred=g["dpred"].unsqueeze(1)),
        dict(dpred=g["dpred"].cpu()),
        dict(E=g["E"].flatten()),
        dict(vals=g["vals"][:-1]),
        dict(row_ptr=g["row_ptr"][:0]),
        dict(nf=0),
        dict(nf=nf + 1),                                   # dDeep mismatch
    ]
    for kw in bad_emit:
        with pytest.raises(RuntimeError):
            emit(**kw)
        _good(c, g, sumVX)
    assert nnz == 5
