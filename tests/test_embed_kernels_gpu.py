"""Direct parity tests for the embedding-table kernels behind the
Wide&Deep and NFM steps (embed_kernels.hip): wide_forward, embed_gather,
embed_backward_emit, nfm_forward, nfm_backward_emit.

Inputs are ragged CSR batches whose row lengths sit on the kernels' loop
edges (G = 64/K entries per trip, four trips unrolled, 64-lane strides),
with non-binary values. Oracles and the tolerance rule live in
``kernel_oracles.py``; every bound is derived there, none is measured.
"""

import pytest
import torch

import kernel_oracles as ko
from lightctr_amd.models.wide_deep import WideDeepHyper, WideDeepModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def dev(d, *names):
    return [d[n].to(DEV) for n in names]


def poison(shape, dtype):
    ko.poison(shape, dtype, DEV)


# ---------------------------------------------------------------------------
# wide_forward
# ---------------------------------------------------------------------------
def test_wide_forward_matches_float64():
    """wide[row] = sum w x against float64 at the sum bound
    n 2^-23 sum|w x|; the bound is 0 for empty rows, so they must be
    exactly 0. Lengths include 63, 64, 65, 130 (64-lane stride)."""
    for lengths, seed in ko.length_cases(4, wide=True):
        d = ko.embed_inputs(4, lengths, seed)
        ref, bound = ko.wide_forward_ref(d["row_ptr"], d["fids"], d["vals"],
                                         d["W"])
        args = dev(d, "row_ptr", "fids", "vals", "W")
        poison((len(lengths),), torch.float32)
        out = ops().wide_forward(*args)
        ko.check_bound("wide_forward", out, ref, bound)
        empty = torch.tensor(lengths) == 0
        assert (out.cpu()[empty] == 0).all()


# ---------------------------------------------------------------------------
# embed_gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", ko.EMBED_KS)
@pytest.mark.parametrize("nf", [1, 5, 39])
def test_embed_gather_ragged_rows_bit_exact_and_zero_padded(K, nf):
    """out = bf16(E[f,k] * x) is one fp32 multiply and one RNE conversion:
    bit-exact. Rows shorter than nf must read exactly +0 in the rest of
    their slice (the CPU gather zero-pads), rows longer than nf lose the
    surplus. The output block is NaN-poisoned first, so padding the kernel
    does not write shows up as NaN instead of depending on what the
    allocator held."""
    for lengths, seed in ko.length_cases(K):
        d = ko.embed_inputs(K, lengths, seed)
        expect = ko.embed_gather_expect(d["row_ptr"], d["fids"], d["vals"],
                                        d["E"], nf)
        args = dev(d, "row_ptr", "fids", "vals", "E")
        poison((len(lengths), nf * K), torch.bfloat16)
        out = ops().embed_gather(*args, nf).cpu()
        assert out.shape == (len(lengths), nf * K)
        assert out.dtype == torch.bfloat16
        # padding first: the clearest message for the likeliest failure
        _, _, counts = ko.rows_pos(d["row_ptr"])
        pad = (torch.arange(nf).unsqueeze(0) >= counts.unsqueeze(1))
        pad = pad.unsqueeze(2).expand(-1, -1, K).reshape(len(lengths), -1)
        got = out.view(torch.int16)[pad]
        assert (got == 0).all(), (
            f"{int((got != 0).sum())} of {got.numel()} padding slots are "
            f"not +0 (lengths {lengths}, nf {nf})")
        ko.check_bits("embed_gather", out, expect)


# ---------------------------------------------------------------------------
# embed_backward_emit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", ko.EMBED_KS)
@pytest.mark.parametrize("nf", [1, 5, 39])
def test_embed_backward_emit_bit_exact(K, nf):
    """gv = d * x and gw = dw * x are single fp32 multiplies: bit-exact.
    Entries at pos >= nf get gv == 0 while their gw is still dw * x."""
    for lengths, seed in ko.length_cases(K):
        d = ko.embed_inputs(K, lengths, seed, nf=nf)
        gw_e, gv_e = ko.embed_backward_emit_expect(
            d["row_ptr"], d["vals"], d["dOut"], d["dwide"], nf, K)
        nnz = d["vals"].numel()
        args = dev(d, "row_ptr", "vals", "dOut", "dwide")
        poison((nnz, K), torch.float32)
        gw, gv = ops().embed_backward_emit(*args, nf, K)
        ko.check_bits("embed_backward_emit.gv", gv, gv_e)
        ko.check_bits("embed_backward_emit.gw", gw, gw_e)
        _, pos, _ = ko.rows_pos(d["row_ptr"])
        over = pos >= nf
        if over.any():
            assert (gv.cpu()[over] == 0).all()
            assert (gw.cpu()[over] != 0).all()


# ---------------------------------------------------------------------------
# nfm_forward / nfm_backward_emit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", ko.EMBED_KS)
def test_nfm_forward_per_element(K):
    """wide, sumVX, vec per element against float64 (bounds derived in
    nfm_forward_ref), vec_bf the exact bf16 of the vec the same call
    returned. One row repeats a fid; a one-entry row has s^2 == q, so its
    vec is 0 within the bound."""
    for ls, seed, dup_row in ko.nfm_cases(K, base=1000):
        d = ko.embed_inputs(K, ls, seed, dup_row=dup_row)
        ref = ko.nfm_forward_ref(d["row_ptr"], d["fids"], d["vals"], d["W"],
                                 d["E"])
        wide, sumVX, vec, vec_bf = ops().nfm_forward(
            *dev(d, "row_ptr", "fids", "vals", "W", "E"))
        ko.check_bound("nfm_forward.wide", wide, *ref["wide"])
        ko.check_bound("nfm_forward.sumVX", sumVX, *ref["sumVX"])
        ko.check_bound("nfm_forward.vec", vec, *ref["vec"])
        ko.check_bits("nfm_forward.vec_bf", vec_bf,
                      vec.cpu().to(torch.bfloat16))
        # a one-entry row has the float64 vec exactly 0, so the bound
        # check above already held |vec| to the bound there
        one = [i for i, n in enumerate(ls) if n == 1]
        assert one or dup_row is None, "the length set holds such a row"
        assert (ref["vec"][0][one] == 0).all()


@pytest.mark.parametrize("K", ko.EMBED_KS)
def test_nfm_backward_emit_per_entry(K):
    """gv[j,k] = dvec (sumVX - v x) x at the four-rounding bound, gw the
    exact product. sumVX comes from the float64 oracle rounded to fp32, so
    only this kernel is under test."""
    for ls, seed, dup_row in ko.nfm_cases(K, base=2000):
        d = ko.embed_inputs(K, ls, seed, dup_row=dup_row)
        fwd = ko.nfm_forward_ref(d["row_ptr"], d["fids"], d["vals"], d["W"],
                                 d["E"])
        d["sumVX"] = fwd["sumVX"][0].float()
        gw_e, gv_ref, bound = ko.nfm_backward_emit_ref(
            d["row_ptr"], d["fids"], d["vals"], d["E"], d["sumVX"],
            d["dvec"], d["dwide"])
        args = dev(d, "row_ptr", "fids", "vals", "E", "sumVX", "dvec",
                   "dwide")
        poison((d["vals"].numel(), K), torch.float32)
        gw, gv = ops().nfm_backward_emit(*args)
        ko.check_bound("nfm_backward_emit.gv", gv, gv_ref, bound)
        ko.check_bits("nfm_backward_emit.gw", gw, gw_e)


# ---------------------------------------------------------------------------
# model level: a ragged libffm-style batch through Wide&Deep
# ---------------------------------------------------------------------------
def test_widedeep_ragged_batch_gpu_matches_cpu():
    """Rows of 0..45 entries at nf = 39 (shorter, equal, longer): the GPU
    score must be finite and match the CPU model on copied weights at the
    atol=0.08, rtol=0.05 that test_mlp_gpu_matches_cpu uses for the bf16
    MLP forward, applied to the pre-sigmoid score."""
    F = ko.F_TABLE
    h = WideDeepHyper(num_features=F, num_fields=39, k=16, hidden=(64, 32),
                      init_sigma=0.1)
    cpu = WideDeepModel(h, device="cpu")
    gpu = WideDeepModel(h, device=DEV)
    g = torch.Generator().manual_seed(5)
    cpu.W.copy_(torch.randn(F, generator=g) * 0.1)
    gpu.W.copy_(cpu.W)
    gpu.E.copy_(cpu.E)
    for lc, lg in zip(cpu.mlp.layers, gpu.mlp.layers):
        lg.W.copy_(lc.W)
        lg.b.copy_(lc.b)
        lg.Wbf.copy_(lg.W.to(torch.bfloat16))
        lg.Wtbf.copy_(lg.W.t().contiguous().to(torch.bfloat16))
    row_ptr, fids, vals = ko.make_csr(list(range(46)), seed=6)
    s_cpu, _ = cpu._forward_cpu(row_ptr, fids, vals, train=False)
    poison((46, 39 * 16), torch.bfloat16)
    s_gpu, _ = gpu._forward_gpu(row_ptr.to(DEV), fids.to(DEV), vals.to(DEV),
                                train=False)
    s_gpu = s_gpu.cpu()
    assert torch.isfinite(s_gpu).all(), s_gpu
    assert torch.allclose(s_gpu, s_cpu, atol=0.08, rtol=0.05), \
        (s_gpu - s_cpu).abs().max()
    poison((46, 39 * 16), torch.bfloat16)
    p = gpu.predict_proba(row_ptr.to(DEV), fids.to(DEV), vals.to(DEV)).cpu()
    assert torch.isfinite(p).all()
    assert ((p > 0) & (p < 1)).all()


# ---------------------------------------------------------------------------
# argument checks: an unsupported K raises instead of aborting the process.
# Each binding checks K before it allocates or launches anything.
# ---------------------------------------------------------------------------
def _k5_inputs():
    d = ko.embed_inputs(4, [3, 0, 2], 77, nf=2)
    g = torch.Generator().manual_seed(78)
    d["E5"] = torch.randn(ko.F_TABLE, 5, generator=g)
    d["dOut5"] = torch.randn(3, 2 * 5, generator=g)
    d["sumVX5"] = torch.randn(3, 5, generator=g)
    d["dvec5"] = torch.randn(3, 5, generator=g)
    return d


def test_embed_gather_rejects_k5():
    d = _k5_inputs()
    with pytest.raises(RuntimeError, match="K must be one of"):
        ops().embed_gather(*dev(d, "row_ptr", "fids", "vals", "E5"), 2)


def test_embed_backward_emit_rejects_k5():
    d = _k5_inputs()
    with pytest.raises(RuntimeError, match="K must be one of"):
        ops().embed_backward_emit(
            *dev(d, "row_ptr", "vals", "dOut5", "dwide"), 2, 5)


def test_nfm_forward_rejects_k5():
    d = _k5_inputs()
    with pytest.raises(RuntimeError, match="K must be one of"):
        ops().nfm_forward(*dev(d, "row_ptr", "fids", "vals", "W", "E5"))


def test_nfm_backward_emit_rejects_k5():
    d = _k5_inputs()
    with pytest.raises(RuntimeError, match="K must be one of"):
        ops().nfm_backward_emit(
            *dev(d, "row_ptr", "fids", "vals", "E5", "sumVX5", "dvec5",
                 "dwide"))
