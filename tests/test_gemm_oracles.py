"""CPU checks of ``gemm_oracles.py``: the reference is held to the
project's CPU path and to plain torch float64 matmul, and every wrong
reference differs on the inputs the GPU tests use (and leaves the bound on
the float set), so a kernel with that mistake cannot pass
``test_gemm_kernels_gpu.py``.
"""

import re
from pathlib import Path

import pytest
import torch

import gemm_oracles as go
import kernel_oracles as ko
from lightctr_amd.models.mlp import DenseLayer

CSRC = Path(__file__).resolve().parent.parent / "lightctr_amd/ops/csrc"
ACTS = ("none", "relu", "sigmoid")


def operands(kind, M, N, K, ta=0, tb=0, fill="random"):
    if kind == "exact":
        return go.exact_operands(M, N, K, ta, tb, fill=fill)
    return go.float_operands(M, N, K, ta, tb,
                             lastk_scale=go.lastk_scale_for(K))


# ---------------------------------------------------------------------------
# 1. the oracle against the CPU path and torch float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "float"])
def test_reference_matches_float64_matmul_all_layouts(kind):
    for ta, tb in go.LAYOUTS:
        for M, N, K in [(129, 65, 72), (17, 129, 200), (1, 1, 1)]:
            A, B, bias = operands(kind, M, N, K, ta, tb)
            a = A.double().t() if ta else A.double()
            b = B.double() if tb else B.double().t()
            z = a @ b + bias.double()
            for act in (0, 1, 2):
                ref, pre = go.gemm_ref(A, B, ta, tb, bias, act)
                want = go.act_ref(z, act)
                if kind == "exact":
                    assert torch.equal(pre, z)
                    assert torch.equal(ref, want)
                else:  # einsum and matmul may order the float64 sum apart
                    assert torch.allclose(ref, want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", ["exact", "float"])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_reference_matches_dense_layer_cpu(kind, act):
    """forward: y = act(x W^T + b), layout (0, 0); backward: dW = dZ^T x,
    layout (1, 1), and dx = dZ W, layout (0, 1) on W and (0, 0) on the
    W^T mirror. DenseLayer computes in fp32: exact on the exact set,
    inside the sum-rule bound on the float set."""
    B_, In, Out = 40, 72, 17
    x, W, b = operands(kind, B_, Out, In)
    layer = DenseLayer(In, Out, act=ACTS[act], device="cpu")
    layer.W, layer.b = W.clone(), b.clone()
    y, _ = layer.forward_cpu(x)
    ref, _ = go.gemm_ref(x, W, 0, 0, b, act)
    s, _ = go.gemm_ref(x, W, 0, 0)
    sb = (torch.zeros_like(s) if kind == "exact"
          else go.sum_bound(x, W, 0, 0))
    ref2, bound = go.epilogue_bound(s, sb, b, act)
    assert torch.equal(ref, ref2)
    if kind == "exact" and act != 2:
        assert torch.equal(y.double(), ref)
    else:
        ko.check_bound(f"forward_cpu-{kind}-{act}", y, ref, bound)

    # backward through a linear layer (dZ = dy), operands bf16-valued
    lin = DenseLayer(In, Out, act="none", device="cpu")
    lin.W, lin.b = W.clone(), b.clone()
    lin.forward_cpu(x)
    dZ, _, _ = operands(kind, B_, 3, Out)     # [B, Out]
    dx = lin.backward_cpu(dZ)
    checks = [("dW", lin._dW, (dZ, x, 1, 1)),
              ("dx", dx, (dZ, W, 0, 1)),
              ("dx.mirror", dx, (dZ, W.t().contiguous(), 0, 0))]
    for name, got, (A, Bm, ta, tb) in checks:
        ref, _ = go.gemm_ref(A, Bm, ta, tb)
        if kind == "exact":
            assert torch.equal(got.double(), ref), name
        else:
            ko.check_bound(f"backward_cpu-{name}", got, ref,
                           go.sum_bound(A, Bm, ta, tb))
    # layout (1, 0) is the remaining one: A stored [K, M], B stored [N, K]
    A, Bm, _ = operands(kind, 33, 9, 40, 1, 0)
    ref, _ = go.gemm_ref(A, Bm, 1, 0)
    assert torch.allclose(ref, A.double().t() @ Bm.double().t(), rtol=0,
                          atol=1e-12)


def test_exact_rule_holds_for_every_case_and_is_tight():
    for K in [c[2] for c in go.generic_cases()] + [k for k, _ in
                                                   go.SPLITK_CASES] + \
            go.G256_K + go.WGRAD_K + [c[2] for c in go.V2_CASES]:
        go.assert_exact(K)
    with pytest.raises(AssertionError):
        go.assert_exact(2 ** 24 // 9 + 1)
    # the largest |value| really is K amax bmax + biasmax
    a = torch.full((1, 200), 3.0)
    ref, _ = go.gemm_ref(a, a, 0, 0, torch.tensor([8.0]))
    assert float(ref) == 200 * 9 + 8


def test_structured_fills():
    A, B, _ = go.exact_operands(17, 9, 200, fill="lastk")
    assert (A[:, :-1] == 0).all() and (A[:, -1] != 0).all()
    assert (B[:, :-1] == 0).all() and (B[:, -1] != 0).all()
    A, B, _ = go.exact_operands(17, 9, 200, 1, 1, fill="tilefirst")
    keep = torch.zeros(200, dtype=torch.bool)
    keep[[0, 64, 128, 192]] = True
    assert (A[~keep] == 0).all() and (A[keep] != 0).all()
    assert (B[~keep] == 0).all() and (B[keep] != 0).all()


def test_operands_are_bf16_valued_and_seeded_per_shape():
    for kind in ("exact", "float"):
        A, B, _ = operands(kind, 33, 17, 72)
        assert torch.equal(A, A.to(go.BF).float())
        assert torch.equal(B, B.to(go.BF).float())
        A2, _, _ = operands(kind, 33, 17, 72)
        assert torch.equal(A, A2)
        A3, _, _ = operands(kind, 33, 17, 72, 1, 0)
        assert not torch.equal(A, A3.t())
    A, B, bias = go.exact_operands(64, 64, 64)
    assert A.abs().max() == go.OP_MAX and bias.abs().max() <= go.BIAS_MAX
    assert set(A.unique().tolist()) == set(range(-3, 4))


def test_embed_is_a_contiguous_view_inside_nan():
    t = torch.arange(12.0).view(3, 4)
    for mis in (False, True):
        off = go.PAD + int(mis)
        buf = torch.full((12 + 2 * go.PAD + 8,), float("nan"),
                         dtype=go.BF)
        view = buf[off:off + 12].view(3, 4)
        view.copy_(t.to(go.BF))
        assert view.is_contiguous()
        assert (view.data_ptr() - buf.data_ptr()) % 16 == (2 if mis else 0)
        assert torch.isnan(buf[:off]).all() and torch.isnan(
            buf[off + 12:]).all()


def test_tile_constants_match_sources():
    """the case lists are built around these; a retuned tile must bring
    its edges into the lists"""
    text = "".join(p.read_text() for p in sorted(CSRC.glob("gemm*.hip"))
                   if not p.name.endswith("_hip.hip"))
    for name, val in go.TILE.items():
        m = re.search(rf"#define {name} (\d+)", text)
        assert m and int(m.group(1)) == val, name
    bm, bk = go.TILE["GEMM_BM"], go.TILE["GEMM_BK"]
    for d in (-1, 0, 1, -8, 8):
        assert bm + d in go.GENERIC_MN
        assert bk + d in go.GENERIC_K and 2 * bk + d in go.GENERIC_K
    wg = go.TILE["WG_BM"]
    assert {wg - 16, wg, wg + 16, 2 * wg, 2 * wg + 16} <= set(go.WGRAD_MN)
    wk = go.TILE["WG_BK"]
    for d in (-1, 0, 1, -8, 8):
        assert 32 * wk + d in go.WGRAD_K
    assert all(k % go.TILE["GN128_BK"] == 0 for _, _, k in go.N128_CASES)
    assert all(k % (2 * go.TILE["V2_CK"]) == 0 for _, _, k in go.V2_CASES)


# ---------------------------------------------------------------------------
# 2. wrong references on the GPU tests' own inputs
# ---------------------------------------------------------------------------
def all_exact_cases():
    """(variant, ta, tb, shape) of every exact-set sweep of the GPU file"""
    out = []
    for ta, tb in go.LAYOUTS:
        out += [("generic", ta, tb, s) for s in go.generic_cases()]
        out += [("generic", ta, tb, go.SPLITK_MN + (k,))
                for k, _ in go.SPLITK_CASES]
    out += [("gemm256", 0, 0, s) for s in go.tile256_cases(go.G256_GRIDS)]
    out += [("p8", 0, 0, s) for s in go.tile256_cases(go.P8_GRIDS)]
    out += [("v2", 0, 0, s) for s in go.V2_CASES]
    out += [("n128", 0, 0, s) for s in go.N128_CASES]
    out += [("wgrad128", 1, 1, s) for s in go.wgrad_cases()]
    return out


def small(cases, limit=2 ** 28):
    """cases whose M N K keeps the CPU matmuls of a mutation sweep short;
    every body and every K of the lists stays represented"""
    return [c for c in cases if c[3][0] * c[3][1] * c[3][2] <= limit]


EXACT_CASES = small(all_exact_cases())


def test_sweep_keeps_every_body_and_k():
    ks = lambda cases: {(c[0], c[3][2]) for c in cases}
    assert ks(EXACT_CASES) == ks(all_exact_cases())


def test_wrong_dropk_and_tail_chunk_differ_everywhere():
    """on every exact case (K = 1 apart: nothing is left to drop from),
    random fill; the 'lastk' fill makes the difference the whole result"""
    for variant, ta, tb, (M, N, K) in EXACT_CASES:
        A, B, _ = go.exact_operands(M, N, K, ta, tb)
        ref, _ = go.gemm_ref(A, B, ta, tb)
        if K > 1:
            assert ko.differs(ref, go.wrong_dropk(A, B, ta, tb)), \
                (variant, ta, tb, M, N, K)
        if go.tail_chunk_start(K) > 0:
            assert ko.differs(ref, go.wrong_drop_tail_chunk(A, B, ta, tb))
    A, B, _ = go.exact_operands(129, 129, 72, fill="lastk")
    ref, _ = go.gemm_ref(A, B, 0, 0)
    assert (ref != 0).all()
    assert (go.wrong_dropk(A, B, 0, 0) == 0).all()
    assert (go.wrong_drop_tail_chunk(A, B, 0, 0) == 0).all()


def test_wrong_tail_readthrough_differs():
    """every untransposed case with a K tail: finite where the next row
    exists, NaN past the end (the GPU buffers hold NaN there too)"""
    n = 0
    for variant, ta, tb, (M, N, K) in EXACT_CASES:
        if ta or tb or K % 64 == 0:
            continue
        A, B, _ = go.exact_operands(M, N, K)
        ref, _ = go.gemm_ref(A, B, 0, 0)
        bad = go.wrong_tail_readthrough(A, B)
        assert ko.differs(ref, bad), (variant, M, N, K)
        assert torch.isnan(bad[-1]).all() and torch.isnan(bad[:, -1]).all()
        r = -(-((-K) % 64) // K)  # rows the read-through runs into
        if M > r and N > r:
            assert torch.isfinite(bad[:M - r, :N - r]).all()
            assert ko.differs(ref[:M - r, :N - r], bad[:M - r, :N - r])
        n += 1
    assert n > 40


def test_wrong_b_layout_differs():
    for variant, ta, tb, (M, N, K) in EXACT_CASES:
        if N == 1 or K == 1:
            continue  # a vector has one layout
        A, B, _ = go.exact_operands(M, N, K, ta, tb)
        ref, _ = go.gemm_ref(A, B, ta, tb)
        assert ko.differs(ref, go.wrong_b_layout(A, B, ta, tb)), \
            (variant, ta, tb, M, N, K)


def test_wrong_swap_halves_differs():
    n = 0
    for variant, ta, tb, (M, N, K) in EXACT_CASES:
        if M < 256:
            continue
        A, B, _ = go.exact_operands(M, N, K, ta, tb)
        ref, _ = go.gemm_ref(A, B, ta, tb)
        assert ko.differs(ref, go.wrong_swap_halves(A, B, ta, tb))
        n += 1
    assert n > 40


def test_wrong_stale_tile_differs():
    n = 0
    for variant, ta, tb, (M, N, K) in EXACT_CASES:
        bk = 32 if variant == "v2" else 64
        if K <= bk:
            continue
        A, B, _ = go.exact_operands(M, N, K, ta, tb)
        ref, _ = go.gemm_ref(A, B, ta, tb)
        assert ko.differs(ref, go.wrong_stale_tile(A, B, ta, tb, bk=bk)), \
            (variant, ta, tb, M, N, K)
        n += 1
    assert n > 100


def test_wrong_epilogues_differ():
    """on the epilogue cases of every body: bias once per split-K block
    (two blocks), relu against the bias, Cbf from the pre-activation"""
    for body, shapes in go.EPILOGUE_SHAPES.items():
        for variant, ta, tb, (M, N, K) in shapes:
            A, B, bias = go.exact_operands(M, N, K, ta, tb)
            for act in (0, 1):
                ref, _ = go.gemm_ref(A, B, ta, tb, bias, act)
                assert ko.differs(ref, go.wrong_bias_per_chunk(
                    A, B, ta, tb, bias, 2, act)), (variant, act)
            relu, z = go.gemm_ref(A, B, ta, tb, bias, 1)
            assert ko.differs(relu, go.wrong_relu_vs_bias(A, B, ta, tb,
                                                          bias))
            for act in (1, 2):
                ref, _ = go.gemm_ref(A, B, ta, tb, bias, act)
                good = ref.float().to(go.BF)
                bad = go.wrong_cbf_preact(A, B, ta, tb, bias, act)
                assert (ko._bits(good) != ko._bits(bad)).any(), (variant,
                                                                 act)
    # split-K itself has no bias: the wrong reference says what a kernel
    # would give if it took one
    M, N = go.SPLITK_MN
    for K, z in go.SPLITK_CASES:
        A, B, bias = go.exact_operands(M, N, K)
        ref, _ = go.gemm_ref(A, B, 0, 0, bias)
        nb = go.split_blocks(K, z)
        assert nb > 1
        assert ko.differs(ref, go.wrong_bias_per_chunk(A, B, 0, 0, bias, nb))


# ---------------------------------------------------------------------------
# 3. the float set: each wrong reference leaves the bound
# ---------------------------------------------------------------------------
def float_cases():
    return [(body, v, ta, tb, z, s) for body, cs in go.FLOAT_CASES.items()
            for v, ta, tb, z, s in cs]


def test_float_bound_is_above_fp32_and_below_the_mistakes():
    """the fp32 CPU product sits inside the bound (so a correct kernel
    can), every wrong reference outside it in at least one element. The
    last k column is scaled by lastk_scale_for(K) (1 below K ~ 1400, 4 at
    K ~ 4100), as kernel_oracles scales the last row for colsum, so that
    one lost column stays above a bound that grows like K^2."""
    for body, variant, ta, tb, z, (M, N, K) in float_cases():
        A, B, bias = operands("float", M, N, K, ta, tb)
        tag = (variant, ta, tb, z, M, N, K)
        ref, _ = go.gemm_ref(A, B, ta, tb)
        bound = go.sum_bound(A, B, ta, tb)
        a, b = go.logical(A, B, ta, tb)
        fp32 = a.float() @ b.float().t()
        assert not ko.differs(fp32, ref, bound), tag
        assert ko.differs(ref, go.wrong_dropk(A, B, ta, tb), bound), tag
        assert ko.differs(ref, go.wrong_drop_tail_chunk(A, B, ta, tb),
                          bound), tag
        assert ko.differs(ref, go.wrong_b_layout(A, B, ta, tb), bound), tag
        bk = 32 if body == "v2" else 64
        assert ko.differs(ref, go.wrong_stale_tile(A, B, ta, tb, bk=bk),
                          bound), tag
        if M >= 256:
            assert ko.differs(ref, go.wrong_swap_halves(A, B, ta, tb),
                              bound), tag
        if not ta and not tb and K % 64:
            bad = go.wrong_tail_readthrough(A, B)
            assert ko.differs(ref[:-1, :-1], bad[:-1, :-1],
                              bound[:-1, :-1]), tag
        if z:
            nb = go.split_blocks(K, z)
            assert ko.differs(ref + bias.double(), go.wrong_bias_per_chunk(
                A, B, ta, tb, bias, nb), bound + ko.U24 * (
                    ref.abs() + bias.double().abs())), tag
        if z == 0 and body != "wgrad128":
            s = ref
            for act in (1, 2):
                want, eb = go.epilogue_bound(s, bound, bias, act)
                if act == 1:
                    assert ko.differs(want, go.wrong_relu_vs_bias(
                        A, B, ta, tb, bias), eb), tag
                good = want.float().to(go.BF)
                bad = go.wrong_cbf_preact(A, B, ta, tb, bias, act)
                assert (ko._bits(good) != ko._bits(bad)).any(), tag


def test_lastk_scale():
    assert go.lastk_scale_for(72) == 1.0 and go.lastk_scale_for(1057) == 1.0
    assert go.lastk_scale_for(4160) == 4.0
    assert all(go.lastk_scale_for(s[2]) <= 4.0
               for _, _, _, _, _, s in float_cases())
