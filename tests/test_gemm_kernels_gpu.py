"""Parity tests for the dense engine (gemm_kernels.hip, gemm256*.hip,
gemm_wgrad_kernels.hip) against the float64 reference of
``gemm_oracles.py``.

Main set: integer operands on which fp32 accumulation is exact in any
order (rule and magnitude condition in ``gemm_oracles.py``, asserted for
every case), so every comparison is bit for bit and no tile order, MFMA
chaining or split-K atomic order can excuse a difference. Operands are
views inside NaN-filled buffers and the outputs' blocks are poisoned, so a
read past a row or a tile and an unwritten output both surface as NaN.

Every body is launched directly through ``gemm_bf16_variant``; wherever
``gemm_bf16_route`` says the default dispatch reaches the same body, the
plain ``gemm_bf16`` / ``gemm_bf16_full`` entry is run and checked too. A
small float set keeps real rounding in view under the derived bounds.
``test_gemm_oracles.py`` shows on the CPU that the wrong references listed
in docs/TESTING.md differ on these same inputs.
"""

import pytest
import torch

import gemm_oracles as go
import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def route_of(M, N, K, ta, tb, has_bias=False, act=0, emit=False):
    return ops().gemm_bf16_route(M, N, K, ta, tb, has_bias, act, emit)


def variant_route(variant, split_z):
    """the name gemm_bf16_route gives a (variant, split_z) pair"""
    if variant in ("generic", "wgrad128"):
        return f"{variant}:split={split_z}"
    return variant


def poison_out(M, N, emit):
    ko.poison((M, N), torch.float32, DEV)
    if emit:
        ko.poison((M, N), BF, DEV)


def launch(entry, Ad, Bd, biasd, shape, ta, tb, act, emit, variant, split_z):
    """one call through the variant binding or the default entries;
    returns (C, Cbf or None)"""
    M, N, K = shape
    poison_out(M, N, emit)
    if entry == "variant":
        out = ops().gemm_bf16_variant(Ad, Bd, biasd, M, N, K, ta, tb, act,
                                      emit, variant, split_z)
        return out[0], (out[1] if emit else None)
    if emit:
        C, Cbf = ops().gemm_bf16_full(Ad, Bd, biasd, M, N, K, ta, tb, act)
        return C, Cbf
    return ops().gemm_bf16(Ad, Bd, biasd, M, N, K, ta, tb, act, False), None


def check_case(name, variant, shape, ta=0, tb=0, split_z=0, has_bias=False,
               act=0, emit=False, fill="random", kind="exact",
               misalign=None, entries=None, repeat=1, expect_default=None):
    """Build the case, run it through the variant binding and, when the
    default dispatch routes the same shape to the same body, through the
    plain entry; compare each output with the reference.

    expect_default: True / False asserts that the default route does / does
    not reach this body (None: whichever it is, both are checked when it
    does). Returns the entries that ran."""
    M, N, K = shape
    if kind == "exact":
        A, B, bias = go.exact_operands(M, N, K, ta, tb, fill=fill)
    else:
        A, B, bias = go.float_operands(M, N, K, ta, tb,
                                       lastk_scale=go.lastk_scale_for(K))
    if not has_bias:
        bias = None
    ref, z = go.gemm_ref(A, B, ta, tb, bias, act)
    if kind == "exact" and act != 2:
        bound = None
    else:
        sb = (torch.zeros_like(ref) if kind == "exact"
              else go.sum_bound(A, B, ta, tb))
        s, _ = go.gemm_ref(A, B, ta, tb)
        ref2, bound = go.epilogue_bound(s, sb, bias, act)
        assert torch.equal(ref2, ref), name
    Ad, Abuf = go.embed(A, DEV, misalign == "A")
    Bd, Bbuf = go.embed(B, DEV, misalign == "B")
    biasd = bias.to(DEV) if has_bias else None

    default = route_of(M, N, K, ta, tb, has_bias, act, emit)
    reached = default == variant_route(variant, split_z)
    if expect_default is not None:
        assert reached == expect_default, (name, default, variant, split_z)
    if entries is None:
        entries = ["variant"] + (["default"] if reached and not misalign
                                 else [])
    first = None
    for entry in entries:
        for it in range(repeat):
            C, Cbf = launch(entry, Ad, Bd, biasd, shape, ta, tb, act, emit,
                            variant, split_z)
            tag = f"{name}[{entry}#{it}]"
            if bound is None:
                ko.check_bits(tag + ".C", C, ref.float())
            else:
                ko.check_bound(tag + ".C", C, ref, bound)
            if emit:
                ko.check_bits(tag + ".Cbf", Cbf, C.cpu().to(BF))
            if repeat > 1:
                if first is None:
                    first = C.cpu()
                ko.check_bits(tag + ".rerun", C, first)
    del Abuf, Bbuf
    return entries


def cname(variant, shape, ta=0, tb=0, extra=""):
    return f"{variant}-{ta}{tb}-{'x'.join(map(str, shape))}{extra}"


# ---------------------------------------------------------------------------
# generic 128^2 kernel, all four layouts
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ta,tb", go.LAYOUTS)
def test_generic_edges(ta, tb):
    """M, N and K one axis at a time around (129, 129, 72): K % 8 == 0
    takes glds on full tiles of untransposed operands, everything else the
    scalar staging."""
    for shape in go.generic_cases():
        check_case(cname("generic", shape, ta, tb), "generic", shape, ta,
                   tb)


@pytest.mark.parametrize("ta,tb", go.LAYOUTS)
@pytest.mark.parametrize("fill", ["lastk", "tilefirst"])
def test_generic_structured(ta, tb, fill):
    """only column K-1 / only the first k of each K tile non-zero"""
    for shape in [(129, 129, 72), (129, 129, 200), (17, 65, 127),
                  (128, 128, 136)]:
        check_case(cname("generic", shape, ta, tb, "-" + fill), "generic",
                   shape, ta, tb, fill=fill)


def test_generic_default_route_reaches_all_layouts():
    """shapes no fast path takes run the generic kernel by default"""
    for ta, tb in go.LAYOUTS:
        for shape in [(129, 129, 72), (257, 129, 72), (129, 129, 9)]:
            ran = check_case(cname("generic", shape, ta, tb), "generic",
                             shape, ta, tb, expect_default=True)
            assert ran == ["variant", "default"]


@pytest.mark.parametrize("ta,tb", go.LAYOUTS)
def test_generic_splitk(ta, tb):
    """split-K atomics: whole chunks, a short last chunk, the K tail
    inside the last chunk, fewer blocks than requested; three runs each,
    bit-identical. (K, 64) is the default fan-out of these shapes."""
    M, N = go.SPLITK_MN
    for K, z in go.SPLITK_CASES:
        if z == 64:
            assert go.split_blocks(K, z) <= 64
        ran = check_case(cname("generic", (M, N, K), ta, tb, f"-z{z}"),
                         "generic", (M, N, K), ta, tb, split_z=z, repeat=3,
                         expect_default=(z == 64))
        assert ("default" in ran) == (z == 64)
    assert go.split_blocks(4160, 4) == 4 and 4160 - 3 * go.split_chunk(
        4160, 4) < go.split_chunk(4160, 4)
    assert go.split_blocks(4104, 64) < 64
    assert (4097 - 7 * go.split_chunk(4097, 8)) % 64 == 1


def test_generic_splitk_structured():
    for fill in ("lastk", "tilefirst"):
        for K, z in [(4097, 8), (4160, 4)]:
            check_case(cname("generic", (129, 65, K), 0, 0, f"-z{z}-{fill}"),
                       "generic", (129, 65, K), split_z=z, fill=fill)


# ---------------------------------------------------------------------------
# 256^2 kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", go.G256_VARIANTS)
def test_gemm256_edges(variant):
    """every K on one tile (NT = 1, 2, 3, 5 with and without a tail; the
    TAIL body for K % 64 != 0), every grid at a tail and a full K"""
    n = 0
    for shape in go.tile256_cases(go.G256_GRIDS):
        if go.g256_variant_ok(variant, shape[2]):
            check_case(cname(variant, shape), variant, shape)
            n += 1
    assert n >= 6  # pipe 2: K = 64, 128, 192 and three more grids at 192


def test_gemm256_default_route():
    """K % 64 == 0 runs pipe 2 without burst by default; the K-tail
    shapes go to p8"""
    for shape in [(256, 256, 64), (512, 512, 192), (256, 768, 128)]:
        ran = check_case(cname("gemm256_p2_b0", shape), "gemm256_p2_b0",
                         shape, expect_default=True)
        assert "default" in ran
    for shape in [(256, 256, 72), (512, 512, 200)]:
        ran = check_case(cname("p8_lite", shape), "p8_lite", shape,
                         expect_default=True)
        assert "default" in ran


@pytest.mark.parametrize("variant", ["gemm256_p0_b0", "gemm256_p1_b1",
                                     "gemm256_p2_b0"])
@pytest.mark.parametrize("fill", ["lastk", "tilefirst"])
def test_gemm256_structured(variant, fill):
    for shape in [(256, 256, 136), (512, 256, 192), (256, 256, 40)]:
        if go.g256_variant_ok(variant, shape[2]):
            check_case(cname(variant, shape, extra="-" + fill), variant,
                       shape, fill=fill)


@pytest.mark.parametrize("variant", go.P8_VARIANTS)
def test_p8_edges(variant):
    """NT = 1, 2, 3, 5 tiles with and without the masked-glds tail; grids
    of 1, 2, 15 (not a multiple of the 8 XCDs) and 16 tiles"""
    for shape in go.tile256_cases(go.P8_GRIDS):
        check_case(cname(variant, shape), variant, shape)


@pytest.mark.parametrize("variant", go.P8_VARIANTS)
@pytest.mark.parametrize("fill", ["lastk", "tilefirst"])
def test_p8_structured(variant, fill):
    for shape in [(256, 256, 136), (512, 256, 200), (256, 256, 40)]:
        check_case(cname(variant, shape, extra="-" + fill), variant, shape,
                   fill=fill)


def test_v2_edges():
    """6, 8, 10 and 14 chunks of 32: the slot rotation wraps once, twice
    and three times"""
    assert go.TILE["V2_CK"] == 32
    for shape in go.V2_CASES:
        check_case(cname("v2", shape), "v2", shape, expect_default=False)
    for fill in ("lastk", "tilefirst"):
        check_case(cname("v2", (256, 256, 320), extra="-" + fill), "v2",
                   (256, 256, 320), fill=fill)


def test_n128_edges():
    """full and partial last column tile, one to three K tiles; the
    default dispatch takes K >= 128"""
    for shape in go.N128_CASES:
        ran = check_case(cname("n128", shape), "n128", shape,
                         expect_default=shape[2] >= 128)
        assert ("default" in ran) == (shape[2] >= 128)
    for fill in ("lastk", "tilefirst"):
        check_case(cname("n128", (256, 200, 192), extra="-" + fill), "n128",
                   (256, 200, 192), fill=fill)


# ---------------------------------------------------------------------------
# wgrad128
# ---------------------------------------------------------------------------
def test_wgrad128_edges():
    """M, N, K one axis at a time around (144, 272, 1057), unsplit and
    with the default fan-out (which the plain entry must reach)"""
    for shape in go.wgrad_cases():
        M, N, K = shape
        check_case(cname("wgrad128", shape, 1, 1), "wgrad128", shape, 1, 1,
                   split_z=0)
        r = route_of(M, N, K, 1, 1)
        assert r.startswith("wgrad128:split="), (shape, r)
        z = int(r.split("=")[1])
        assert (z > 0) == (K >= 2048)
        ran = check_case(cname("wgrad128", shape, 1, 1, f"-z{z}"),
                         "wgrad128", shape, 1, 1, split_z=z,
                         expect_default=True)
        assert "default" in ran


def test_wgrad128_explicit_splits():
    """explicit fan-outs with a short last chunk, three runs each"""
    for K, z in go.WGRAD_SPLITS:
        for M, N in [(144, 272), (128, 128), (16, 624)]:
            check_case(cname("wgrad128", (M, N, K), 1, 1, f"-z{z}"),
                       "wgrad128", (M, N, K), 1, 1, split_z=z, repeat=3)
    assert 4100 - 2 * go.split_chunk(4100, 3) < go.split_chunk(4100, 3)
    for fill in ("lastk", "tilefirst"):
        check_case(cname("wgrad128", (144, 272, 2049), 1, 1, "-" + fill),
                   "wgrad128", (144, 272, 2049), 1, 1, split_z=5, fill=fill)


def test_wgrad128_own_binding():
    for M, N, K in [(144, 272, 1057), (128, 256, 4100)]:
        A, B, _ = go.exact_operands(M, N, K, 1, 1)
        ref, _ = go.gemm_ref(A, B, 1, 1)
        Ad, Abuf = go.embed(A, DEV)
        Bd, Bbuf = go.embed(B, DEV)
        ko.poison((M, N), torch.float32, DEV)
        C = ops().gemm_wgrad_bf16(Ad, Bd, M, N, K)
        ko.check_bits(f"gemm_wgrad_bf16-{M}x{N}x{K}", C, ref.float())


# ---------------------------------------------------------------------------
# epilogues
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("body", sorted(go.EPILOGUE_SHAPES))
def test_epilogues(body):
    """no bias / bias x act 0/1/2 x with / without Cbf, at an interior and
    an edge shape of each body; sigmoid under its bound, the rest bit for
    bit, Cbf bit-equal to bf16(C)"""
    for variant, ta, tb, shape in go.EPILOGUE_SHAPES[body]:
        for hb, act, emit in go.EPILOGUES:
            check_case(cname(variant, shape, ta, tb,
                             f"-b{int(hb)}a{act}e{int(emit)}"),
                       variant, shape, ta, tb, has_bias=hb, act=act,
                       emit=emit)


def test_epilogue_default_entries_reach_each_body():
    """gemm_bf16_full with bias + relu reaches gemm256, p8, n128 and the
    generic kernel by default"""
    for variant, shape in [("gemm256_p2_b0", (512, 512, 128)),
                           ("p8_lite", (256, 512, 72)),
                           ("n128", (256, 200, 192)),
                           ("generic:split=0", (129, 65, 72))]:
        M, N, K = shape
        assert route_of(M, N, K, 0, 0, True, 1, True) == variant


# ---------------------------------------------------------------------------
# float set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("body", sorted(go.FLOAT_CASES))
def test_float_set(body):
    """bf16 of 0.5 N(0,1) under K 2^-23 sum|a b| plus the epilogue chain"""
    for variant, ta, tb, z, shape in go.FLOAT_CASES[body]:
        check_case(f"float.{body}." + cname(variant, shape, ta, tb,
                                            f"-z{z}"),
                   variant, shape, ta, tb, split_z=z, kind="float")
        if z == 0 and body != "wgrad128":
            for hb, act, emit in go.FLOAT_EPILOGUES:
                check_case(f"float.{body}." + cname(variant, shape, ta, tb,
                                                    f"-a{act}"),
                           variant, shape, ta, tb, has_bias=hb, act=act,
                           emit=emit, kind="float")


# ---------------------------------------------------------------------------
# race screen of the body the old screen never ran
# ---------------------------------------------------------------------------
def test_v2_race_screen_exact():
    """10 runs of the v2 body on a 4 x 4 grid, 16 chunks deep, bit for
    bit (test_nn.py::test_gemm_v2_race_screen runs the same count under
    its own tolerance)"""
    check_case("v2-race", "v2", (1024, 1024, 512), repeat=10)


# ---------------------------------------------------------------------------
# misaligned views
# ---------------------------------------------------------------------------
MISALIGNED = [
    # (shape, ta, tb, body the aligned shape routes to)
    ((256, 256, 64), 0, 0, "gemm256_p2_b0"),
    ((256, 256, 72), 0, 0, "p8_lite"),
    ((256, 384, 128), 0, 0, "n128"),
    ((144, 272, 1056), 1, 1, "wgrad128:split=0"),
    ((128, 128, 64), 0, 0, "generic:split=0"),
    ((129, 129, 72), 1, 0, "generic:split=0"),
    ((129, 129, 72), 0, 1, "generic:split=0"),
    ((129, 65, 4096), 0, 0, "generic:split=64"),
]


@pytest.mark.parametrize("which", ["A", "B"])
def test_misaligned_views_run_exact(which):
    """an operand whose base is two bytes off 16-byte alignment runs (on
    the element-wise staging of the generic kernel) and is exact through
    gemm_bf16"""
    for shape, ta, tb, aligned_route in MISALIGNED:
        M, N, K = shape
        assert route_of(M, N, K, ta, tb) == aligned_route
        check_case(cname("misaligned" + which, shape, ta, tb), "generic",
                   shape, ta, tb, misalign=which, entries=["default"])
        check_case(cname("misaligned" + which, shape, ta, tb, "-variant"),
                   "generic", shape, ta, tb, misalign=which,
                   entries=["variant"])


@pytest.mark.parametrize("which", ["A", "B"])
def test_misaligned_views_raise_on_glds_bodies(which):
    for variant, ta, tb, shape in [("gemm256_p2_b0", 0, 0, (256, 256, 64)),
                                   ("gemm256_p0_b0", 0, 0, (256, 256, 72)),
                                   ("p8_lite", 0, 0, (256, 256, 72)),
                                   ("p8_full_xcd", 0, 0, (256, 256, 64)),
                                   ("v2", 0, 0, (256, 256, 192)),
                                   ("n128", 0, 0, (256, 384, 128)),
                                   ("wgrad128", 1, 1, (144, 272, 1056))]:
        M, N, K = shape
        A, B, _ = go.exact_operands(M, N, K, ta, tb)
        Ad, Abuf = go.embed(A, DEV, which == "A")
        Bd, Bbuf = go.embed(B, DEV, which == "B")
        with pytest.raises(RuntimeError, match="aligned"):
            ops().gemm_bf16_variant(Ad, Bd, None, M, N, K, ta, tb, 0, False,
                                    variant, 0)
    M, N, K = 144, 272, 1056
    A, B, _ = go.exact_operands(M, N, K, 1, 1)
    Ad, Abuf = go.embed(A, DEV, which == "A")
    Bd, Bbuf = go.embed(B, DEV, which == "B")
    with pytest.raises(RuntimeError, match="aligned"):
        ops().gemm_wgrad_bf16(Ad, Bd, M, N, K)


# ---------------------------------------------------------------------------
# binding checks: raise, never abort
# ---------------------------------------------------------------------------
def _entries():
    """the three GEMM bindings behind one signature"""
    o = ops()
    return {
        "gemm_bf16": lambda A, B, bias, M, N, K, ta, tb, act:
            o.gemm_bf16(A, B, bias, M, N, K, ta, tb, act, False),
        "gemm_bf16_full": lambda A, B, bias, M, N, K, ta, tb, act:
            o.gemm_bf16_full(A, B, bias, M, N, K, ta, tb, act),
        "gemm_bf16_variant": lambda A, B, bias, M, N, K, ta, tb, act:
            o.gemm_bf16_variant(A, B, bias, M, N, K, ta, tb, act, False,
                                "generic", 0),
    }


@pytest.mark.parametrize("entry", ["gemm_bf16", "gemm_bf16_full",
                                   "gemm_bf16_variant"])
def test_bindings_raise(entry):
    f = _entries()[entry]
    M, N, K = 32, 48, 64
    A = torch.ones(M, K, dtype=BF, device=DEV)
    B = torch.ones(N, K, dtype=BF, device=DEV)
    bias = torch.zeros(N, device=DEV)
    f(A, B, bias, M, N, K, 0, 0, 0)  # the well-formed call passes
    bad = {
        "A not contiguous":
            (torch.ones(K, M, dtype=BF, device=DEV).t(), B, bias, M, N, K,
             0, 0, 0),
        "B not contiguous":
            (A, torch.ones(N, 2 * K, dtype=BF, device=DEV)[:, ::2], bias, M,
             N, K, 0, 0, 0),
        "A too small": (A, B, bias, M + 1, N, K, 0, 0, 0),
        "A too large": (A, B, bias, M - 1, N, K, 0, 0, 0),
        "B too small": (A, B, bias, M, N + 16, K, 0, 0, 0),
        "B too large": (A, B, bias[:N - 16], M, N - 16, K, 0, 0, 0),
        "K mismatch": (A, B, bias, M, N, K + 8, 0, 0, 0),
        "bias short": (A, B, bias[:N - 1], M, N, K, 0, 0, 0),
        "bias long": (A, B, torch.zeros(N + 1, device=DEV), M, N, K, 0, 0,
                      0),
        "bias bf16": (A, B, bias.to(BF), M, N, K, 0, 0, 0),
        "bias f64": (A, B, bias.double(), M, N, K, 0, 0, 0),
        "bias on cpu": (A, B, bias.cpu(), M, N, K, 0, 0, 0),
        "A fp32": (A.float(), B, bias, M, N, K, 0, 0, 0),
        "B on cpu": (A, B.cpu(), bias, M, N, K, 0, 0, 0),
        "M = 0": (A[:0], B, bias, 0, N, K, 0, 0, 0),
        "N = 0": (A, B[:0], bias[:0], M, 0, K, 0, 0, 0),
        "K = 0": (A[:, :0].contiguous(), B[:, :0].contiguous(), bias, M, N,
                  0, 0, 0, 0),
        "M < 0": (A, B, bias, -M, N, K, 0, 0, 0),
        "transA = 2": (A, B, bias, M, N, K, 2, 0, 0),
        "transA = -1": (A, B, bias, M, N, K, -1, 0, 0),
        "transB = 2": (A, B, bias, M, N, K, 0, 2, 0),
        "act = 3": (A, B, bias, M, N, K, 0, 0, 3),
        "act = -1": (A, B, bias, M, N, K, 0, 0, -1),
    }
    for what, args in bad.items():
        with pytest.raises(RuntimeError):
            f(*args)
            pytest.fail(f"{entry}: {what} did not raise")
    torch.cuda.synchronize()
    f(A, B, bias, M, N, K, 0, 0, 0)  # and the process is still healthy


def test_variant_binding_rejects_what_a_body_cannot_take():
    o = ops()

    def call(variant, shape, ta=0, tb=0, act=0, emit=False, z=0, bias=False):
        M, N, K = shape
        A = torch.ones(M * K, dtype=BF, device=DEV)
        B = torch.ones(N * K, dtype=BF, device=DEV)
        b = torch.zeros(N, device=DEV) if bias else None
        return o.gemm_bf16_variant(A, B, b, M, N, K, ta, tb, act, emit,
                                   variant, z)

    bad = [
        ("nosuch", (256, 256, 64), {}),
        ("gemm256_p3_b0", (256, 256, 64), {}),
        ("gemm256_p0_b2", (256, 256, 64), {}),
        ("p8_full_apipe", (256, 256, 64), {}),
        ("p8_deepa", (256, 256, 64), {}),
        ("gemm256_p0_b0", (128, 256, 64), {}),
        ("gemm256_p0_b0", (256, 384, 64), {}),
        ("gemm256_p0_b0", (256, 256, 68), {}),
        ("gemm256_p0_b0", (256, 256, 24), {}),
        ("gemm256_p2_b0", (256, 256, 72), {}),      # pipe 2 has no tail
        ("gemm256_p0_b0", (256, 256, 64), dict(ta=1)),
        ("gemm256_p0_b0", (256, 256, 64), dict(z=2)),
        ("p8_lite", (256, 256, 60), {}),
        ("p8_lite", (256, 200, 64), {}),
        ("p8_lite", (256, 256, 64), dict(tb=1)),
        ("v2", (256, 256, 128), {}),
        ("v2", (256, 256, 224), {}),
        ("v2", (256, 128, 192), {}),
        ("n128", (128, 128, 128), {}),
        ("n128", (256, 128, 96), {}),
        ("n128", (256, 128, 128), dict(ta=1)),
        ("wgrad128", (144, 272, 1056), dict(ta=0, tb=1)),
        ("wgrad128", (140, 272, 1056), dict(ta=1, tb=1)),
        ("wgrad128", (144, 272, 512), dict(ta=1, tb=1)),
        ("wgrad128", (144, 272, 1056), dict(ta=1, tb=1, bias=True)),
        ("wgrad128", (144, 272, 1056), dict(ta=1, tb=1, act=1)),
        ("wgrad128", (144, 272, 1056), dict(ta=1, tb=1, emit=True)),
        ("generic", (129, 65, 4096), dict(z=8, bias=True)),
        ("generic", (129, 65, 4096), dict(z=8, act=1)),
        ("generic", (129, 65, 4096), dict(z=8, emit=True)),
        ("generic", (129, 65, 4096), dict(z=-1)),
        ("generic", (129, 65, 4096), dict(z=1 << 20)),
    ]
    for variant, shape, kw in bad:
        with pytest.raises(RuntimeError):
            call(variant, shape, **kw)
            pytest.fail(f"{variant} {shape} {kw} did not raise")
    for variant, shape, kw in [("gemm256_p0_b0", (256, 256, 72), {}),
                               ("p8_lite_apipe", (256, 256, 64), {}),
                               ("generic", (129, 65, 4096), dict(z=8))]:
        call(variant, shape, **kw)
    torch.cuda.synchronize()


def test_wgrad_binding_raises():
    o = ops()
    M, N, K = 32, 48, 1024
    At = torch.ones(K, M, dtype=BF, device=DEV)
    Bt = torch.ones(K, N, dtype=BF, device=DEV)
    C = o.gemm_wgrad_bf16(At, Bt, M, N, K)
    assert torch.equal(C.cpu(), torch.full((M, N), float(K)))
    bad = {
        "At not contiguous":
            (torch.ones(M, K, dtype=BF, device=DEV).t(), Bt, M, N, K),
        "Bt not contiguous":
            (At, torch.ones(K, 2 * N, dtype=BF, device=DEV)[:, ::2], M, N,
             K),
        "At too small": (At, Bt, M + 16, N, K),
        "Bt too large": (At, Bt, M, N - 16, K),
        "K mismatch": (At, Bt, M, N, K + 64),
        "M = 0": (At[:, :0].contiguous(), Bt, 0, N, K),
        "N < 0": (At, Bt, M, -N, K),
        "At fp32": (At.float(), Bt, M, N, K),
        "Bt on cpu": (At, Bt.cpu(), M, N, K),
        "M % 16 != 0": (At[:, :24].contiguous(), Bt, 24, N, K),
        "K < 1024": (At[:512], Bt[:512], M, N, 512),
    }
    for what, args in bad.items():
        with pytest.raises(RuntimeError):
            o.gemm_wgrad_bf16(*args)
            pytest.fail(f"gemm_wgrad_bf16: {what} did not raise")


def test_route_binding_raises_on_bad_arguments():
    o = ops()
    for args in [(0, 1, 1, 0, 0, False, 0, False),
                 (1, 1, 1, 2, 0, False, 0, False),
                 (1, 1, 1, 0, 0, False, 3, False),
                 (1 << 31, 1, 1, 0, 0, False, 0, False)]:
        with pytest.raises(RuntimeError):
            o.gemm_bf16_route(*args)
