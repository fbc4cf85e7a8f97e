"""Direct parity tests for the dense-NN support kernels (nn_kernels.hip):
act_backward, colsum, to_bf16, dense_adam, dense_adagrad and the
degenerate-GEMM fast paths (gemv_n1, wrowsum_m1, outer_k1, small_wgrad)
reached through gemm_bf16 / gemm_bf16_full with the argument patterns
models/mlp.py uses.

Oracles, shared inputs and the tolerance rule are in ``kernel_oracles.py``;
every bound is derived there, none is measured.
"""

import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def poison(shape, dtype):
    ko.poison(shape, dtype, DEV)


# ---------------------------------------------------------------------------
# act_backward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2])
def test_act_backward(act):
    """act 0/1 are selections (bit-exact); relu's gradient is 0 at
    Y == +0.0 and Y == -0.0 because the kernel tests Y > 0. Sigmoid is a
    three-rounding chain. dZbf is the exact bf16 of the dZ returned."""
    for n in (1, 255, 256, 257, 1025):
        g = torch.Generator().manual_seed(40 + n + act)
        dY = torch.randn(n, generator=g)
        if act == 2:
            Y = torch.rand(n, generator=g) * 0.98 + 0.01
        else:
            Y = torch.randn(n, generator=g)
            Y[0] = 0.0
            Y[n // 2] = -0.0
            Y[n - 1] = 0.0 if n % 2 else -0.0
            dY[0] = 1.5  # a non-zero gradient sits on every zero of Y
        ref, bound = ko.act_backward_ref(dY, Y, act)
        a, b = dY.to(DEV), Y.to(DEV)
        poison((n,), torch.float32)
        dZ, dZbf = ops().act_backward(a, b, act)
        if bound is None:
            ko.check_bits(f"act_backward.act{act}", dZ, ref)
            if act == 1:
                assert (dZ.cpu()[Y == 0] == 0).all()
        else:
            ko.check_bound("act_backward.sigmoid", dZ, ref, bound)
        ko.check_bits("act_backward.dZbf", dZbf, dZ.cpu().to(BF))


# ---------------------------------------------------------------------------
# colsum
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 255, 256, 257, 624])
def test_colsum_column_tiled(N):
    """db[n] = sum_m dZ[m,n], entries in [0.5, 1.5], at M 2^-23 sum|dZ|.
    M covers the 4-way unroll tail and the row-chunk split
    ychunks = min(2048/xtiles, ceil(M/128))."""
    for M in (1, 3, 4, 5, 127, 128, 129, 385, 1000):
        dZ = ko.unit_matrix(M, N, seed=M * 7 + N)
        ref, bound = ko.colsum_ref(dZ)
        x = dZ.to(DEV)
        poison((N,), torch.float32)
        ko.check_bound("colsum.tiled", ops().colsum(x), ref, bound)


def test_colsum_flat_n1():
    """The N == 1 path: 512 x 256 threads, so M = 131073 puts exactly one
    element into a second grid-stride trip. That element is scaled up
    (colsum_flat_scale) so that losing it exceeds the bound."""
    for M in (1, 63, 64, 65, 131072, 131073):
        dZ = ko.unit_matrix(M, 1, seed=M, last_row_scale=ko.colsum_flat_scale(M))
        ref, bound = ko.colsum_ref(dZ)
        x = dZ.to(DEV)
        poison((1,), torch.float32)
        ko.check_bound("colsum.flat", ops().colsum(x), ref, bound)


@pytest.mark.parametrize("shape", [(129, 257), (1000, 1)])
def test_colsum_all_zero_is_exact_zero(shape):
    """An all-zero input skips every atomic; the launcher's memset alone
    must leave exactly 0 in a poisoned output block."""
    x = torch.zeros(*shape, device=DEV)
    poison((shape[1],), torch.float32)
    ko.check_bits("colsum.zero", ops().colsum(x), torch.zeros(shape[1]))


# ---------------------------------------------------------------------------
# to_bf16
# ---------------------------------------------------------------------------
def test_to_bf16_round_to_nearest_even():
    """Bit-exact against torch's RNE conversion around the x4 vector body
    and its scalar tail; values that round up into the next binade, ties
    to even in both directions, +-0 and +-inf lead every input."""
    special = torch.tensor([
        1.99609375,              # tie below 2.0: to even, up into 2.0
        1.998046875,             # above that tie: rounds up to 2.0
        1.0 + 2.0 ** -8,         # tie to even: down to 1.0
        1.0 + 3 * 2.0 ** -8,     # tie to even: up to 1.015625
        -(1.0 + 2.0 ** -8), 0.0, -0.0, float("inf"), float("-inf"),
        3.3895313892515355e38,   # largest finite bf16
        3.4028234663852886e38,   # largest fp32: rounds up to +inf
    ])
    for n in (1, 3, 4, 5, 1023, 1024, 1025, 4099):
        g = torch.Generator().manual_seed(n)
        x = torch.randn(n, generator=g) * 3
        k = min(n, special.numel())
        x[:k] = special[:k]
        x[n - 1] = special[(n - 1) % special.numel()]
        xd = x.to(DEV)
        poison((n,), BF)
        ko.check_bits("to_bf16", ops().to_bf16(xd), x.to(BF))


# ---------------------------------------------------------------------------
# dense optimizers
# ---------------------------------------------------------------------------
def _mirrors(W):
    if W.dim() == 1:
        return None, None
    return (torch.zeros(W.shape, dtype=BF, device=DEV),
            torch.zeros(W.shape[1], W.shape[0], dtype=BF, device=DEV))


def _check_mirrors(name, Wd, Wbf, Wtbf):
    if Wbf is None:
        return
    W = Wd.cpu()
    ko.check_bits(name + ".Wbf", Wbf, W.to(BF))
    ko.check_bits(name + ".Wtbf", Wtbf, ko.transposed_mirror(W))


DENSE_CASES = ko.DENSE_SHAPES + [(17,)]  # 1-D: the bias form, no mirrors


def _seed(shape):
    return 31 * sum(shape) + len(shape)


@pytest.mark.parametrize("shape", DENSE_CASES, ids=str)
@pytest.mark.parametrize("scale", [1.0, 1e-6])
@pytest.mark.parametrize("l2", [0.0, 1e-3])
def test_dense_adam(shape, scale, l2):
    """Steps 1, 2 and 1000, 1001: two consecutive Adam calls from zero
    state, so the second of each pair runs on non-zero m and v. W, m, v
    against adam_ref computed from the state the GPU held before each
    call, then both bf16 mirrors against the W that call produced. At
    |g| ~ 1e-6, eps = 1e-8 is a percent of the denominator."""
    for step0 in (1, 1000):
        W0, grad = ko.dense_inputs(shape, scale, seed=_seed(shape))
        W = W0.to(DEV)
        m = torch.zeros_like(W)
        v = torch.zeros_like(W)
        Wbf, Wtbf = _mirrors(W)
        for i, step in enumerate((step0, step0 + 1)):
            gr = grad if i == 0 else -0.5 * grad + 0.25 * scale
            ref = ko.adam_ref(W.cpu(), gr, m.cpu(), v.cpu(), step=step,
                              l2=l2, **ko.ADAM)
            ops().dense_adam(W, gr.to(DEV), m, v, Wbf, Wtbf, ko.ADAM["lr"],
                             ko.ADAM["beta1"], ko.ADAM["beta2"],
                             ko.ADAM["eps"], step, l2)
            ko.check_bound("dense_adam.m", m, *ref["m"])
            ko.check_bound("dense_adam.v", v, *ref["v"])
            ko.check_bound("dense_adam.W", W, *ref["W"])
            _check_mirrors("dense_adam", W, Wbf, Wtbf)


@pytest.mark.parametrize("shape", DENSE_CASES, ids=str)
@pytest.mark.parametrize("scale", [1.0, 1e-4])
@pytest.mark.parametrize("l2", [0.0, 1e-3])
def test_dense_adagrad(shape, scale, l2):
    """Two consecutive Adagrad calls: W and n against adagrad_ref from the
    state the GPU held before each call, then both mirrors. At |g| ~ 1e-4,
    g^2 and eps = 1e-8 are the same size, so eps on the wrong side of the
    square root moves the update by tens of percent."""
    W0, grad = ko.dense_inputs(shape, scale, seed=_seed(shape) + 1)
    W = W0.to(DEV)
    n = torch.zeros_like(W)
    Wbf, Wtbf = _mirrors(W)
    for i in range(2):
        gr = grad if i == 0 else -0.5 * grad + 0.25 * scale
        ref = ko.adagrad_ref(W.cpu(), gr, n.cpu(), l2=l2, **ko.ADAGRAD)
        ops().dense_adagrad(W, gr.to(DEV), n, Wbf, Wtbf, ko.ADAGRAD["lr"],
                            ko.ADAGRAD["eps"], l2)
        ko.check_bound("dense_adagrad.n", n, *ref["n"])
        ko.check_bound("dense_adagrad.W", W, *ref["W"])
        _check_mirrors("dense_adagrad", W, Wbf, Wtbf)


# ---------------------------------------------------------------------------
# degenerate GEMM fast paths
# ---------------------------------------------------------------------------
def _bf(x):
    return x.to(BF).to(DEV)


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("with_bias", [False, True])
def test_gemv_n1(act, with_bias):
    """Forward of a 1-wide layer, C[M,1] = act(X[M,K] w[1,K]^T + b), as
    DenseLayer.forward_gpu calls it (N=1, transA=0 routes to gemv_n1).
    Bound: K 2^-23 sum|x w| through the epilogue (gemm_epilogue_ref); Cbf
    is the exact bf16 of C. For act 1/2 the weights are signed and scaled
    by 2/K so the pre-activation stays where the activation has slope."""
    for M in (1, 3, 4, 5, 257):
        for K in (1, 63, 64, 65, 130):
            X = ko.bf16_values((M, K), seed=M * 131 + K)
            w = ko.bf16_values((1, K), seed=K, signed=act != 0,
                               scale=1.0 if act == 0 else 2.0 / K)
            bias = torch.tensor([0.375]) if with_bias else None
            s, sb = ko.gemm_sum_ref(X, w)
            ref, bound = ko.gemm_epilogue_ref(s, sb, bias, act)
            bd = bias.to(DEV) if with_bias else None
            poison((M, 1), torch.float32)
            C, Cbf = ops().gemm_bf16_full(_bf(X), _bf(w), bd, M, 1, K, 0, 0,
                                          act)
            ko.check_bound(f"gemv_n1.act{act}", C, ref, bound)
            ko.check_bits("gemv_n1.Cbf", Cbf, C.cpu().to(BF))


@pytest.mark.parametrize("N", [2, 255, 256, 257])
def test_wrowsum_m1(N):
    """wgrad of a 1-wide layer, dW[1,N] = dZ[K,1]^T X[K,N], as
    DenseLayer.backward_gpu calls it (M=1, transA=transB=1, no bias, act or
    Cbf routes to wrowsum_m1). K covers the 4-way unroll tail and the
    K-chunk split."""
    for K in (1, 3, 4, 5, 127, 128, 129, 1000):
        dZ = ko.bf16_values((K, 1), seed=K * 3 + N)
        X = ko.bf16_values((K, N), seed=K * 5 + N)
        ref, bound = ko.gemm_sum_ref(dZ.t(), X.t())
        poison((1, N), torch.float32)
        C = ops().gemm_bf16(_bf(dZ), _bf(X), None, 1, N, K, 1, 1, 0, False)
        ko.check_bound("wrowsum_m1", C, ref, bound)


@pytest.mark.parametrize("act", [0, 1, 2])
def test_outer_k1(act):
    """K=1, transA=0, N>1 routes to outer_k1: C[m,n] = act(a[m] b[n] +
    bias[n]), one exact product, one rounding for the bias add. Without
    bias and activation the product is exact."""
    for M, N in ((1, 2), (3, 85), (257, 3)):
        a = ko.bf16_values((M, 1), seed=M, signed=True)
        b = ko.bf16_values((N, 1), seed=N + 1, signed=True)
        bias = ko.bf16_values((N,), seed=N + 2, signed=True) * 0.3
        s, _ = ko.gemm_sum_ref(a, b)
        ref, bound = ko.gemm_epilogue_ref(s, torch.zeros_like(s), bias, act)
        C, Cbf = ops().gemm_bf16_full(_bf(a), _bf(b), bias.to(DEV), M, N, 1,
                                      0, 0, act)
        ko.check_bound(f"outer_k1.act{act}", C, ref, bound)
        ko.check_bits("outer_k1.Cbf", Cbf, C.cpu().to(BF))
        if act == 0:
            # dgrad pattern of the 1-wide layer: no bias, no mirror, exact
            C0 = ops().gemm_bf16(_bf(a), _bf(b), None, M, N, 1, 0, 0, 0,
                                 False)
            ko.check_bits("outer_k1.exact", C0, s.float())


SMALL_WGRAD_SHAPES = [(63, 65, 8192), (64, 15, 8193), (3, 5, 16384),
                      (2, 2048, 8192)]


@pytest.mark.parametrize("M,N,K", SMALL_WGRAD_SHAPES)
def test_small_wgrad_kernel_is_reached(M, N, K):
    """dW[M,N] = dZ[K,M]^T X[K,N] with M or N not a multiple of 16.

    Routing in gemm_bf16_launch, in order: gemv_n1 wants N == 1 and
    transA == 0; wrowsum_m1 wants M == 1; the wgrad128 kernel is tried
    next and takes ``transA == 1 && transB == 1 && M % 16 == 0 &&
    N % 16 == 0 && K >= 1024`` (gemm_wgrad_eligible), which every shape
    here fails on M or N; small_wgrad then takes ``transA == 1 &&
    transB == 1 && M * N <= 4096 && K >= 8192 && no bias/act/Cbf``.
    63*65 = 4095 and 2*2048 = 4096 give threads four outputs each;
    K = 8193 makes the per-block K chunk 17, so the trailing blocks of the
    512 are empty. Bound K 2^-23 sum|a b|; at K >= 8192 that is ~K^2 2^-23
    for unit entries, so the last k row of both operands is scaled by 16
    to keep the loss of that row above it."""
    assert M % 16 or N % 16
    assert M * N <= 4096 and K >= 8192
    dZ = ko.unit_matrix(K, M, seed=K + M, last_row_scale=16.0).to(BF).float()
    X = ko.unit_matrix(K, N, seed=K + N + 1, last_row_scale=16.0).to(BF).float()
    ref, bound = ko.gemm_sum_ref(dZ.t(), X.t())
    poison((M, N), torch.float32)
    C = ops().gemm_bf16(_bf(dZ), _bf(X), None, M, N, K, 1, 1, 0, False)
    ko.check_bound("small_wgrad", C, ref, bound)
