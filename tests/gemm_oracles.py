"""References, input builders, case lists, bounds and wrong references for
the dense-engine (MFMA bf16 GEMM) parity tests.

Plain helper module (imported like ``ffm_oracles``). Everything here runs
on the CPU; ``test_gemm_kernels_gpu.py`` uploads the inputs and brings the
outputs back, ``test_gemm_oracles.py`` holds the reference to the project's
CPU path and shows that the wrong references below differ on the very
inputs the GPU tests use.

The operation: ``C[m,n] = act(sum_k opA[m,k] opB[n,k] + bias[n])`` with A
stored [M,K] (transA = 0) or [K,M] (transA = 1) and B stored [N,K]
(transB = 0) or [K,N] (transB = 1); ``Cbf = bf16(C)``.

Exact set. bf16 x bf16 products are exact in fp32 and accumulate in fp32.
With integer operands |a| <= amax, |b| <= bmax and an integer bias every
product, every partial sum in any order and the biased total is an integer
of magnitude at most ``K amax bmax + biasmax``; below 2^24 all of them are
representable, so any tile order, MFMA chaining or split-K atomic order
gives the integer result exactly and the comparison is bit for bit
(``assert_exact`` is called for every generated case). relu is a
selection. Only the sigmoid epilogue rounds; it is held to the short-chain
bound of ``kernel_oracles.gemm_epilogue_ref`` with a zero sum bound.

Float set. bf16 of 0.5 N(0,1): sum rule ``|C - ref64| <= K 2^-23 sum|a b|``
plus the same epilogue chain.

Every set: ``Cbf`` equals ``C.to(bfloat16)`` of the same call bit for bit.
"""

from __future__ import annotations

import torch

import kernel_oracles as ko

BF = torch.bfloat16
OP_MAX = 3      # operands are integers in {-3..3}
BIAS_MAX = 8    # bias integers in {-8..8}
PAD = 64        # NaN elements on either side of an operand view
LAYOUTS = ((0, 0), (1, 0), (0, 1), (1, 1))

# tile constants of the sources (checked against the .hip files by
# test_gemm_oracles.py::test_tile_constants_match_sources)
TILE = {"GEMM_BM": 128, "GEMM_BN": 128, "GEMM_BK": 64, "G256_BK": 64,
        "P8_BK": 64, "V2_CK": 32, "GN128_BK": 64, "WG_BM": 128,
        "WG_BN": 128, "WG_BK": 64}


# ---------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------
def assert_exact(K, amax=OP_MAX, bmax=OP_MAX, biasmax=BIAS_MAX):
    """every partial sum and the biased total is an integer below 2^24"""
    assert K * amax * bmax + biasmax < 2 ** 24, (K, amax, bmax, biasmax)


def split_chunk(K, split_z, bk=64):
    """K range per z-block for a requested fan-out (both split-K
    launchers): ceil(K / split_z) rounded up to whole K-tiles"""
    return ((K + split_z - 1) // split_z + bk - 1) // bk * bk


def split_blocks(K, split_z, bk=64):
    """z-blocks actually launched"""
    c = split_chunk(K, split_z, bk)
    return (K + c - 1) // c


# ---------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------
_EINSUM = {(0, 0): "mk,nk->mn", (1, 0): "km,nk->mn",
           (0, 1): "mk,kn->mn", (1, 1): "km,kn->mn"}


def act_ref(z, act):
    if act == 1:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == 2:
        return torch.sigmoid(z.clamp(-16, 16))
    return z


def gemm_ref(A, B, transA, transB, bias=None, act=0):
    """float64 act(sum_k opA[m,k] opB[n,k] + bias[n]) from the operands as
    stored, index by index from the definition. On the exact set every
    value is an integer far below 2^53, so float64 is exact too.
    Returns (C, z) with z the pre-activation value."""
    z = torch.einsum(_EINSUM[(transA, transB)], A.double(), B.double())
    if bias is not None:
        z = z + bias.double()
    z = z + 0.0  # -0 -> +0: an fp32 accumulator that starts at +0 never
    #              ends at -0 under round-to-nearest
    return act_ref(z, act), z


def sum_bound(A, B, transA, transB):
    """K 2^-23 sum_k |a b| (the sum rule of kernel_oracles, n = K)"""
    K = A.shape[0] if transA else A.shape[1]
    mag = torch.einsum(_EINSUM[(transA, transB)], A.double().abs(),
                       B.double().abs())
    return K * ko.U23 * mag


def epilogue_bound(s, sbound, bias, act):
    """(ref64, bound) of act(s + bias) from the sum and its bound: the
    chain derived in kernel_oracles.gemm_epilogue_ref"""
    return ko.gemm_epilogue_ref(s, sbound, bias, act)


def logical(A, B, transA, transB):
    """operands as [M,K] and [N,K] float64, whatever the storage"""
    a = A.double().t() if transA else A.double()
    b = B.double().t() if transB else B.double()
    return a, b


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def case_seed(M, N, K, transA, transB, salt=0):
    return (((M * 1009 + N) * 1013 + K) * 4 + transA * 2 + transB) * 7 + salt


def _store(a, b, transA, transB):
    A = a.t().contiguous() if transA else a.contiguous()
    B = b.t().contiguous() if transB else b.contiguous()
    return A, B


def exact_operands(M, N, K, transA=0, transB=0, fill="random", salt=0):
    """(A, B, bias) as stored, fp32 holding integers: operands in {-3..3},
    bias in {-8..8}, seeded per shape and layout so that transposes, tile
    swaps and swizzle slips show. Column k = K-1 is nowhere zero (zeros
    there become 1), so that losing the last k shows in every row.
    fill 'lastk': only column k = K-1 is non-zero (and nowhere zero);
    fill 'tilefirst': only the first k of each 64-wide K tile."""
    assert_exact(K)
    g = torch.Generator().manual_seed(case_seed(M, N, K, transA, transB,
                                                salt))
    a = torch.randint(-OP_MAX, OP_MAX + 1, (M, K), generator=g).float()
    b = torch.randint(-OP_MAX, OP_MAX + 1, (N, K), generator=g).float()
    bias = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (N,), generator=g).float()
    for t in (a, b):
        t[:, K - 1][t[:, K - 1] == 0] = 1.0
    if fill != "random":
        keep = torch.zeros(K, dtype=torch.bool)
        if fill == "lastk":
            keep[K - 1] = True
        elif fill == "tilefirst":
            keep[::64] = True
        else:
            raise ValueError(fill)
        for t in (a, b):
            t[t == 0] = 1.0
            t[:, ~keep] = 0.0
    A, B = _store(a, b, transA, transB)
    return A, B, bias


def float_operands(M, N, K, transA=0, transB=0, lastk_scale=1.0, salt=0):
    """(A, B, bias) as stored, fp32 holding bf16 values of 0.5 N(0,1); the
    last k column of both operands optionally scaled (a power of two) so
    that losing it stays above the K 2^-23 sum|a b| bound at deep K"""
    g = torch.Generator().manual_seed(case_seed(M, N, K, transA, transB,
                                                salt + 1))
    a = torch.randn(M, K, generator=g) * 0.5
    b = torch.randn(N, K, generator=g) * 0.5
    a[:, -1] *= lastk_scale
    b[:, -1] *= lastk_scale
    bias = torch.randn(N, generator=g)
    A, B = _store(a.to(BF).float(), b.to(BF).float(), transA, transB)
    return A, B, bias


def lastk_scale_for(K):
    """smallest power of two s such that a last-column term (0.5 s)^2 of
    typical size exceeds K 2^-23 (0.25 K + 0.25 s^2), the typical sum
    bound: 1 up to K ~ 1400, then growing like K"""
    s = 1.0
    while 0.25 * s * s <= 4 * K * ko.U23 * (0.25 * K + 0.25 * s * s):
        s *= 2.0
    return s


def embed(t, device, misalign=False):
    """Upload a stored operand as a bf16 view inside a larger NaN-filled
    buffer: a read past a row, a tile or the end that reaches an MFMA gives
    NaN, not silence. The view starts PAD elements (128 bytes) into the
    buffer, 16-byte-aligned; with misalign one element (two bytes) later.
    Returns (view, buffer); keep the buffer alive."""
    n = t.numel()
    off = PAD + (1 if misalign else 0)
    buf = torch.full((n + 2 * PAD + 8,), float("nan"), dtype=BF,
                     device=device)
    view = buf[off:off + n].view(t.shape)
    view.copy_(t.to(BF))
    assert view.is_contiguous()
    assert (view.data_ptr() % 16 == 0) != misalign
    return view, buf


# ---------------------------------------------------------------------------
# case lists (shared by the GPU tests and the CPU mutation tests)
# ---------------------------------------------------------------------------
def _uniq(xs):
    out = []
    for x in xs:
        if x not in out:
            out.append(x)
    return out


# the issue's lists plus the +-8 neighbours of the 128 / 64 tile edges
GENERIC_MN = [1, 15, 16, 17, 63, 64, 65, 120, 127, 128, 129, 136, 257]
GENERIC_K = [1, 7, 8, 9, 31, 32, 33, 56, 63, 64, 65, 72, 120, 127, 128, 129,
             136, 200]
GENERIC_CENTRE = (129, 129, 72)   # one full (glds) tile and an edge tile
#                                   per operand, one full K tile and a tail


def generic_cases():
    """(M, N, K), one axis at a time around the centre"""
    cM, cN, cK = GENERIC_CENTRE
    return _uniq([(m, cN, cK) for m in GENERIC_MN] +
                 [(cM, n, cK) for n in GENERIC_MN] +
                 [(cM, cN, k) for k in GENERIC_K])


# (K, requested fan-out): K % 64 == 0 with one tile per block; last chunk
# short (3 x 1088 + 896); the K tail inside the last chunk (7 x 576 + 65);
# fewer blocks than requested (kchunk 128 -> 33 of 64); default fan-out
SPLITK_CASES = [(4096, 64), (4160, 4), (4097, 8), (4104, 64), (4097, 64),
                (4160, 64)]
SPLITK_MN = (129, 65)

G256_K = [32, 40, 56, 64, 72, 120, 128, 136, 192, 200, 264]
G256_GRIDS = [(1, 1), (1, 3), (3, 1), (2, 2)]      # tiles of 256, (my, nx)
G256_GRID_K = [136, 192]                            # K for the grid sweep
G256_VARIANTS = [f"gemm256_p{p}_b{b}" for p in (0, 1, 2) for b in (0, 1)]

P8_VARIANTS = ["p8_lite", "p8_lite_xcd", "p8_full", "p8_full_xcd",
               "p8_lite_apipe"]
P8_GRIDS = [(1, 1), (1, 2), (3, 5), (4, 4)]


def tile256_cases(grids, ks=G256_K, grid_ks=G256_GRID_K):
    """(M, N, K): every K on one tile, every grid at a tail K and a
    three-tile K"""
    return _uniq([(256, 256, k) for k in ks] +
                 [(256 * gy, 256 * gx, k) for gy, gx in grids
                  for k in grid_ks])


def g256_variant_ok(variant, K):
    """pipe 2 (branch-free staging) exists for K % 64 == 0 only"""
    return not (variant.startswith("gemm256_p2") and K % 64)


V2_CASES = [(256 * gy, 256 * gx, k) for gy, gx in [(1, 1), (2, 3)]
            for k in (192, 256, 320, 448)]

N128_CASES = [(m, n, k) for m in (256, 512)
              for n in (128, 129, 136, 200, 384, 624)
              for k in (64, 128, 192)]

WGRAD_MN = [16, 32, 112, 128, 144, 256, 272, 624]
WGRAD_K = [1024, 1025, 1032, 1055, 1056, 1057, 2040, 2047, 2048, 2049, 2056,
           4100]
WGRAD_CENTRE = (144, 272, 1057)
# explicit fan-outs whose last chunk is short: 4100 = 2 x 1408 + 1284,
# 2049 = 4 x 448 + 257, 1057 = 64 x 16 + 33 (kchunk 64 -> 17 blocks)
WGRAD_SPLITS = [(4100, 3), (2049, 5), (1057, 64), (1024, 1)]


def wgrad_cases():
    cM, cN, cK = WGRAD_CENTRE
    return _uniq([(m, cN, cK) for m in WGRAD_MN] +
                 [(cM, n, cK) for n in WGRAD_MN] +
                 [(cM, cN, k) for k in WGRAD_K])


# epilogues: (has_bias, act, emit_bf16), all twelve
EPILOGUES = [(hb, act, emit) for hb in (False, True) for act in (0, 1, 2)
             for emit in (False, True)]

# body -> [(variant, transA, transB, (M, N, K))]: one interior and one
# edge shape per body that has an epilogue
EPILOGUE_SHAPES = {
    "generic": [("generic", 0, 0, (128, 128, 64)),
                ("generic", 0, 0, (129, 65, 72)),
                ("generic", 1, 0, (129, 65, 72)),
                ("generic", 0, 1, (65, 129, 33)),
                ("generic", 1, 1, (17, 129, 65))],
    "gemm256": [("gemm256_p2_b0", 0, 0, (512, 512, 128)),
                ("gemm256_p0_b0", 0, 0, (256, 512, 72)),
                ("gemm256_p1_b1", 0, 0, (256, 256, 136))],
    "p8": [("p8_lite", 0, 0, (512, 512, 128)),
           ("p8_lite", 0, 0, (256, 512, 72)),
           ("p8_full", 0, 0, (256, 256, 136)),
           ("p8_lite_apipe", 0, 0, (256, 256, 72))],
    "v2": [("v2", 0, 0, (256, 256, 192)), ("v2", 0, 0, (512, 256, 320))],
    "n128": [("n128", 0, 0, (256, 128, 128)),
             ("n128", 0, 0, (256, 200, 192))],
}

# float set: body -> [(variant, transA, transB, split_z, (M, N, K))]
FLOAT_CASES = {
    "generic": [("generic", ta, tb, 0, s) for ta, tb in LAYOUTS
                for s in ((129, 129, 72), (65, 17, 200))] +
               [("generic", 0, 0, 64, (129, 65, 4097)),
                ("generic", 1, 1, 4, (129, 65, 4160))],
    "gemm256": [("gemm256_p2_b0", 0, 0, 0, (256, 256, 192)),
                ("gemm256_p0_b0", 0, 0, 0, (512, 256, 136)),
                ("gemm256_p1_b1", 0, 0, 0, (256, 512, 264))],
    "p8": [("p8_lite", 0, 0, 0, (256, 256, 136)),
           ("p8_lite", 0, 0, 0, (512, 512, 264)),
           ("p8_full_xcd", 0, 0, 0, (768, 1280, 200)),
           ("p8_lite_apipe", 0, 0, 0, (256, 512, 192))],
    "v2": [("v2", 0, 0, 0, (256, 256, 192)),
           ("v2", 0, 0, 0, (512, 768, 448))],
    "n128": [("n128", 0, 0, 0, (256, 128, 128)),
             ("n128", 0, 0, 0, (512, 624, 192))],
    "wgrad128": [("wgrad128", 1, 1, 0, (144, 272, 1057)),
                 ("wgrad128", 1, 1, 3, (128, 256, 4100)),
                 ("wgrad128", 1, 1, 64, (16, 624, 2049))],
}
FLOAT_EPILOGUES = [(True, 0, True), (True, 1, True), (True, 2, True)]


# ---------------------------------------------------------------------------
# wrong references (what a subtly broken kernel would compute); each
# returns the float64 C it would produce, from the operands as stored
# ---------------------------------------------------------------------------
def _from_logical(a, b, bias, act):
    z = a @ b.t()
    if bias is not None:
        z = z + bias.double()
    return act_ref(z + 0.0, act)


def wrong_dropk(A, B, transA, transB, bias=None, act=0):
    """the last k left out"""
    a, b = logical(A, B, transA, transB)
    return _from_logical(a[:, :-1], b[:, :-1], bias, act)


def tail_chunk_start(K):
    """first k of the last 8-element chunk (whole or partial)"""
    return (K - 1) // 8 * 8


def wrong_drop_tail_chunk(A, B, transA, transB, bias=None, act=0):
    """the last 8-element chunk of the K tail left out (a masked 16-byte
    load that masks one chunk too many)"""
    a, b = logical(A, B, transA, transB)
    k = tail_chunk_start(a.shape[1])
    return _from_logical(a[:, :k], b[:, :k], bias, act)


def wrong_tail_readthrough(A, B, bias=None, act=0):
    """row-major operands: the K tail of the last tile read through into
    the next row's first elements in place of zeros; past the last row the
    buffer holds NaN"""
    a, b = A.double(), B.double()
    K = a.shape[1]
    pad = (-K) % 64
    assert pad, "needs a K tail"
    def through(x):
        flat = torch.cat([x.reshape(-1),
                          torch.full((pad,), float("nan"),
                                     dtype=torch.float64)])
        idx = (torch.arange(x.shape[0]).unsqueeze(1) * K
               + torch.arange(K + pad).unsqueeze(0))
        return flat[idx]
    return _from_logical(through(a), through(b), bias, act)


def wrong_b_layout(A, B, transA, transB, bias=None, act=0):
    """Bst's buffer indexed as the other layout ([K,N] for [N,K] and the
    reverse)"""
    a, _ = logical(A, B, transA, transB)
    N, K = (B.shape[1], B.shape[0]) if transB else B.shape
    flat = B.double().reshape(-1)
    b = flat.view(N, K) if transB else flat.view(K, N).t()
    return _from_logical(a, b, bias, act)


def wrong_swap_halves(A, B, transA, transB, bias=None, act=0):
    """the two 128-row halves of every complete 256-row A tile swapped"""
    a, b = logical(A, B, transA, transB)
    M = a.shape[0]
    assert M >= 256
    a = a.clone()
    for m0 in range(0, M - 255, 256):
        top = a[m0:m0 + 128].clone()
        a[m0:m0 + 128] = a[m0 + 128:m0 + 256]
        a[m0 + 128:m0 + 256] = top
    return _from_logical(a, b, bias, act)


def wrong_stale_tile(A, B, transA, transB, bias=None, act=0, bk=64):
    """the last K tile computed from the previous tile's data (a slot that
    was not refilled)"""
    a, b = logical(A, B, transA, transB)
    K = a.shape[1]
    k0 = (K - 1) // bk * bk
    assert k0 >= bk, "needs two K tiles"
    a, b = a.clone(), b.clone()
    a[:, k0:] = a[:, k0 - bk:K - bk]
    b[:, k0:] = b[:, k0 - bk:K - bk]
    return _from_logical(a, b, bias, act)


def wrong_bias_per_chunk(A, B, transA, transB, bias, nblocks, act=0):
    """bias added once per split-K block"""
    a, b = logical(A, B, transA, transB)
    return act_ref(a @ b.t() + nblocks * bias.double(), act)


def wrong_relu_vs_bias(A, B, transA, transB, bias):
    """relu that keeps z where z > bias, not where z > 0"""
    a, b = logical(A, B, transA, transB)
    z = a @ b.t() + bias.double()
    return torch.where(z > bias.double(), z, torch.zeros_like(z))


def wrong_cbf_preact(A, B, transA, transB, bias, act):
    """the bf16 mirror taken from the pre-activation value"""
    _, z = gemm_ref(A, B, transA, transB, bias, 0)
    return z.float().to(BF)
