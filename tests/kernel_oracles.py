"""float64 oracles, CSR builders, shared inputs and derived tolerances for
the Wide&Deep / NFM / MLP step-kernel parity tests.

Plain helper module (imported like ``gbm_forest_util``). Everything here
runs on the CPU; the GPU tests move the inputs to ``cuda:0`` and bring the
kernel outputs back. The same input builders feed ``test_kernel_oracles.py``
(CPU), which shows that every bound used on the GPU is smaller than the
effect of the kernel mistakes it is meant to catch.

Tolerance rule (u = 2^-24 is the fp32 unit roundoff, 2^-23 one ulp of 1):

* bit-exact: an output that is one fp32 multiply, a selection, or a
  round-to-nearest-even bf16 conversion is compared bit for bit with the
  same expression evaluated in fp32 on the CPU.
* sums: n once-rounded fp32 terms accumulated in any order obey
  ``|out - ref64| <= n * 2^-23 * sum|term_i|`` (first-order worst case is
  ``n * u * sum|term|``: u per term for its own rounding plus (n-1) u for
  the additions; the rule keeps a factor 2 over that). bf16 x bf16
  products are exact in fp32, so GEMM sums use it with n = K.
* short chains: every fp32 rounding contributes u times the magnitude of
  the value it rounds; the bound is the first-order propagation of those
  through the chain, with absolute values taken at every addition so that
  cancellation cannot shrink it. FMA contraction only removes roundings.
  A result subtracted from a stored weight adds one ulp of that weight.
"""

from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np
import torch

U23 = 2.0 ** -23
U24 = 2.0 ** -24
EMBED_KS = (4, 8, 16, 32, 64)
F_TABLE = 4096

# ---------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------
def check_bound(name, out, ref64, bound):
    """assert |out - ref64| <= bound elementwise; a zero bound means exact.
    Prints the largest err/bound (the figures quoted in docs/TESTING.md,
    information only)."""
    out64 = out.detach().cpu().double().reshape(ref64.shape)
    bound = bound.reshape(ref64.shape)
    assert torch.isfinite(out64).all(), f"{name}: non-finite output"
    err = (out64 - ref64).abs()
    pos = bound > 0
    ratio = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"RATIO {name} {ratio:.4f}")
    bad = err > bound
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the "
        f"bound, worst err/bound {ratio:.3g}, max err {float(err.max()):.3g}")


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_bits(name, out, expect):
    """bit-for-bit equality (distinguishes +-0, catches NaN payloads)."""
    out = out.detach().cpu()
    assert out.dtype == expect.dtype, (name, out.dtype, expect.dtype)
    assert out.shape == expect.shape, (name, out.shape, expect.shape)
    ne = _bits(out) != _bits(expect)
    assert not ne.any(), (
        f"{name}: {int(ne.sum())} of {ne.numel()} elements differ bitwise, "
        f"first at flat index {int(ne.flatten().nonzero()[0])}")


def differs(a, b, bound=None):
    """True when two references differ (by more than bound, if given) in at
    least one element. NaN against a number counts as a difference."""
    a, b = a.double(), b.double()
    d = (a - b).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    if bound is None:
        return bool((d > 0).any())
    return bool((d > bound.reshape(d.shape)).any())


def f32(x):
    """the value a double scalar takes when a binding casts it to float"""
    return float(np.float32(x))


def poison(shape, dtype, device):
    """Fill a block of an op's exact output shape with NaN and free it, so
    that the caching allocator hands the same block to the op's at::empty
    and anything the kernel leaves unwritten reads NaN. Upload the op's
    inputs first and do not call empty_cache in between."""
    p = torch.full(shape, float("nan"), dtype=dtype, device=device)
    torch.cuda.synchronize()
    del p


# ---------------------------------------------------------------------------
# CSR builders
# ---------------------------------------------------------------------------
def length_set(K, wide=False):
    """Row lengths from the kernels' loop structure: G = 64/K entries per
    trip, 4 trips unrolled; 39 is the Criteo width; the wide kernel
    lane-strides by 64. Empty rows first, in the middle and last."""
    G = 64 // K
    ls = [1, G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1, 8 * G + 1, 39]
    if wide:
        ls += [63, 64, 65, 130]
    seen = []
    for n in ls:
        if n > 0 and n not in seen:
            seen.append(n)
    mid = len(seen) // 2
    return [0] + seen[:mid] + [0] + seen[mid:] + [0]


def batch_lengths(K, B):
    """First B of a fixed mix of empty / short / unroll-edge / long rows,
    for the rows-per-block sweep (a block holds 4 rows)."""
    G = 64 // K
    mix = [G + 1, 0, 39, 4 * G + 1, 1, 8 * G + 1, 0, G, 45]
    return mix[:B]


BATCHES = (1, 3, 4, 5, 9)  # a block holds 4 rows


def length_cases(K, wide=False, base=0):
    """(lengths, seed) pairs: the full length set, then the rows-per-block
    sweep. `base` separates the seeds of the tests that share this."""
    yield length_set(K, wide=wide), base + 10 + K
    for B in BATCHES:
        yield batch_lengths(K, B), base + 100 * B + K


def make_csr(lengths, F=F_TABLE, seed=0, dup_row=None):
    """(row_ptr i32, fids i32, vals f32) with vals uniform in [0.5, 1.5].
    dup_row: that row's second entry repeats the fid of its first."""
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor(lengths, dtype=torch.int64)
    nnz = int(counts.sum())
    row_ptr = torch.zeros(len(lengths) + 1, dtype=torch.int32)
    row_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    fids = torch.randint(0, F, (nnz,), generator=g, dtype=torch.int32)
    vals = 0.5 + torch.rand(nnz, generator=g)
    if dup_row is not None:
        b = int(row_ptr[dup_row])
        assert lengths[dup_row] >= 2
        fids[b + 1] = fids[b]
    return row_ptr, fids, vals


def rows_pos(row_ptr):
    """entry -> (row index, position in row, row lengths), all int64"""
    rp = row_ptr.long()
    counts = rp[1:] - rp[:-1]
    B = counts.numel()
    row = torch.repeat_interleave(torch.arange(B), counts)
    pos = torch.arange(int(rp[-1])) - rp[:-1][row]
    return row, pos, counts


def drop_last_entry(row_ptr, fids, vals, r):
    """the CSR with the last entry of row r removed (mutant input)"""
    rp = row_ptr.long()
    j = int(rp[r + 1]) - 1
    assert j >= int(rp[r])
    keep = torch.ones(fids.numel(), dtype=torch.bool)
    keep[j] = False
    rp2 = row_ptr.clone()
    rp2[r + 1:] -= 1
    return rp2, fids[keep], vals[keep]


def table(F, K, seed):
    g = torch.Generator().manual_seed(seed)
    if K == 0:
        return torch.randn(F, generator=g) * 0.1
    return torch.randn(F, K, generator=g) * 0.1


# ---------------------------------------------------------------------------
# embedding / NFM oracles
# ---------------------------------------------------------------------------
def wide_forward_ref(row_ptr, fids, vals, W):
    """wide[row] = sum_j W[fid_j] x_j in float64, with the sum bound
    n * 2^-23 * sum|w x| (n = row length; empty rows: exactly 0)."""
    row, _, counts = rows_pos(row_ptr)
    t = W.double()[fids.long()] * vals.double()
    B = counts.numel()
    ref = torch.zeros(B, dtype=torch.float64).index_add_(0, row, t)
    mag = torch.zeros(B, dtype=torch.float64).index_add_(0, row, t.abs())
    return ref, counts.double() * U23 * mag


def embed_gather_expect(row_ptr, fids, vals, E, nf, mutant=None):
    """out[row, pos*K+k] = bf16(E[fid,k] * x) for pos < min(len, nf), zero
    for len <= pos < nf; entries at pos >= nf are ignored. The product is
    one fp32 multiply, so the result is bit-exact.
    mutants: 'pos+1' reads the next entry, 'nopad' leaves the padding
    unwritten (NaN stands for whatever the allocator held)."""
    row, pos, counts = rows_pos(row_ptr)
    B, K = counts.numel(), E.shape[1]
    src = torch.arange(fids.numel())
    if mutant == "pos+1":
        src = (src + 1).clamp(max=max(fids.numel() - 1, 0))
    prod = E[fids.long()[src]] * vals[src].unsqueeze(1)
    fill = float("nan") if mutant == "nopad" else 0.0
    out = torch.full((B, nf, K), fill)
    keep = pos < nf
    out[row[keep], pos[keep]] = prod[keep]
    return out.view(B, nf * K).to(torch.bfloat16)


def embed_backward_emit_expect(row_ptr, vals, dOut, dwide, nf, K,
                               mutant=None):
    """gv[j,k] = dOut[row, pos*K+k] * x_j (0 for pos >= nf) and
    gw[j] = dwide[row] * x_j: single fp32 multiplies, bit-exact.
    mutant 'pos+1' reads the next position's gradient."""
    row, pos, counts = rows_pos(row_ptr)
    B = counts.numel()
    p = pos + 1 if mutant == "pos+1" else pos
    d = dOut.view(B, nf, K)[row, p.clamp(max=nf - 1)]
    d = torch.where((p < nf).unsqueeze(1), d, torch.zeros_like(d))
    return dwide[row] * vals, d * vals.unsqueeze(1)


def nfm_forward_ref(row_ptr, fids, vals, W, V):
    """float64 wide / sumVX / vec and their bounds.

    wide, sumVX: sum rule. vec = 0.5 (s^2 - q), s = sum vx, q = sum (vx)^2,
    A = sum|vx|: s carries n u A, so fl(s^2) carries (2n+1) u |s| A; q
    carries (n+2) u q (each square rounds its product and itself, then the
    sum); the subtraction adds u (|s| A + q). Halved, the total is
    u [(n+1)|s|A + (n+3)/2 q] <= n 2^-23 (|s| A + q) for every n >= 1,
    which is the bound used."""
    row, _, counts = rows_pos(row_ptr)
    B, K = counts.numel(), V.shape[1]
    n = counts.double()
    x = vals.double()
    wx = W.double()[fids.long()] * x
    vx = V.double()[fids.long()] * x.unsqueeze(1)
    z1 = lambda: torch.zeros(B, dtype=torch.float64)
    zk = lambda: torch.zeros(B, K, dtype=torch.float64)
    wide = z1().index_add_(0, row, wx)
    wide_b = n * U23 * z1().index_add_(0, row, wx.abs())
    s = zk().index_add_(0, row, vx)
    A = zk().index_add_(0, row, vx.abs())
    q = zk().index_add_(0, row, vx * vx)
    nk = n.unsqueeze(1)
    return {
        "wide": (wide, wide_b),
        "sumVX": (s, nk * U23 * A),
        "vec": (0.5 * (s * s - q), nk * U23 * (s.abs() * A + q)),
    }


def nfm_backward_emit_ref(row_ptr, fids, vals, V, sumVX, dvec, dwide,
                          mutant=None):
    """gv[j,k] = dvec[row,k] (sumVX[row,k] - V[fid,k] x) x in float64 and
    gw[j] = dwide[row] x as the exact fp32 multiply.

    Four roundings: v x, the subtraction, and the two multiplies. The
    first two are absolute errors of at most u|vx| and u(|sv| + |vx|)
    scaled by |dv x|, the multiplies add 2u|gv| <= 2u|dv x|(|sv| + |vx|):
    bound 4 u |dv x| (|sv| + |vx|).
    mutant 'noself' omits the -v x term."""
    row, _, _ = rows_pos(row_ptr)
    x = vals.double().unsqueeze(1)
    vx = V.double()[fids.long()] * x
    sv = sumVX.double()[row]
    dv = dvec.double()[row]
    inner = sv if mutant == "noself" else sv - vx
    gv = dv * inner * x
    bound = 4 * U24 * (dv * x).abs() * (sv.abs() + vx.abs())
    return dwide[row] * vals, gv, bound


# ---------------------------------------------------------------------------
# dense elementwise oracles
# ---------------------------------------------------------------------------
def act_backward_ref(dY, Y, act, mutant=None):
    """dZ = dY * act'(Y) with Y the activation's output. act 0/1 are
    selections: returns (fp32 expectation, None), compared bit for bit.
    act 2: (float64 dY y (1-y), bound); three roundings (1-y, y(1-y), the
    product with dY), each relative to a factor of the result, so the
    bound is 3 u |dY| |y| (1 + |y|) >= 3 u |result|.
    mutant 'ge' uses Y >= 0 for relu."""
    if act == 0:
        return dY.clone(), None
    if act == 1:
        mask = (Y >= 0) if mutant == "ge" else (Y > 0)
        return torch.where(mask, dY, torch.zeros_like(dY)), None
    d, y = dY.double(), Y.double()
    return d * y * (1 - y), 3 * U24 * d.abs() * y.abs() * (1 + y.abs())


def colsum_ref(dZ, mutant=None):
    """db[n] = sum_m dZ[m,n]; sum rule with n = M.
    mutant 'droprow' leaves out the last matrix row."""
    d = dZ.double()
    M = d.shape[0]
    bound = M * U23 * d.abs().sum(0)
    if mutant == "droprow":
        d = d[:-1]
    return d.sum(0), bound


def _libm_powf():
    try:
        lib = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        fn = lib.powf
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_float, ctypes.c_float]
        return fn
    except (OSError, AttributeError):
        return None


_POWF = _libm_powf()


def adam_bias_corrections(beta1, beta2, step):
    """bc = 1 - powf((float)beta, (float)step), formed in fp32 exactly as
    the binding forms it (libm powf, then an fp32 subtraction). Forming it
    in float64 would differ by the fp32 rounding of 0.999 alone: 3e-5
    relative in bc2 at step 1."""
    def bc(beta):
        if _POWF is not None:
            p = np.float32(_POWF(float(np.float32(beta)), float(step)))
        else:
            p = np.power(np.float32(beta), np.float32(step))
        return float(np.float32(1.0) - np.float32(p))
    return bc(beta1), bc(beta2)


def adam_ref(W, grad, m, v, lr, beta1, beta2, eps, step, l2, mutant=None):
    """One dense Adam step in float64 on the fp32 state, with the scalar
    hyper-parameters rounded to fp32 as the binding passes them.
    Returns {name: (ref64, bound)} for W, m, v.

      g = grad + l2 W                     2 roundings, on |grad| + |l2 W|
      m' = b1 m + (1-b1) g                3 roundings + (1-b1) err(g)
      v' = b2 v + (1-b2) g g              4 roundings + 2 (1-b2)|g| err(g)
      d  = sqrt(v'/bc2) + eps             relative: half of v's, +u divide,
                                          +u sqrt, +u for the libm the
                                          host's bc2 came from; then +u d
      up = lr (m'/bc1) / d                err(m') scaled, + 3u |up| for the
                                          three operations, +u for bc1,
                                          + |up| err(d)/d
      W' = W - up                         err(up) + one ulp of W'
    (1 - b1) and (1 - b2) are exact in fp32 (Sterbenz), so the oracle's
    double subtraction equals the kernel's.
    mutants: 'eps_in' sqrt(v/bc2 + eps); 'nol2'; 'nobc' bc1 = bc2 = 1."""
    lr, b1, b2, eps, l2 = (f32(t) for t in (lr, beta1, beta2, eps, l2))
    bc1, bc2 = adam_bias_corrections(beta1, beta2, step)
    if mutant == "nobc":
        bc1 = bc2 = 1.0
    if mutant == "nol2":
        l2 = 0.0
    W, grad, m, v = (t.double() for t in (W, grad, m, v))
    g = grad + l2 * W
    eg = 2 * U24 * (grad.abs() + (l2 * W).abs())
    m1 = b1 * m + (1 - b1) * g
    em = (1 - b1) * eg + 3 * U24 * ((b1 * m).abs() + ((1 - b1) * g).abs())
    v1 = b2 * v + (1 - b2) * g * g
    ev = 2 * (1 - b2) * g.abs() * eg + 4 * U24 * v1
    root = torch.sqrt(v1 / bc2)
    if mutant == "eps_in":
        d = torch.sqrt(v1 / bc2 + eps)
    else:
        d = root + eps
    rel_v = torch.where(v1 > 0, ev / v1.clamp(min=1e-300),
                        torch.zeros_like(v1))
    ed = root * (0.5 * rel_v + 3 * U24) + U24 * d
    up = lr * (m1 / bc1) / d
    eup = lr / bc1 / d * em + up.abs() * (4 * U24 + ed / d)
    W1 = W - up
    eW = eup + U23 * W1.abs()
    return {"W": (W1, eW), "m": (m1, em), "v": (v1, ev)}


def adagrad_ref(W, grad, n, lr, eps, l2, mutant=None):
    """One dense Adagrad step in float64: {name: (ref64, bound)} for W, n.

      g  = grad + l2 W                    2 roundings on |grad| + |l2 W|
      n' = n + g g                        2 roundings + 2|g| err(g)
      r  = rsqrt(n' + eps)                +u for the add, half of the
                                          radicand's relative error, and
                                          one ulp (2u) for the hardware
                                          reciprocal square root
      up = lr g r                         err(g) scaled + 2u |up| + |up|
                                          err(r)/r
      W' = W - up                         err(up) + one ulp of W'
    mutants: 'eps_out' 1 / (sqrt(n') + eps); 'nol2'."""
    lr, eps, l2 = f32(lr), f32(eps), f32(l2)
    if mutant == "nol2":
        l2 = 0.0
    W, grad, n = W.double(), grad.double(), n.double()
    g = grad + l2 * W
    eg = 2 * U24 * (grad.abs() + (l2 * W).abs())
    n1 = n + g * g
    en = 2 * g.abs() * eg + 2 * U24 * n1
    rad = n1 + eps
    if mutant == "eps_out":
        r = 1.0 / (torch.sqrt(n1) + eps)
    else:
        r = 1.0 / torch.sqrt(rad)
    rel_r = 0.5 * (en / rad + U24) + 2 * U24
    up = lr * g * r
    eup = lr * r * eg + up.abs() * (2 * U24 + rel_r)
    W1 = W - up
    return {"W": (W1, eup + U23 * W1.abs()), "n": (n1, en)}


def ftrl_ref(w, z, n, g, alpha, beta, l1, l2, mutant=None):
    """Per-coordinate FTRL-proximal in float64 (the arithmetic of
    ``fm_ref.ftrl_apply_ref``'s ``upd``): {name: (ref64, bound)} for
    w, z, n.

      s1 = sqrt(n + g g), s0 = sqrt(n)    relative 2u and u
      sigma = (s1 - s0) / alpha           absolute 2u s1 + u s0 + u|s1-s0|,
                                          scaled by 1/alpha, + u|sigma|
      z' = z + g - sigma w                |w| err(sigma) + u|sigma w| +
                                          2u (|z| + |g| + |sigma w|)
      n' = n + g g                        2u n'
      w' = -(z' - sign(z') l1) / den,     den = (beta + sqrt(n'))/alpha + l2
           0 if |z'| <= l1                all-positive, 5 roundings
    err(w') = (err(z') + u|num|)/den + 6u|w'|. The function is continuous
    at |z'| = l1 (both branches give 0 there), so a kernel that lands on
    the other side of the threshold than the oracle stays inside
    err(z')/den.
    mutant 'lt' uses |z'| < l1; it differs from '<=' only by returning
    -0.0 instead of +0.0 at |z'| == l1."""
    alpha, beta, l1, l2 = f32(alpha), f32(beta), f32(l1), f32(l2)
    w, z, n, g = w.double(), z.double(), n.double(), g.double()
    g2 = g * g
    s1, s0 = torch.sqrt(n + g2), torch.sqrt(n)
    sigma = (s1 - s0) / alpha
    esig = (2 * U24 * s1 + U24 * s0 + U24 * (s1 - s0)) / alpha \
        + U24 * sigma.abs()
    sw = sigma * w
    z1 = z + g - sw
    ez = w.abs() * esig + U24 * sw.abs() \
        + 2 * U24 * (z.abs() + g.abs() + sw.abs())
    n1 = n + g2
    num = z1 - torch.sign(z1) * l1
    den = (beta + torch.sqrt(n1)) / alpha + l2
    live = -num / den
    dead = (z1.abs() < l1) if mutant == "lt" else (z1.abs() <= l1)
    w1 = torch.where(dead, torch.zeros_like(w), live)
    ew = (ez + U24 * num.abs()) / den + 6 * U24 * live.abs()
    return {"w": (w1, ew), "z": (z1, ez), "n": (n1, 2 * U24 * n1)}


# ---------------------------------------------------------------------------
# degenerate-GEMM oracles (bf16 operands held as fp32/64 values)
# ---------------------------------------------------------------------------
def gemm_sum_ref(A, B, mutant=None):
    """C[m,n] = sum_k A[m,k] B[n,k] in float64 from bf16-valued operands;
    products are exact in fp32, so the sum rule applies with n = K.
    mutant 'dropk' leaves out the last k."""
    A, B = A.double(), B.double()
    K = A.shape[1]
    bound = K * U23 * (A.abs() @ B.abs().t())
    if mutant == "dropk":
        A, B = A[:, :-1], B[:, :-1]
    return A @ B.t(), bound


def gemm_epilogue_ref(s, sbound, bias, act):
    """act(s + bias) with its bound. The bias add is one rounding on
    |s| + |bias|. relu is 1-Lipschitz. sigmoid (clamped at +-16) is
    1/4-Lipschitz and is evaluated as 1 / (1 + exp(-z)) with the hardware
    exponential: scaling z by log2(e) and the 1-ulp exp2 give exp a
    relative error within (|z| + 2) 2^-23, the add and the divide one
    rounding each, and d(sigma)/sigma = (1 - sigma) d(e)/e, so the
    evaluation error is within (|z| + 3) 2^-23 sigma."""
    z, b = s, sbound
    if bias is not None:
        z = s + bias.double()
        b = sbound + U24 * (s.abs() + bias.double().abs())
    if act == 0:
        return z, b
    if act == 1:
        return torch.relu(z), b
    zc = z.clamp(-16, 16)
    sig = torch.sigmoid(zc)
    return sig, b / 4 + (zc.abs() + 3) * U23 * sig


def bf16_values(shape, seed, signed=False, scale=1.0):
    """fp32 tensor of bf16-representable values, magnitudes in
    [0.5, 1.5] * scale"""
    g = torch.Generator().manual_seed(seed)
    x = (0.5 + torch.rand(*shape, generator=g)) * scale
    if signed:
        x = x * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
    return x.to(torch.bfloat16).float()


# ---------------------------------------------------------------------------
# shared inputs (GPU tests and the CPU mutation tests build the same ones)
# ---------------------------------------------------------------------------
def embed_inputs(K, lengths, seed, nf=39, dup_row=None):
    row_ptr, fids, vals = make_csr(lengths, seed=seed, dup_row=dup_row)
    B = len(lengths)
    g = torch.Generator().manual_seed(seed + 1000)
    return {
        "row_ptr": row_ptr, "fids": fids, "vals": vals,
        "W": table(F_TABLE, 0, seed + 1), "E": table(F_TABLE, K, seed + 2),
        "dOut": torch.randn(B, nf * K, generator=g),
        "dvec": torch.randn(B, K, generator=g),
        "dwide": torch.randn(B, generator=g),
    }


def nfm_cases(K, base):
    """(lengths, seed, dup_row): length_cases, with the longest row of the
    full set repeating a fid (the set also holds a one-entry row)"""
    for i, (ls, seed) in enumerate(length_cases(K, base=base)):
        yield ls, seed, (ls.index(max(ls)) if i == 0 else None)


def unit_matrix(M, N, seed, last_row_scale=1.0):
    """[M, N] uniform in [0.5, 1.5]; the last row optionally scaled up so
    that losing it stays above an n 2^-23 sum|.| bound when M is large"""
    g = torch.Generator().manual_seed(seed)
    x = 0.5 + torch.rand(M, N, generator=g)
    x[-1] *= last_row_scale
    return x


def colsum_flat_scale(M):
    """The flat N == 1 sum has bound M 2^-23 sum|x| ~ M^2 2^-23; past
    M ~ 2900 that exceeds one element of [0.5, 1.5], so the last element
    (the one a short grid-stride loop loses) is scaled to stay above it:
    the smallest power of two with 0.5 s > M 2^-23 (1.5 M + 1.5 s)."""
    s = 1.0
    while 0.5 * s <= M * U23 * (1.5 * M + 1.5 * s):
        s *= 2.0
    return s


def dense_inputs(shape, scale, seed):
    """W ~ 0.1 randn, grad = +-[0.5, 1.5] * scale, zero optimizer state"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(*shape, generator=g) * 0.1
    mag = (0.5 + torch.rand(*shape, generator=g)) * scale
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return W, (mag * sign).float()


DENSE_SHAPES = [(1, 1), (3, 5), (16, 17), (128, 1), (1, 128), (37, 300)]
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
ADAGRAD = dict(lr=1e-2, eps=1e-8)


def transposed_mirror(W, mutant=None):
    """Wtbf = bf16 of W^T laid out [cols, rows]; mutant 'swapped' indexes
    the flat buffer with rows and cols exchanged, which leaves W's own
    layout in place."""
    rows, cols = W.shape
    if mutant == "swapped":
        return W.contiguous().view(cols, rows).to(torch.bfloat16)
    return W.t().contiguous().to(torch.bfloat16)


SPARSE_F = 512
SPARSE_NLIVE = 37
FTRL = dict(alpha=0.15, beta=1.0, l1=1e-2, l2=1e-4)


def sparse_inputs(D, seed, ftrl=False):
    """State for the runtime-D sparse optimizers: F = 512 rows, 37 listed
    fids followed by 11 more distinct in-range fids past `count` that must
    stay untouched. Under ftrl the first listed rows get gradients at and
    around the l1 dead-zone edge: from zero state z' = g exactly, so
    g = +-l1 sits on the edge, 0.5 l1 inside, (1 + 2^-10) l1 just outside.
    """
    g = torch.Generator().manual_seed(seed)
    F = SPARSE_F
    perm = torch.randperm(F, generator=g)
    uniq = perm[:SPARSE_NLIVE + 11].to(torch.int32)
    st = {
        "uniq": uniq,
        "W": torch.randn(F, generator=g) * 0.1,
        "V": torch.randn(F, D, generator=g) * 0.1,
        "gradW": torch.randn(F, generator=g),
        "gradV": torch.randn(F, D, generator=g),
        "nW": torch.zeros(F), "nV": torch.zeros(F, D),
    }
    if ftrl:
        st["zW"] = torch.zeros(F)
        st["zV"] = torch.zeros(F, D)
        # FTRL's closed form owns the weights: start from w = 0, z = 0
        st["W"].zero_()
        l1 = float(np.float32(FTRL["l1"]))
        edge = torch.tensor([l1, -l1, 0.5 * l1, -0.5 * l1,
                             l1 * (1 + 2.0 ** -10), -l1 * (1 + 2.0 ** -10)])
        live = uniq[:6].long()
        st["gradW"][live] = edge
        st["V"][live] = 0.0
        st["gradV"][live, :] = edge.unsqueeze(1).expand(6, D).contiguous()
    return st
