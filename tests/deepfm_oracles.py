"""float64 oracles, exact-arithmetic inputs and derived bounds for the two
DeepFM kernels (``deepfm_forward``, ``deepfm_backward_emit``).

Plain helper module in the style of ``fm_oracles`` / ``kernel_oracles``;
everything here runs on the CPU. ``test_deepfm_kernels_gpu.py`` feeds these
inputs to the kernels; ``test_deepfm_oracles.py`` (CPU) holds the oracles to
the model's fp32 CPU path and to autograd, and shows that every wrong
reference listed there is caught on the same inputs.

The definition the oracles are written from (CSR batch, nf = num_fields,
pos = position of entry j in its row r):

    wide[r]  = sum_j W[f_j] x_j                                 all entries
    s[r,k]   = sum_j E[f_j,k] x_j                               all entries
    fm[r]    = wide[r] + 1/2 sum_k (s[r,k]^2 - sum_j (E[f_j,k] x_j)^2)
    concat[r, pos*K+k] = bf16(E[f_j,k] x_j)  for pos < nf, +0 elsewhere
    gw[j]    = d x_j                                            d = dpred[r]
    gv[j,k]  = (D + d (s[r,k] - E[f_j,k] x_j)) x_j
               D = dDeep[r, pos*K+k] for pos < nf, 0 past nf

Exact-input rule (``fm_oracles``): with E in {-2..2}, W in {-3..3},
x in {1, 2}, dpred = +-2^-s and dDeep in {-4..4} 2^-s every product and every
partial sum is an integer multiple of 2^-s (of 1/2 for fm), exact in fp32 as
long as it stays below 2^24 units; ``assert_exact`` checks that on the float64
side of every case, for the accumulators of the kernel's reduction:

* per lane and across the feature groups, sums of E x and of (E x)^2 for one
  k: sum_j |E x| < 2^24 and sum_j (E x)^2 < 2^24;
* s_k^2 - q_k per k, then one butterfly over the K lanes of a group: every
  term once, no replication factor (unlike fm_forward, which adds each
  square G times), so sum_k (s_k^2 + q_k) < 2^24;
* the wide sum: sum_j |w x| < 2^24;
* fm = wide + 1/2 pair in units of 1/2: 2 sum|w x| + sum_k (s_k^2 + q_k)
  < 2^24;
* gv in units of 2^-s: (|D| + |d| (|s| + |E x|)) x < 2^24 units.

Then fm, sumVX and gw compare bit for bit, gv by value (a negative d times a
zero bracket is -0 where the oracle holds +0), the concat bit for bit against
bf16(E x) and its padding against +0.
"""

from __future__ import annotations

import torch

from fm_oracles import EXACT_LIMIT, check_value, padded  # noqa: F401
from kernel_oracles import (U23, U24, check_bits, check_bound,  # noqa: F401
                            differs, length_cases, length_set, make_csr,
                            poison, rows_pos)

KS = (4, 8, 16, 32, 64)
NFS = (1, 5, 39)       # rows shorter than, equal to and longer than nf
F_DFM = 2048           # table rows; row F-1 is NaN


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
def _keep(row_ptr, K, nf, mutant):
    """entries a (wrong) forward sums over"""
    row, pos, counts = rows_pos(row_ptr)
    keep = torch.ones(row.numel(), dtype=torch.bool)
    if mutant == "droplast":
        keep = pos != (counts[row] - 1)
    elif mutant == "drop4G":
        keep = pos != 4 * (64 // K)
    elif mutant == "fm_nf":
        keep = pos < nf
    return row, pos, counts, keep


def forward64(row_ptr, fids, vals, W, E, nf, keep=None):
    """(wide, s, q, deep_in) in float64 from the definition; differentiable
    in W and E. keep: entries that take part (all by default)."""
    row, pos, counts = rows_pos(row_ptr)
    B, K = counts.numel(), E.shape[1]
    f = fids.long()
    x = vals.double()
    if keep is not None:
        x = torch.where(keep, x, torch.zeros(1, dtype=torch.float64))
    wx = W.double()[f] * x
    vx = E.double()[f] * x.unsqueeze(1)
    wide = torch.zeros(B, dtype=torch.float64).index_add(0, row, wx)
    s = torch.zeros(B, K, dtype=torch.float64).index_add(0, row, vx)
    q = torch.zeros(B, K, dtype=torch.float64).index_add(0, row, vx * vx)
    in_nf = pos < nf
    if keep is not None:
        in_nf = in_nf & keep
    deep = torch.zeros(B * nf, K, dtype=torch.float64).index_add(
        0, (row * nf + pos)[in_nf], vx[in_nf])
    return wide, s, q, deep.view(B, nf * K)


def concat_expect(row_ptr, fids, vals, E, nf, mutant=None):
    """bf16 [B, nf*K]: bf16 of the single fp32 product E x at pos < nf, +0
    elsewhere; bit-exact. mutants: 'nopad' leaves the padding unwritten (NaN
    stands for what the allocator held); 'droplast' / 'drop4G' lose that
    entry's slot as well."""
    K = E.shape[1]
    row, pos, counts, keep = _keep(
        row_ptr, K, nf, mutant if mutant in ("droplast", "drop4G") else None)
    B = counts.numel()
    prod = E[fids.long()] * vals.unsqueeze(1)
    fill = float("nan") if mutant == "nopad" else 0.0
    out = torch.full((B, nf, K), fill)
    w = (pos < nf) & keep
    out[row[w], pos[w]] = prod[w]
    return out.view(B, nf * K).to(torch.bfloat16)


def deepfm_forward_ref(row_ptr, fids, vals, W, E, nf, mutant=None):
    """fm and sumVX in float64 with their float-set bounds, the expected
    concat, and the magnitudes ``assert_exact`` reads.

    sumVX_k: the sum rule, n 2^-23 A_k with A_k = sum_j |E x| (n = row
    length; per-lane chains and the group butterfly are one n-term sum in
    some order).
    fm: v_k = s_k^2 - q_k. s_k carries n u A_k, so fl(s_k^2) carries
    (2n + 1) u |s_k| A_k; q_k, an n-term sum of squares of once-rounded
    products, (n + 2) u q_k; the subtraction u (s_k^2 + q_k) <= u (|s_k| A_k
    + q_k): in all (2n + 2) u |s_k| A_k + (n + 3) u q_k <= 2 n 2^-23
    (|s_k| A_k + q_k) for n >= 1. The butterfly over k is a K-term sum of the
    v_k: K 2^-23 sum_k |v_k| <= K 2^-23 (T + Q), T = sum s_k^2, Q = sum q_k.
    The halving is exact, so the pair term carries n 2^-23 sum_k (|s_k| A_k
    + q_k) + K 2^-23 (T + Q) / 2. The wide part is an n-term sum (the lanes
    that hold no w add exact zeros): n 2^-23 sum|w x|. The last addition
    rounds once on |wide| + (T + Q) / 2.

    mutants: 'droplast' / 'drop4G' lose the last entry / the entry at
    position 4G of every row; 'nohalf'; 'wide_all' takes sum w x from every
    lane of a group (K times); 'fm_nf' drops the entries past nf from the FM
    sums; 'nopad' (concat only)."""
    K = E.shape[1]
    row, pos, counts, keep = _keep(row_ptr, K, nf, mutant)
    B = counts.numel()
    n = counts.double()
    wide, s, q, _ = forward64(row_ptr, fids, vals, W, E, nf, keep)
    ax = vals.double().abs()
    A = torch.zeros(B, K, dtype=torch.float64).index_add_(
        0, row, E.double()[fids.long()].abs() * ax.unsqueeze(1))
    alin = torch.zeros(B, dtype=torch.float64).index_add_(
        0, row, W.double()[fids.long()].abs() * ax)
    T, Q = (s * s).sum(1), q.sum(1)
    half = 1.0 if mutant == "nohalf" else 0.5
    if mutant == "wide_all":
        wide = wide * K
    fm = wide + half * (s * s - q).sum(1)
    has = (n > 0).double()
    fm_b = (n * U23 * (s.abs() * A + q).sum(1)
            + has * K * U23 * 0.5 * (T + Q)
            + n * U23 * alin
            + has * U24 * (alin + 0.5 * (T + Q)))
    return {"fm": (fm, fm_b), "sumVX": (s, n.unsqueeze(1) * U23 * A),
            "concat": concat_expect(row_ptr, fids, vals, E, nf, mutant),
            "A": A, "T": T, "Q": Q, "alin": alin}


# ---------------------------------------------------------------------------
# backward emit
# ---------------------------------------------------------------------------
def deepfm_emit_ref(row_ptr, fids, vals, E, sumVX, dDeep, dpred, nf,
                    mutant=None):
    """(gw64, gv64, gv bound) from the sumVX, dDeep and dpred handed to the
    kernel.

    gw is one fp32 multiply: compared bit for bit with that multiply.
    gv = (D + d (s - e x)) x has five roundings, 2^-24 each to first order,
    absolute values at the additions: e x (u|ex|), the subtraction
    (u (|s| + |ex|)), the product with d (u |d| (|s| + |ex|)), the addition
    of D (u (|D| + |d| (|s| + |ex|))) and the product with x. Carried to the
    result: u |x| [ |d| |ex| + 4 |d| (|s| + |ex|) + 2 |D| ]
    <= 5 u |x| (|D| + |d| (|s| + |ex|)), the bound used. FMA contraction
    only removes roundings.

    mutants: 'noself' omits -e x; 'pos+1' reads the next position's D;
    'past_nf' gives the entries past nf the D of the last slot (a clamped
    index without the guard); 'D_after' adds D after the multiply by x."""
    row, pos, counts = rows_pos(row_ptr)
    B, K = counts.numel(), E.shape[1]
    x = vals.double().unsqueeze(1)
    d = dpred.double()[row].unsqueeze(1)
    ex = E.double()[fids.long()] * x
    sv = sumVX.double()[row]
    p = pos + 1 if mutant == "pos+1" else pos
    D = dDeep.double().reshape(B, nf, K)[row, p.clamp(max=nf - 1)]
    if mutant != "past_nf":
        D = torch.where((p < nf).unsqueeze(1), D, torch.zeros_like(D))
    inner = sv if mutant == "noself" else sv - ex
    if mutant == "D_after":
        gv = D + d * inner * x
    else:
        gv = (D + d * inner) * x
    bound = 5 * U24 * x.abs() * (D.abs() + d.abs() * (sv.abs() + ex.abs()))
    return dpred.double()[row] * vals.double(), gv, bound


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def case(K, lengths, seed, nf, exact=True, s=3, small=False, dup_row=None):
    """One CSR batch with its tables and upstream gradients. exact: E in
    {-2..2}, W in {-3..3}, x in {1, 2}, dpred = +-2^-s, dDeep in {-4..4}
    2^-s (small: E in {-1, 0, 1}, x = 1, for rows of 130 and 1000 entries).
    float: E ~ 0.1 N(0, 1), W ~ N(0, 1), x in [0.5, 1.5], dpred and dDeep
    ~ N(0, 1) / B. Fids are below F-1; row F-1 of W and E is NaN (the padding
    around the fids view names it). dup_row repeats a fid inside that row."""
    g = torch.Generator().manual_seed(seed)
    F = F_DFM
    row_ptr, fids, vals = make_csr(lengths, F=F - 1, seed=seed,
                                   dup_row=dup_row)
    B, nnz = len(lengths), fids.numel()
    if exact:
        hi = 1 if small else 2
        E = torch.randint(-hi, hi + 1, (F, K), generator=g).float()
        W = torch.randint(-3, 4, (F,), generator=g).float()
        vals = torch.ones(nnz) if small else \
            torch.randint(1, 3, (nnz,), generator=g).float()
        sign = torch.randint(0, 2, (B,), generator=g).float() * 2 - 1
        dpred = sign * 2.0 ** -s
        dDeep = torch.randint(-4, 5, (B, nf * K), generator=g).float() \
            * 2.0 ** -s
    else:
        E = torch.randn(F, K, generator=g) * 0.1
        W = torch.randn(F, generator=g)
        dpred = torch.randn(B, generator=g) / max(B, 1)
        dDeep = torch.randn(B, nf * K, generator=g) / max(B, 1)
    E[F - 1] = float("nan")
    W[F - 1] = float("nan")
    return {"K": K, "F": F, "B": B, "nf": nf, "row_ptr": row_ptr,
            "fids": fids, "vals": vals, "W": W, "E": E, "dpred": dpred,
            "dDeep": dDeep, "exact": exact, "s": s}


def exact_cases(K):
    """The exact cases of one K, each at nf = 1, 5 and 39: the loop-edge
    lengths of ``length_set`` (0, 1, G-1, G, G+1, 4G-1, 4G, 4G+1, 8G+1, 39,
    empty rows first, in the middle and last) and the rows-per-block sweep
    of ``length_cases`` (batches of 1, 3, 4, 5 and 9 rows), adjacent empty
    rows, one fid twice in a row, and the long rows 130 / 1000 on the small
    value set."""
    G = 64 // K
    out = []
    for nf in NFS:
        for i, (ls, seed) in enumerate(length_cases(K, base=9000 + nf)):
            dup = ls.index(max(ls)) if i == 0 else None
            out.append(case(K, ls, seed, nf, s=2 + i, dup_row=dup))
        out.append(case(K, [0, 0, G + 1, 0, 0, 39, 2, 0, 0], 9900 + nf + K,
                        nf, s=5))
        out.append(case(K, [130, 0, 1000, 1, 130], 9950 + nf + K, nf, s=4,
                        small=True))
    return out


def float_case(K):
    """one float case per K: every length of the set plus 130 and 1000 at
    nf = 39"""
    return case(K, length_set(K) + [130, 1000], 9990 + K, 39, exact=False)


def case_sumvx32(c):
    """the sumVX the backward is handed: float64 s cast to fp32"""
    fw = deepfm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"],
                            c["E"], c["nf"])
    return fw["sumVX"][0].float()


def _mx(t):
    return float(t.max()) if t.numel() else 0.0


def assert_exact(c):
    """Exactness conditions of one exact case (module text): fails the case
    when an accumulator could leave the exactly representable range."""
    assert c["exact"]
    fw = deepfm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"],
                            c["E"], c["nf"])
    s = fw["sumVX"][0]
    assert _mx(fw["A"]) < EXACT_LIMIT, "sum |E x|"
    assert _mx(fw["Q"]) < EXACT_LIMIT, "sum (E x)^2"
    assert _mx(fw["T"] + fw["Q"]) < EXACT_LIMIT, "sum_k (s_k^2 + q_k)"
    assert _mx(fw["alin"]) < EXACT_LIMIT, "sum |w x|"
    assert _mx(2 * fw["alin"] + fw["T"] + fw["Q"]) < EXACT_LIMIT, "fm"
    assert torch.equal(s.float().double(), s)
    fm = fw["fm"][0]
    assert torch.equal(fm.float().double(), fm)
    gw, gv, bound = deepfm_emit_ref(c["row_ptr"], c["fids"], c["vals"],
                                    c["E"], s.float(), c["dDeep"],
                                    c["dpred"], c["nf"])
    unit = 2.0 ** -c["s"]
    # bound / (5 u) = |x| (|D| + |d| (|s| + |e x|)): every partial of gv
    assert _mx(bound / (5 * U24)) / unit < EXACT_LIMIT, "gv"
    for t in (gw, gv):
        assert torch.equal(t.float().double(), t)
        qn = t / unit
        assert torch.equal(qn, qn.round())
