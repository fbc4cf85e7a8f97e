"""float64 oracles, exact-arithmetic inputs and derived bounds for the four
field-addressed embedding-bag kernels (``embed_bag_forward``,
``embed_bag_backward_emit``, ``deepfm_bag_forward``,
``deepfm_bag_backward_emit``; embed_bag_kernels.hip).

Plain helper module in the style of ``deepfm_oracles``; everything here runs
on the CPU. ``test_embed_bag_kernels_gpu.py`` feeds these inputs to the
kernels; ``test_embed_bag_oracles.py`` (CPU) holds the oracles to a plain
Python loop and shows that every wrong reference listed there differs on the
same inputs.

The definition (CSR batch, nf slots, c_j = fields[j], an entry is *in* when
0 <= c_j < nf; cnt(r,c) = number of in-entries of row r with field c):

    concat[r, c*K+k] = bf16( fl32( S * inv ) ),  S = sum_{j in (r,c)} E[f_j,k] x_j
                       inv = 1 (sum) or fl32(1 / cnt(r,c)) (mean); +0 when
                       the slot has no entry
    wide, s, fm      : deepfm_oracles, over every entry of the row
    embed emit       : gw[j] = dwide[r] x_j,  gv[j,k] = fl32(D inv) x_j
    deepfm emit      : gw[j] = d x_j,
                       gv[j,k] = (fl32(D inv) + d (s[r,k] - E[f_j,k] x_j)) x_j
                       D = dOut[r, c_j*K+k] for an in-entry, 0 otherwise

Exact-input rule: the value sets of ``deepfm_oracles.case`` (E in {-2..2},
x in {1, 2}, dpred = +-2^-s, dDeep in {-4..4} 2^-s; `small`: E in {-1, 0, 1},
x = 1). Every slot sum S is then an integer below 2^24 in any order
(``assert_exact`` checks sum |E x| per slot), exact in fp32. inv is the
correctly rounded fp32 reciprocal of a small integer, which numpy's float32
divide reproduces bit for bit; S * inv has at most 48 significant bits, so
the float64 product is exact and its cast to fp32 IS the kernel's single
correctly rounded multiply (asserted: S and inv are fp32 values, |S| < 2^24);
the cast to bf16 is the second rounding the kernel does as well. The same
holds for D * inv in the backward. With d a power of two and s - E x an
integer, d (s - E x) is exact, so fl32(D inv) + d (s - E x) rounds once
whether or not the compiler contracts it into an FMA, and x in {1, 2} makes
the last multiply exact: the mean-pooled gv is reproduced by value too.
"""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import torch

import deepfm_oracles as do
from fm_oracles import EXACT_LIMIT, check_value, padded  # noqa: F401
from kernel_oracles import (U23, U24, check_bits, check_bound,  # noqa: F401
                            differs, poison, rows_pos)

KS = do.KS
NFS = do.NFS           # 1, 5, 39
POOLINGS = (0, 1)      # sum, mean
BF16_U = 2.0 ** -8     # unit roundoff of bf16: 8 significant bits, half an
                       # ulp of 2^-7 relative
# the per-block LDS limit of gfx950 documented in docs/KERNELS.md
LDS_LIMIT = 163840


def lds_bytes(nf, K):
    """dynamic LDS of the forward kernels: per wave nf*K fp32 of staging and
    nf counters, four waves per block"""
    return 16 * nf * (K + 1)


def nf_past_lds(K):
    """smallest nf whose staging does not fit LDS_LIMIT"""
    return LDS_LIMIT // (16 * (K + 1)) + 1


# ---------------------------------------------------------------------------
# slots
# ---------------------------------------------------------------------------
def slots(row_ptr, fields, nf, mutant=None):
    """entry -> (row, in mask, flat slot row*nf + c (0 where out), counts
    [B*nf] int64). mutant 'clamp' clamps an out-of-range field into
    [0, nf-1] instead of leaving the entry out."""
    row, _, counts = rows_pos(row_ptr)
    B = counts.numel()
    c = fields.long()
    if mutant == "clamp":
        c = c.clamp(0, nf - 1)
    inn = (c >= 0) & (c < nf)
    flat = torch.where(inn, row * nf + c, torch.zeros_like(c))
    cnt = torch.zeros(B * nf, dtype=torch.int64).index_add_(
        0, flat[inn], torch.ones(int(inn.sum()), dtype=torch.int64))
    return row, inn, flat, cnt


def inv32(cnt, pooling):
    """fp32 [len(cnt)]: 1 (sum, and empty slots) or the correctly rounded
    fp32 reciprocal of the count (mean)"""
    n = cnt.clamp(min=1).numpy().astype(np.float32)
    if pooling == 0:
        return torch.ones(cnt.numel())
    return torch.from_numpy(np.float32(1.0) / n)


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
def bag_sums64(row_ptr, fields, fids, vals, E, nf, mutant=None):
    """(S [B*nf, K] float64 slot sums, A [B*nf, K] sums of |E x|, cnt)"""
    row, inn, flat, cnt = slots(row_ptr, fields, nf, mutant)
    B, K = row_ptr.numel() - 1, E.shape[1]
    vx = E.double()[fids.long()] * vals.double().unsqueeze(1)
    S = torch.zeros(B * nf, K, dtype=torch.float64).index_add_(
        0, flat[inn], vx[inn])
    A = torch.zeros(B * nf, K, dtype=torch.float64).index_add_(
        0, flat[inn], vx[inn].abs())
    return S, A, cnt


def concat_ref(row_ptr, fields, fids, vals, E, nf, pooling, mutant=None):
    """(value64 [B, nf*K] = S * inv32 exactly, bound, cnt). The bound is for
    float inputs: the n-term sum of once-rounded products carries
    n 2^-23 A (the sum rule of ``deepfm_oracles``), inv and the multiply one
    2^-24 each, relative; the bf16 rounding 2^-8 of the fp32 value:
    e32 = inv A (n 2^-23 + 2 2^-24), bound = e32 + 2^-8 (|S inv| + e32).

    mutants (wrong references): 'position' lays the concat out by position in
    the row; 'sum' pools a mean by sum; 'mean_x' divides by the slot's sum of
    x instead of its count; 'clamp' clamps out-of-range fields; 'nopad'
    leaves empty slots unwritten (NaN)."""
    B, K = row_ptr.numel() - 1, E.shape[1]
    if mutant == "position":
        _, pos, _ = rows_pos(row_ptr)
        fields = pos
    S, A, cnt = bag_sums64(row_ptr, fields, fids, vals, E, nf,
                           "clamp" if mutant == "clamp" else None)
    inv = inv32(cnt, 0 if mutant == "sum" else pooling).double()
    if mutant == "mean_x" and pooling == 1:
        row, inn, flat, _ = slots(row_ptr, fields, nf)
        sx = torch.zeros(B * nf, dtype=torch.float64).index_add_(
            0, flat[inn], vals.double()[inn])
        inv = torch.where(sx > 0, 1.0 / sx.clamp(min=1e-30).float().double(),
                          torch.ones_like(sx))
    val = S * inv.unsqueeze(1)
    n = cnt.double().unsqueeze(1)
    e32 = inv.unsqueeze(1) * A * (n * U23 + 2 * U24)
    bound = e32 + BF16_U * (val.abs() + e32)
    if mutant == "nopad":
        val = torch.where((cnt == 0).unsqueeze(1),
                          torch.full_like(val, float("nan")), val)
    return val.view(B, nf * K), bound.view(B, nf * K), cnt


def concat_expect(row_ptr, fields, fids, vals, E, nf, pooling, mutant=None):
    """bf16 [B, nf*K] of an exact case, bit for bit: fp32(S * inv) -> bf16;
    empty slots and zero sums are +0 (the accumulator starts at +0)."""
    val, _, _ = concat_ref(row_ptr, fields, fids, vals, E, nf, pooling,
                           mutant)
    return (val.float() + 0.0).to(torch.bfloat16)


def concat_loop(row_ptr, fields, fids, vals, E, nf, pooling):
    """the definition as a plain loop, float64"""
    B, K = row_ptr.numel() - 1, E.shape[1]
    out = torch.zeros(B, nf, K, dtype=torch.float64)
    cnt = torch.zeros(B, nf)
    for r in range(B):
        for j in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            c = int(fields[j])
            if 0 <= c < nf:
                out[r, c] += E[int(fids[j])].double() * float(vals[j])
                cnt[r, c] += 1
    if pooling == 1:
        inv = np.float32(1.0) / cnt.clamp(min=1).numpy().astype(np.float32)
        out = out * torch.from_numpy(inv).double().unsqueeze(2)
    return out.view(B, nf * K)


# ---------------------------------------------------------------------------
# backward emits
# ---------------------------------------------------------------------------
def _dm64(row_ptr, fields, dOut, nf, K, pooling, mutant=None):
    """per-entry (row, fl32(D inv) as float64 [nnz, K], |D| inv [nnz, K])"""
    B = row_ptr.numel() - 1
    if mutant == "position":
        _, pos, _ = rows_pos(row_ptr)
        fields = pos
    row, inn, flat, cnt = slots(row_ptr, fields, nf,
                                "clamp" if mutant == "clamp" else None)
    inv = inv32(cnt, 0 if mutant == "sum" else pooling).double()[flat]
    D = dOut.double().reshape(B * nf, K)[flat]
    D = torch.where(inn.unsqueeze(1), D, torch.zeros_like(D))
    prod = D * inv.unsqueeze(1)
    return row, prod.float().double(), prod.abs()


def embed_bag_emit_ref(row_ptr, fields, vals, dOut, dwide, nf, K, pooling,
                       mutant=None):
    """(gw64, gv64, gv bound). gw is one fp32 multiply. gv = fl(fl(D inv) x):
    inv, D inv and the product with x round once each, 3 2^-24 |D inv x|."""
    row, dm, mag = _dm64(row_ptr, fields, dOut, nf, K, pooling, mutant)
    x = vals.double().unsqueeze(1)
    return (dwide.double()[row] * vals.double(), dm * x,
            3 * U24 * mag * x.abs())


def deepfm_bag_emit_ref(row_ptr, fields, fids, vals, E, sumVX, dDeep, dpred,
                        nf, pooling, mutant=None):
    """(gw64, gv64 rounded as the kernel rounds an exact case, gv bound).

    gv = (fl(D inv) + d (s - e x)) x. ``deepfm_oracles.deepfm_emit_ref``
    derives u |x| [ |d| |ex| + 4 |d| (|s| + |ex|) + 2 |D| ] for the position
    kernel; fl(D inv) adds the roundings of inv and of the product, 2 u
    |D inv| at the addition, carried through: 4 u |x| |D inv| for the deep
    part, still within 5 u |x| (|D inv| + |d| (|s| + |ex|)), the bound used.
    On an exact case d (s - e x) is exact and the sum rounds once: gv64 is
    that fp32 value times x (module text)."""
    K = E.shape[1]
    row, dm, mag = _dm64(row_ptr, fields, dDeep, nf, K, pooling, mutant)
    x = vals.double().unsqueeze(1)
    d = dpred.double()[row].unsqueeze(1)
    ex = E.double()[fids.long()] * x
    sv = sumVX.double()[row]
    inner = dm + d * (sv - ex)
    gv = inner.float().double() * x
    bound = 5 * U24 * x.abs() * (mag + d.abs() * (sv.abs() + ex.abs()))
    return dpred.double()[row] * vals.double(), gv, bound


def emit_loops(row_ptr, fields, fids, vals, E, sumVX, dOut, dscore, nf,
               pooling):
    """Both emits from the definition as a plain loop over rows and entries
    (a twin of the vectorised oracles above): (gw, embed gv, deepfm gv) in
    float64, with fl32 applied where the kernel rounds an exact case: D inv,
    and the sum fl32(D inv) + d (s - e x)."""
    B, K = row_ptr.numel() - 1, E.shape[1]
    nnz = fids.numel()
    gw = torch.zeros(nnz, dtype=torch.float64)
    gv_e = torch.zeros(nnz, K, dtype=torch.float64)
    gv_d = torch.zeros(nnz, K, dtype=torch.float64)
    for r in range(B):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        cnt = [0] * nf
        for j in range(lo, hi):
            if 0 <= int(fields[j]) < nf:
                cnt[int(fields[j])] += 1
        d = float(dscore[r])
        for j in range(lo, hi):
            c, x = int(fields[j]), float(vals[j])
            dm = torch.zeros(K, dtype=torch.float64)
            if 0 <= c < nf:
                inv = float(np.float32(1.0) / np.float32(cnt[c])) \
                    if pooling == 1 else 1.0
                dm = (dOut[r, c * K:(c + 1) * K].double() * inv) \
                    .float().double()
            ex = E[int(fids[j])].double() * x
            gw[j] = d * x
            gv_e[j] = dm * x
            gv_d[j] = (dm + d * (sumVX[r].double() - ex)).float().double() * x
    return gw, gv_e, gv_d


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def case(K, rows, nf, seed, exact=True, s=3, small=False, dup_row=None,
         nonzero=False):
    """One CSR batch: ``rows`` lists the field of every entry, row by row.
    Tables and upstream gradients are ``deepfm_oracles.case``'s (fids below
    F-1; row F-1 of W and E is NaN). dup_row: the first two entries of that
    row carry the same fid. nonzero: no zero in E (no zero products)."""
    lengths = [len(r) for r in rows]
    c = do.case(K, lengths, seed, nf, exact=exact, s=s, small=small,
                dup_row=dup_row)
    c["fields"] = torch.tensor([f for r in rows for f in r],
                               dtype=torch.int32)
    if nonzero:
        E = c["E"]
        c["E"] = torch.where(E == 0, torch.ones_like(E), E)
    c["dwide"] = c["dpred"]
    return c


def _shuffled(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(n, generator=g).tolist()


def pattern_rows(K, nf, seed):
    """The rows every exact case is cut from, by name. G = 64/K entries make
    one trip, four trips are unrolled."""
    G = 64 // K
    a, b, mid = 0, nf - 1, nf // 2
    full = list(range(nf))
    rows = {
        "empty": [],
        "one_first": [a], "one_last": [b],
        "in_order": full, "reversed": full[::-1],
        "shuffled": [full[i] for i in _shuffled(nf, seed)],
        "no_first": full[1:], "no_last": full[:-1],
        "no_mid": full[:mid] + full[mid + 1:],
        # a, b, a: the two a's in one trip (G >= 3) and in different trips
        "aba": [a, b, a], "aba_far": [a] + [b] * G + [a],
        "dup_fid": [mid, mid, a],              # with dup_row: one fid twice
        "outside": [-1, a, nf, b, nf + 5, mid, -1],
        # mean counts 3, 5, 7 (and 15 when nf = 1)
        "cnt357": [a] * 3 + [mid] * 5 + [b] * 7,
        "multi": [full[i % nf] for i in _shuffled(3 * nf, seed + 1)][:45],
    }
    for n in sorted({G - 1, G, G + 1, 4 * G - 1, 4 * G, 4 * G + 1} - {0}):
        rows[f"same{n}"] = [mid] * n
    return rows


def exact_cases(K, nf):
    """The exact cases of one (K, nf): batches of 1, 3, 4, 5 and 9 rows
    around the four rows of a block; empty rows first, last, in the middle
    and adjacent; every pattern of ``pattern_rows``; one slot of 130 entries
    on the small value set."""
    G = 64 // K
    p = pattern_rows(K, nf, 700 + K + nf)
    same = [p[k] for k in p if k.startswith("same")]
    e = p["empty"]
    base = 7000 + 10 * K + nf
    out = [
        case(K, [p["multi"]], nf, base + 1),                        # B = 1
        case(K, [p["dup_fid"], e, p["in_order"]], nf, base + 2,     # B = 3
             dup_row=0),
        case(K, [p["reversed"], p["aba"], p["aba_far"], p["outside"]], nf,
             base + 3, s=4),                                        # B = 4
        case(K, [e, p["shuffled"], p["no_first"], p["no_last"], e], nf,
             base + 4, s=2),                                        # B = 5
        case(K, [p["one_first"], e, e, p["no_mid"], p["one_last"],
                 p["cnt357"], p["multi"][::-1], e, p["in_order"]], nf,
             base + 5, s=5),                                        # B = 9
        case(K, same + [e], nf, base + 6),
        case(K, [[nf // 2] * 130, e, p["multi"], [0] * (4 * G + 1)], nf,
             base + 7, s=4, small=True),
    ]
    return out


def position_cases(K, nf):
    """Rows whose fields are 0..len-1 in order with len <= nf and no zero
    product (E has no zero, x > 0): the field layout with sum pooling is the
    position layout there, so the bag kernels must be bit-equal to the
    position kernels."""
    G = 64 // K
    lens = sorted({0, 1, min(G, nf), min(G + 1, nf), min(4 * G + 1, nf),
                   nf // 2, nf - 1, nf})
    rows = [list(range(n)) for n in lens] + [[], list(range(nf))]
    return [case(K, rows, nf, 7700 + K + nf, nonzero=True),
            case(K, [list(range(nf))] * 5, nf, 7800 + K + nf, nonzero=True)]


def float_case(K):
    """one float case per K at nf = 39: every pattern, a slot of 130
    entries, fields outside [0, nf) mixed in"""
    p = pattern_rows(K, 39, 900 + K)
    rows = [p[k] for k in p] + [[19] * 130, []]
    return case(K, rows, 39, 7990 + K, exact=False)


def permuted(c, seed):
    """(case with the entries of every row permuted, perm): new[j] =
    old[perm[j]] for fields, fids and vals"""
    g = torch.Generator().manual_seed(seed)
    rp = c["row_ptr"].tolist()
    perm = torch.cat([rp[r] + torch.randperm(rp[r + 1] - rp[r], generator=g)
                      for r in range(c["B"])] + [torch.zeros(0).long()])
    out = dict(c)
    for k in ("fields", "fids", "vals"):
        out[k] = c[k][perm].contiguous()
    return out, perm


def case_sumvx32(c):
    return do.case_sumvx32(c)


def assert_product_exact(a, b, what):
    """The float64 product a * b of two float64 tensors is exact, so that
    its cast to fp32 is the single correctly rounded fp32 multiply of the
    kernel. Checked in integers: with a = ma 2^ea and b = mb 2^eb (frexp,
    53-bit integer mantissas, trailing zeros stripped) the product's
    mantissa ma mb must fit 53 bits. Python integers do not round."""
    if a.numel() == 0:
        return
    pairs = torch.unique(torch.stack([a.flatten(), b.flatten()], 1), dim=0)
    prod = (pairs[:, 0] * pairs[:, 1]).tolist()
    for (x, y), p in zip(pairs.tolist(), prod):
        if x == 0.0 or y == 0.0:
            continue
        ms = []
        for v in (x, y):
            m, _ = math.frexp(v)
            m = int(abs(m) * (1 << 53))
            ms.append(m // (m & -m))
        assert (ms[0] * ms[1]).bit_length() <= 53, (what, x, y)
        assert Fraction(x) * Fraction(y) == Fraction(p), (what, x, y)


def assert_exact(c):
    """Exactness conditions (module text) of one exact case, on top of
    ``deepfm_oracles.assert_exact`` for fm, sumVX and the FM part of gv."""
    do.assert_exact(c)
    nf, K = c["nf"], c["K"]
    S, A, cnt = bag_sums64(c["row_ptr"], c["fields"], c["fids"], c["vals"],
                           c["E"], nf)
    # S and inv are fp32 values with |S| < 2^24 and cnt < 2^24: the float64
    # product S * inv is exact, its fp32 cast the kernel's one rounding
    if A.numel():
        assert float(A.max()) < EXACT_LIMIT, "slot sum of |E x|"
        assert int(cnt.max()) < EXACT_LIMIT, "slot count"
    assert torch.equal(S.float().double(), S)
    inv = inv32(cnt, 1).double()
    assert_product_exact(S, inv.unsqueeze(1).expand_as(S), "S inv")
    # the backward's D inv, per entry
    _, inn, flat, _ = slots(c["row_ptr"], c["fields"], nf)
    D = c["dDeep"].double().reshape(-1, K)[flat][inn]
    assert_product_exact(D, inv[flat][inn].unsqueeze(1).expand_as(D),
                         "D inv")
    # x in {1, 2} and d = +-2^-s: the last multiply and d (s - e x) are exact
    assert set(c["vals"].tolist()) <= {1.0, 2.0}
    assert bool(((c["dpred"].abs().log2() % 1) == 0).all())
