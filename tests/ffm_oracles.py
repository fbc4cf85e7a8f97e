"""float64 oracles, builders and exact inputs for the FFM kernel parity
tests (``ffm_kernels.hip``). Plain helper module, sibling of
``kernel_oracles.py``; everything runs on the CPU. ``test_ffm_oracles.py``
(CPU) holds the oracles to ``ffm_ref`` and shows that the listed wrong
references differ on the inputs ``test_ffm_kernels_gpu.py`` uses.

Exact-input rule. The FFM operations are sums of products. On the exact
set every factor is a small integer times a power of two:

* V in {-2..2} (exact in fp32, bf16 and fp16), W in {-3..3}, x in {1, 2};
* dpred = +-1/scale with the block scale a power of two, so d * scale is
  +-1 and the emitted fp16 blocks hold integers (d = +-1 itself would push
  every non-zero element past fp16's largest finite value at scale 2^16);
* hand-built fp16 blocks for the apply kernels hold integers in {-4..4}.

Then every product and every partial sum, in any order, is an integer
multiple of one power of two, and it is exactly representable as long as

* fp32 accumulators: sum|term| < 2^24 (in units of that power of two);
* fp16 block elements: |sum over same-field partners| * scale <= 2048.

``assert_exact_fp32`` / ``assert_exact_fp16`` state these on the float64
side for every generated case, so an inexact case fails instead of passing
loosely. Under them any summation order, any atomic order, the fp16 stage,
the fp16 block and the bf16 mirror all give the float64 result exactly,
and the comparisons are ``check_bits`` / ``check_equal``.

The one sign caveat: a partner whose V element is 0 under a negative
coefficient is emitted as -0 by the direct (duplicate-free) path and as +0
by the accumulating path. ``check_equal`` therefore compares values (NaN
never equal); the slots that no partner feeds are compared bit for bit
against +0.
"""

from __future__ import annotations

import numpy as np
import torch

import kernel_oracles as ko

KS = (4, 8, 16, 32, 64)
F_TABLE = 4096
MAXN = 40            # staging cap of ffm_row_emit
APPLY_CHUNK = 64     # entries per wave, f16 and fp32 block apply
SORTED_CHUNK = 32    # entries per wave, sorted backward

# nfields per K for the D classes of ffm_blocks_apply_f16 (MAXQ = 1: D <=
# 256, 2: D <= 512, 4: D <= 1024), all eligible for the staged row emit
# (its LDS caps D near 560), plus nfields = 1 and nfields = 39.
SHAPES = {
    4: {"q1": 5, "q2": 70, "q4": 130, "nf1": 1, "nf39": 39},
    8: {"q1": 7, "q2": 40, "q4": 66, "nf1": 1, "nf39": 39},
    16: {"q1": 3, "q2": 20, "q4": 34, "nf1": 1, "nf39": 39},
    32: {"q1": 3, "q2": 10, "q4": 17, "nf1": 1, "nf39": 39},
    64: {"q1": 2, "q2": 5, "q4": 9, "nf1": 1, "nf39": 39},
}
ROW_KINDS = ("ordered", "shuffled", "dup1", "onefield", "samefid2f",
             "samefid1f")
# two batches of 9 rows: empty rows first, in the middle and last
LENGTHS_A = [0, 1, 2, 3, 7, 0, 8, 9, 11]
LENGTHS_B = [12, 16, 17, 39, 40, 41, 65, 131, 0]
BATCH_MIX = [9, 0, 41, 17, 1, 40, 0, 3, 12]  # first B rows, B in BATCHES


def row_emit_lds_bytes(nfields, K, maxn=MAXN, nwaves=8):
    """LDS footprint of ffm_row_emit (acc | stage | vals | fmap | flag)"""
    return (nwaves * nfields * (K + 1) * 4 + maxn * nfields * K * 2
            + maxn * 4 + nfields * 4 + 4)


def row_emit_eligible(nfields, K):
    return row_emit_lds_bytes(nfields, K) <= (64 << 10)


def maxq_of(D):
    return 1 if D <= 256 else (2 if D <= 512 else 4)


def check_equal(name, out, expect):
    """value equality with the float64 result cast to the output dtype
    (+-0 equal, NaN never)"""
    out = out.detach().cpu()
    assert out.dtype == expect.dtype, (name, out.dtype, expect.dtype)
    assert out.shape == expect.shape, (name, out.shape, expect.shape)
    ne = ~(out == expect)
    assert not ne.any(), (
        f"{name}: {int(ne.sum())} of {ne.numel()} elements differ, first "
        f"at flat index {int(ne.flatten().nonzero()[0])}")


def assert_exact_fp32(name, mag):
    """sum|term| < 2^24 (mag in units of the case's power of two)"""
    assert float(mag.max()) < 2.0 ** 24 if mag.numel() else True, \
        (name, float(mag.max()))


def assert_exact_fp16(name, blocks64, scale):
    """|sum over same-field partners| * scale <= 2048, and an integer"""
    s = blocks64 * scale
    assert float(s.abs().max()) <= 2048.0 if s.numel() else True, \
        (name, float(s.abs().max()))
    assert bool((s == s.round()).all()), name


# ---------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------
def make_ffm_csr(rows):
    """rows: list of lists of (fid, field, x) -> (row_ptr i32, fields i32,
    fids i32, vals f32)"""
    counts = torch.tensor([len(r) for r in rows], dtype=torch.int64)
    row_ptr = torch.zeros(len(rows) + 1, dtype=torch.int32)
    row_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    flat = [e for r in rows for e in r]
    fids = torch.tensor([e[0] for e in flat], dtype=torch.int32)
    fields = torch.tensor([e[1] for e in flat], dtype=torch.int32)
    vals = torch.tensor([float(e[2]) for e in flat], dtype=torch.float32)
    return row_ptr, fields, fids, vals


def make_row(n, nfields, kind, rng, F=F_TABLE, xs=(1.0, 2.0), float_x=False):
    """One row of n entries. Distinct fids except for the samefid kinds.
    'ordered' / 'shuffled': duplicate-free when n <= nfields (the direct
    emit path), fields ascending / shuffled; 'dup1': exactly one field
    used twice; 'onefield': every entry in one field; 'samefid2f' /
    'samefid1f': the first two entries share a fid, in two fields / in one
    field. Where a kind cannot be built (n > nfields, n < 2, nfields < 2)
    the fields are drawn at random."""
    fids = rng.choice(F, size=n, replace=False).tolist() if n else []
    free = n <= nfields
    if kind == "onefield":
        fl = [int(rng.integers(nfields))] * n
    elif kind in ("ordered", "shuffled") and free:
        fl = sorted(rng.choice(nfields, size=n, replace=False).tolist())
        if kind == "shuffled":
            rng.shuffle(fl)
    elif kind == "dup1" and 2 <= n <= nfields + 1:
        fl = rng.choice(nfields, size=n - 1, replace=False).tolist()
        fl.insert(int(rng.integers(n)), fl[int(rng.integers(n - 1))])
    elif kind in ("samefid2f", "samefid1f") and n >= 2:
        if free:
            fl = rng.choice(nfields, size=n, replace=False).tolist()
        else:
            fl = rng.integers(nfields, size=n).tolist()
        fids[1] = fids[0]
        if kind == "samefid1f":
            fl[1] = fl[0]
        elif fl[1] == fl[0]:
            fl[1] = (fl[0] + 1) % nfields
    else:
        fl = rng.integers(nfields, size=n).tolist()
    if float_x:
        x = (0.5 + rng.random(n)).tolist()
    else:
        x = rng.choice(xs, size=n).tolist()
    return list(zip(fids, fl, x))


def exact_tables(nfields, K, seed, F=F_TABLE, vmax=2, wmax=3):
    g = torch.Generator().manual_seed(seed)
    W = torch.randint(-wmax, wmax + 1, (F,), generator=g).float()
    V = torch.randint(-vmax, vmax + 1, (F, nfields, K), generator=g).float()
    return W, V


def exact_case(K, nfields, kind, lengths, seed, scale=1.0, vmax=2,
               xs=(1.0, 2.0)):
    """CSR + tables + dpred = +-1/scale on the exact set"""
    rng = np.random.default_rng(seed)
    rows = [make_row(n, nfields, kind, rng, xs=xs) for n in lengths]
    row_ptr, fields, fids, vals = make_ffm_csr(rows)
    W, V = exact_tables(nfields, K, seed + 1, vmax=vmax)
    sign = torch.tensor(rng.choice([-1.0, 1.0], size=len(lengths)),
                        dtype=torch.float32)
    return {"row_ptr": row_ptr, "fields": fields, "fids": fids,
            "vals": vals, "W": W, "V": V, "dpred": sign / scale,
            "nfields": nfields, "K": K, "scale": scale}


def float_case(K, nfields, lengths, seed):
    """the float set: V ~ 0.1 N(0,1), x in [0.5, 1.5], mixed row kinds"""
    rng = np.random.default_rng(seed)
    rows = [make_row(n, nfields, ROW_KINDS[i % len(ROW_KINDS)], rng,
                     float_x=True) for i, n in enumerate(lengths)]
    row_ptr, fields, fids, vals = make_ffm_csr(rows)
    g = torch.Generator().manual_seed(seed + 1)
    W = torch.randn(F_TABLE, generator=g) * 0.1
    V = torch.randn(F_TABLE, nfields, K, generator=g) * 0.1
    dpred = torch.randn(len(lengths), generator=g)
    return {"row_ptr": row_ptr, "fields": fields, "fids": fids,
            "vals": vals, "W": W, "V": V, "dpred": dpred,
            "nfields": nfields, "K": K, "scale": 1.0}


def make_runs(run_lengths, F, seed):
    """(sorted_fids i32, perm i32) straight from a list of run lengths:
    distinct random fids in ascending order, run i repeated
    run_lengths[i] times; perm is a random permutation of the entries."""
    g = torch.Generator().manual_seed(seed)
    nruns = len(run_lengths)
    fid = torch.sort(torch.randperm(F, generator=g)[:nruns]).values
    sorted_fids = torch.repeat_interleave(
        fid, torch.tensor(run_lengths)).to(torch.int32)
    perm = torch.randperm(int(sum(run_lengths)), generator=g).to(torch.int32)
    return sorted_fids, perm


def sort_entries(fids):
    """(sorted_fids i32, perm i32) of a CSR's fids, stable"""
    s, p = torch.sort(fids.long(), stable=True)
    return s.to(torch.int32), p.to(torch.int32)


def touched_words(fids, F):
    """the bitmap with exactly the bits of `fids` set, as int64 words"""
    words = np.zeros((F + 63) // 64, dtype=np.uint64)
    for f in torch.unique(fids.long()).tolist():
        words[f >> 6] |= np.uint64(1) << np.uint64(f & 63)
    return torch.from_numpy(words.view(np.int64).copy())


def bit_is_set(touched, f):
    return bool((int(touched[f >> 6]) >> (f & 63)) & 1)


# ---------------------------------------------------------------------------
# oracles
# ---------------------------------------------------------------------------
def ffm_forward_ref64(row_ptr, fields, fids, vals, W, V, mutant=None):
    """pred[r] = sum w x + sum_{i<j} x_i x_j <V[f_i, F_j], V[f_j, F_i]> in
    float64; also sum|term| over the n + K npairs terms and that count.
    Float-set bound (the sum rule): nterms 2^-23 sum|term|. A pair term is
    rounded three times (the product, then by x_i and x_j) where the rule
    allows one; a row with a pair has nterms >= K + 2 >= 6, and the rule's
    factor 2 (nterms u to spare) covers the two extra u.
    mutant 'droppair' leaves out the last pair of each row."""
    B = row_ptr.numel() - 1
    W, V, x = W.double(), V.double(), vals.double()
    K = V.shape[2]
    pred = torch.zeros(B, dtype=torch.float64)
    mag = torch.zeros(B, dtype=torch.float64)
    nterms = torch.zeros(B, dtype=torch.float64)
    for r in range(B):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        f, fl, xr = fids[lo:hi].long(), fields[lo:hi].long(), x[lo:hi]
        n = hi - lo
        lin = W[f] * xr
        pred[r], mag[r], nterms[r] = lin.sum(), lin.abs().sum(), n
        if n < 2:
            continue
        ii, jj = torch.triu_indices(n, n, offset=1)
        if mutant == "droppair":
            ii, jj = ii[:-1], jj[:-1]
        t = V[f[ii], fl[jj]] * V[f[jj], fl[ii]] * (xr[ii] * xr[jj])[:, None]
        pred[r] += t.sum()
        mag[r] += t.abs().sum()
        nterms[r] += t.numel()
    return pred, mag, nterms


def ffm_entry_blocks_ref(row_ptr, fields, fids, vals, V, dpred,
                         mutant=None):
    """Per entry p of a row with gradient d:
         gw[p] = d x_p
         block[p, F_j, :] += d x_p x_j V[f_j, F_p, :]   over j != p
    Returns float64 (gw [nnz], blocks [nnz, nf, K], mag = the same sums of
    |term|, npart [nnz, nf] = partners per field, cmag [nnz, nf] = the
    sum of |d x_p x_j| over them).
    mutants: 'droplastpartner' (each entry loses its last partner),
    'wrongslice' (V[f_j, F_j] for V[f_j, F_p]), 'dupdrop' (a partner whose
    field already occurred earlier in the row is dropped: a field map
    without the atomic fallback), 'self' (j = p included), 'dropmaxn'
    (partner at position maxn = 40 dropped), 'quadfield' (output quad u
    filled from field (4u+4)/K: the last quad of every field slice takes
    the next field's)."""
    nnz = fids.numel()
    _, nf, K = V.shape
    V64, x, d = V.double(), vals.double(), dpred.double()
    gw = torch.zeros(nnz, dtype=torch.float64)
    blocks = torch.zeros(nnz, nf, K, dtype=torch.float64)
    mag = torch.zeros(nnz, nf, K, dtype=torch.float64)
    npart = torch.zeros(nnz, nf, dtype=torch.float64)
    cmag = torch.zeros(nnz, nf, dtype=torch.float64)
    B = row_ptr.numel() - 1
    for r in range(B):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        n = hi - lo
        if n == 0:
            continue
        f, fl, xr = fids[lo:hi].long(), fields[lo:hi].long(), x[lo:hi]
        gw[lo:hi] = d[r] * xr
        keep = ~torch.eye(n, dtype=torch.bool)       # [p, j]
        if mutant == "self":
            keep[:] = True
        elif mutant == "droplastpartner":
            for p in range(n):
                js = keep[p].nonzero().flatten()
                if js.numel():
                    keep[p, js[-1]] = False
        elif mutant == "dupdrop":
            seen = set()
            for j in range(n):
                if int(fl[j]) in seen:
                    keep[:, j] = False
                seen.add(int(fl[j]))
        elif mutant == "dropmaxn" and n > MAXN:
            keep[:, MAXN] = False
        if mutant == "wrongslice":
            part = V64[f, fl][None, :, :].expand(n, n, K)
        else:
            part = V64[f[None, :], fl[:, None]]      # [p, j] = V[f_j, F_p]
        coef = d[r] * xr[:, None] * xr[None, :] * keep
        t = coef[:, :, None] * part
        blocks[lo:hi] = torch.zeros(n, nf, K, dtype=torch.float64) \
            .index_add_(1, fl, t)
        mag[lo:hi] = torch.zeros(n, nf, K, dtype=torch.float64) \
            .index_add_(1, fl, t.abs())
        npart[lo:hi] = torch.zeros(n, nf, dtype=torch.float64) \
            .index_add_(1, fl, keep.double())
        cmag[lo:hi] = torch.zeros(n, nf, dtype=torch.float64) \
            .index_add_(1, fl, coef.abs())
    if mutant == "quadfield":
        m = blocks.clone()
        m[:, :-1, K - 4:] = blocks[:, 1:, K - 4:]
        m[:, -1, K - 4:] = 0.0
        blocks = m
    return gw, blocks, mag, npart, cmag


def ffm_totals_ref(sorted_fids, perm, blocks, gw, F, inv_scale=1.0,
                   chunk=APPLY_CHUNK, mutant=None):
    """Per-fid totals of per-entry blocks [nnz, D] and gw [nnz], float64:
    (gradW [F], gradV [F, D], magW, magV). Entry e of the sorted order
    contributes blocks[perm[e]] * inv_scale to fid sorted_fids[e].
    mutants: 'droprunlast' (last entry of every run), 'dropchunkfirst'
    (entry e > 0 with e % chunk == 0), 'noinvscale', 'droplastquad' (the
    last four columns), 'dropgwtail' (gw of every run's last entry)."""
    sf, pm = sorted_fids.long(), perm.long()
    nnz, D = sf.numel(), blocks.shape[1]
    e = torch.arange(nnz)
    last = torch.ones(nnz, dtype=torch.bool)
    last[:-1] = sf[1:] != sf[:-1]
    useV = torch.ones(nnz, dtype=torch.bool)
    useW = torch.ones(nnz, dtype=torch.bool)
    if mutant == "droprunlast":
        useV &= ~last
        useW &= ~last
    elif mutant == "dropchunkfirst":
        first = (e > 0) & (e % chunk == 0)
        useV &= ~first
        useW &= ~first
    elif mutant == "dropgwtail":
        useW &= ~last
    b = blocks.double().reshape(nnz, D)[pm] * \
        (1.0 if mutant == "noinvscale" else inv_scale)
    if mutant == "droplastquad":
        b = b.clone()
        b[:, D - 4:] = 0.0
    w = gw.double()[pm]
    zV = lambda: torch.zeros(F, D, dtype=torch.float64)
    zW = lambda: torch.zeros(F, dtype=torch.float64)
    gradV = zV().index_add_(0, sf[useV], b[useV])
    gradW = zW().index_add_(0, sf[useW], w[useW])
    magV = zV().index_add_(0, sf, b.abs())
    magW = zW().index_add_(0, sf, w.abs())
    return gradW, gradV, magW, magV


def ffm_backward_totals_ref(c, mutant=None, total_mutant=None,
                            chunk=APPLY_CHUNK):
    """case dict -> (gradW, gradV, magW, magV): the totals of its
    per-entry blocks (unscaled) and of the |term| sums under them"""
    gw, blocks, mag, _, _ = ffm_entry_blocks_ref(
        c["row_ptr"], c["fields"], c["fids"], c["vals"], c["V"], c["dpred"],
        mutant=mutant)
    nnz, F = c["fids"].numel(), c["V"].shape[0]
    sf, pm = sort_entries(c["fids"])
    gradW, gradV, magW, _ = ffm_totals_ref(
        sf, pm, blocks.reshape(nnz, -1), gw, F, chunk=chunk,
        mutant=total_mutant)
    magV = ffm_totals_ref(sf, pm, mag.reshape(nnz, -1), gw, F)[1]
    return gradW, gradV, magW, magV


# ---------------------------------------------------------------------------
# float-set bound of ffm_row_emit
# ---------------------------------------------------------------------------
U11 = 2.0 ** -11       # fp16 unit roundoff
F16_SUBNORMAL = 2.0 ** -24


def row_emit_bound(mag, npart, cmag, scale, v_is_fp32):
    """Per element of the emitted fp16 block (value out/scale against the
    float64 block), from sum|term| = mag and the partner count m = npart:

      staging   one fp16 rounding of each staged V element (fp32 V only;
                a bf16 V is staged raw): 2^-11 mag, plus half an fp16
                subnormal step per element that is subnormal in fp16,
                times its coefficient: 2^-25 cmag
      chain     d x_p x_j scale and the product with v: 3 fp32 roundings
                per term, 3 2^-24 mag
      reduce    m terms accumulated in fp32 in any order (the atomic
                path): the run-length sum rule m 2^-23 mag
      store     one fp16 rounding of the stored value, at most 2^-11 of
                its magnitude <= mag (1 + the above), plus half an fp16
                subnormal step where it is subnormal, divided by scale
    Rows longer than maxn read V unstaged, which only removes the first
    term. Nothing here is measured."""
    m = npart.unsqueeze(-1)
    pre = ((U11 if v_is_fp32 else 0.0) + 3 * ko.U24 + m * ko.U23) * mag
    if v_is_fp32:
        pre = pre + 0.5 * F16_SUBNORMAL * cmag.unsqueeze(-1)
    return pre + U11 * (mag + pre) + 0.5 * F16_SUBNORMAL / scale


def scale_last_x_until(c, differs_enough, limit=2.0 ** 12):
    """double the last entry's x of every row with at least two entries
    until `differs_enough(case)` holds (what colsum does with its last
    row); returns the case"""
    rp = c["row_ptr"].long()
    last = (rp[1:] - 1)[(rp[1:] - rp[:-1]) >= 2]
    s = 1.0
    while not differs_enough(c):
        s *= 2.0
        assert s <= limit, "mutant stays inside the bound at any scale"
        c = dict(c)
        c["vals"] = c["vals"].clone()
        c["vals"][last] *= 2.0
    return c


# ---------------------------------------------------------------------------
# shared cases (the GPU tests and the CPU mutation tests build the same)
# ---------------------------------------------------------------------------
BATCHES = (1, 3, 4, 5, 9)
SCALES = (1.0, 128.0, 65536.0)


def shape_names(K, row_emit=False):
    """shape names of SHAPES[K]; with row_emit only the eligible ones
    (nfields = 39 fits the staged emit's LDS at K = 4 and 8 only)"""
    return [s for s, nf in SHAPES[K].items()
            if not row_emit or row_emit_eligible(nf, K)]


def case_seed(K, shape, kind, extra=0):
    return (1000 * K + 100 * list(SHAPES[K]).index(shape)
            + 10 * ROW_KINDS.index(kind) + extra)


def exact_cases(K, shape, kind, scale=1.0):
    """the two 9-row batches of one (K, D class, row kind) combination.
    At scale 2^16 the value set narrows to V in {-1, 0, 1}, x = 1."""
    nf = SHAPES[K][shape]
    narrow = scale >= 65536.0
    for i, ls in enumerate((LENGTHS_A, LENGTHS_B)):
        yield exact_case(K, nf, kind, ls, case_seed(K, shape, kind, i),
                         scale=scale, vmax=1 if narrow else 2,
                         xs=(1.0,) if narrow else (1.0, 2.0))


def batch_case(K, B):
    """first B rows of BATCH_MIX with the row kinds cycling, MAXQ 2 shape"""
    nf = SHAPES[K]["q2"]
    rng = np.random.default_rng(7000 + 10 * K + B)
    rows = [make_row(n, nf, ROW_KINDS[i % len(ROW_KINDS)], rng)
            for i, n in enumerate(BATCH_MIX[:B])]
    row_ptr, fields, fids, vals = make_ffm_csr(rows)
    W, V = exact_tables(nf, K, 7001 + 10 * K + B)
    sign = torch.tensor(rng.choice([-1.0, 1.0], size=B), dtype=torch.float32)
    return {"row_ptr": row_ptr, "fields": fields, "fids": fids,
            "vals": vals, "W": W, "V": V, "dpred": sign, "nfields": nf,
            "K": K, "scale": 1.0}


def long_row_case(n=1000, K=4, nfields=5):
    """one row of n entries, V in {-1, 0, 1}, x = 1: n (n-1)/2 pairs of K
    terms each of magnitude <= 1, 1,998,000 < 2^24 at n = 1000, K = 4"""
    return exact_case(K, nfields, "shuffled", [n], 4242, vmax=1, xs=(1.0,))


# run lists for the apply kernels (chunk 64): every length of 1, 2, 3, 63,
# 64, 65, 128, 129, 200; a run that ends exactly on a chunk boundary
# followed by one that starts on it; total nnz 1, 2, 63, 64, 65, 255, 256,
# 257
RUNS = {
    "n1": [1], "n2": [2], "n63": [63], "n64": [64], "n65": [65],
    "n255": [63, 1, 64, 127], "n256": [64, 64, 128], "n257": [65, 63, 129],
    "mix": [3, 61, 64, 65, 63, 128, 1, 129, 2, 200, 1, 1, 5],
}
# chunk 32 for the sorted walk
SORTED_RUNS = [31, 1, 32, 33, 31, 70, 2]
APPLY_DS = (4, 252, 256, 260, 508, 512, 516, 1020, 1024)
FUSED_DS = (48, 256, 260, 312, 512, 516, 1024)
APPLY_F = 1024
APPLY_INV_SCALE = 1.0 / 128.0


def apply_inputs(D, runs_name, F=APPLY_F):
    """hand-built integer blocks for ffm_blocks_apply_f16: fp16 blocks in
    {-4..4}, gw in +-{1, 2, 3}, inv_scale = 2^-7. Sums over a run of at most
    200 entries stay below 2^10 in magnitude: exact in fp32."""
    runs = RUNS[runs_name]
    seed = 9000 + 31 * D + list(RUNS).index(runs_name)
    sorted_fids, perm = make_runs(runs, F, seed)
    g = torch.Generator().manual_seed(seed + 1)
    nnz = int(sum(runs))
    gblocks = torch.randint(-4, 5, (nnz, D), generator=g).to(torch.float16)
    gw = (torch.randint(1, 4, (nnz,), generator=g)
          * (torch.randint(0, 2, (nnz,), generator=g) * 2 - 1)).float()
    return {"sorted_fids": sorted_fids, "perm": perm, "gblocks": gblocks,
            "gw": gw, "inv_scale": APPLY_INV_SCALE, "F": F, "D": D}


def csr_from_runs(run_lengths, nfields, K, seed, F=F_TABLE):
    """an exact CSR whose fid-sorted order has exactly these run lengths:
    run i's fid appears once in each of run_lengths[i] different rows"""
    rng = np.random.default_rng(seed)
    B = max(run_lengths)
    fid = rng.choice(F, size=len(run_lengths), replace=False)
    rows = [[] for _ in range(B)]
    for f, ln in zip(fid, run_lengths):
        for r in rng.choice(B, size=ln, replace=False):
            rows[r].append((int(f), int(rng.integers(nfields)),
                            float(rng.choice([1.0, 2.0]))))
    row_ptr, fields, fids, vals = make_ffm_csr(rows)
    W, V = exact_tables(nfields, K, seed + 1, F=F)
    sign = torch.tensor(rng.choice([-1.0, 1.0], size=B), dtype=torch.float32)
    return {"row_ptr": row_ptr, "fields": fields, "fids": fids,
            "vals": vals, "W": W, "V": V, "dpred": sign, "nfields": nfields,
            "K": K, "scale": 1.0}


FLOAT_LENGTHS = [0, 1, 2, 9, 17, 40, 41, 65, 3]


def float_emit_case(K):
    """the float-set case of one K (MAXQ 2 shape). The last entry's x of
    every row is doubled until the dropped-partner and the wrong-slice
    references leave the row-emit bound for both V types."""
    nf = SHAPES[K]["q2"]

    def caught(c):
        for v_is_fp32 in (True, False):
            V = c["V"] if v_is_fp32 else c["V"].to(torch.bfloat16).float()
            args = (c["row_ptr"], c["fields"], c["fids"], c["vals"], V,
                    c["dpred"])
            _, ref, mag, npart, cmag = ffm_entry_blocks_ref(*args)
            bound = row_emit_bound(mag, npart, cmag, 1.0, v_is_fp32)
            for m in ("droplastpartner", "wrongslice"):
                if not ko.differs(ffm_entry_blocks_ref(*args, mutant=m)[1],
                                  ref, bound):
                    return False
        return True

    return scale_last_x_until(float_case(K, nf, FLOAT_LENGTHS, 8000 + K),
                              caught)
