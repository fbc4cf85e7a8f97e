"""float64 oracles, exact-arithmetic inputs and derived bounds for the FM
kernel parity tests (forward, training forward, loss, atomic backward, emit,
sorted apply in every chunk mode, fused walk, sparse optimizers, list-fed
and tile-local segment reduces).

Plain helper module (imported like ``kernel_oracles``); everything here runs
on the CPU. ``test_fm_kernels_gpu.py`` feeds these inputs to the kernels and
``test_fm_oracles.py`` (CPU) holds the oracles to ``fm_ref``, checks the
exactness conditions of every case list, and shows that every wrong
reference listed there is caught on the same inputs.

Exact-input rule. Every FM quantity except the loss is a sum of products.
With V in {-2..2}, W in {-3..3}, x in {1, 2} and dpred = +-2^-s per row
every product and every partial sum in any order, tiling or atomic
interleaving is an integer multiple of 2^-s below 2^24 in magnitude, hence
exact in fp32, and the kernel has to reproduce the float64 result exactly.
``assert_exact`` checks the magnitudes on the float64 side of each case and
fails the case (it never passes loosely) when one is too large.

Comparisons on the exact set:

* bit-level (``check_bits``) for pred, sumVX, gw, rec, the slab totals and
  every tensor an op must leave alone;
* value-level (``check_value``) in two places only. Per-entry gv: the
  kernel forms d (s - v x) x, and a negative d times a zero bracket is -0
  while the oracle may hold +0. Totals out of an accumulator that started at
  +0: (+0) + (-0) = +0, so a reference -0 is folded. Both compare equal as
  values; any other difference, NaN included, fails.

On the float set the bounds follow the tolerance rule of ``kernel_oracles``
and are derived next to each oracle.
"""

from __future__ import annotations

import numpy as np
import torch

from kernel_oracles import (U23, U24, adagrad_ref, check_bits,  # noqa: F401
                            check_bound, differs, f32, ftrl_ref,
                            length_cases, make_csr, poison, rows_pos)
from zoo_oracles import W2V_INTRINSIC_REL

KS = (4, 8, 16, 32, 64)
F_FM = 2048            # rows of the row-kernel tables; row F-1 is NaN
EXACT_LIMIT = 2.0 ** 24
PAD = 8                # ints / floats around the fids / vals views

ADAGRAD = dict(lr=1e-2, eps=1e-8, l2=1e-4)
FTRL = dict(alpha=0.15, beta=1.0, l1=1e-2, l2=1e-4)
V_ADAGRAD = dict(lr=5e-2, eps=1e-8, l2=1e-5)


# ---------------------------------------------------------------------------
# comparison helpers
# ---------------------------------------------------------------------------
def check_value(name, out, ref64):
    """Equality as values with the float64 result cast to fp32 (+0 == -0;
    NaN equals nothing). The reference must be representable, i.e. the case
    must be exact."""
    out = out.detach().cpu()
    assert out.dtype == torch.float32, (name, out.dtype)
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64), f"{name}: inexact reference"
    ref32 = ref32.reshape(out.shape)
    ne = ~(out == ref32)
    assert not ne.any(), (
        f"{name}: {int(ne.sum())} of {ne.numel()} elements differ, first at "
        f"flat index {int(ne.flatten().nonzero()[0])}")


def exact32(ref64):
    """fp32 image of an exactly representable float64 tensor, with -0
    folded to +0 (the value an accumulator that started at +0 holds)."""
    r = ref64.float()
    assert torch.equal(r.double(), ref64), "inexact reference"
    return r + 0.0


def fid_words(fids, F):
    """the touched bitmap of a batch: int64 [ceil(F/64)], bit f%64 of word
    f/64 set for every fid f that occurs"""
    words = np.zeros((F + 63) // 64, dtype=np.uint64)
    for f in np.unique(np.asarray(fids, dtype=np.int64)):
        words[f >> 6] |= np.uint64(1) << np.uint64(f & 63)
    return torch.from_numpy(words.view(np.int64).copy())


def words_to_fids(words):
    """inverse of fid_words: sorted int64 fids"""
    w = words.detach().cpu().numpy().view(np.uint64)
    out = [i * 64 + b for i in range(len(w)) for b in range(64)
           if (int(w[i]) >> b) & 1]
    return torch.tensor(out, dtype=torch.int64)


def padded(t, fill):
    """(buffer, offset): t inside a longer buffer whose surroundings hold
    `fill`; the GPU test uploads the buffer and hands the kernel the view
    [offset, offset + len), so a read one past either end reaches `fill`"""
    buf = torch.full((t.numel() + 2 * PAD,), fill, dtype=t.dtype)
    buf[PAD:PAD + t.numel()] = t
    return buf, PAD


# ---------------------------------------------------------------------------
# row-kernel oracles (forward, emit, totals), written from the definitions
# ---------------------------------------------------------------------------
def _keep_mask(row_ptr, K, mutant):
    row, pos, counts = rows_pos(row_ptr)
    keep = torch.ones(row.numel(), dtype=torch.bool)
    if mutant == "droplast":
        keep = pos != (counts[row] - 1)
    elif mutant == "drop4G":
        keep = pos != 4 * (64 // K)
    return row, keep


def fm_forward_ref(row_ptr, fids, vals, W, V, mutant=None):
    """pred = sum w x + 1/2 (sum_k (sum_j v_jk x_j)^2 - sum_jk (v_jk x_j)^2)
    and sumVX in float64, with their float-set bounds.

    sumVX_k: the sum rule, n 2^-23 A_k with A_k = sum_j |v_jk x_j|.
    pred: per k, 1/2 (s_k^2 - q_k) carries n 2^-23 (|s_k| A_k + q_k) exactly
    as derived for ``nfm_forward_ref``'s vec (s_k from an n-term sum, q_k an
    n-term sum of twice-rounded squares; a lane's chain is at most n long).
    The kernel then adds the 64 lane values of s^2 (each k held G = 64/K
    times, the total scaled by the exact 1/G) and of the q partials with a
    wave butterfly: the sum rule with 64 terms on 1/2 (T + Q), T = sum s_k^2,
    Q = sum q_k. The linear part is an n-term sum (fma chain and the same
    butterfly): (n + 64) 2^-23 sum|w x|. The last two additions round on
    |lin| + 1/2 (T + Q).

    mutants: 'droplast' / 'drop4G' lose the last entry / the entry at
    position 4G of every row; 'nohalf'; 'lin_all' takes sum w x from every
    lane (K times); 'droplane' loses lane K-1; 'noG' sums the squares G
    times without the 1/G."""
    K = V.shape[1]
    G = 64 // K
    row, keep = _keep_mask(row_ptr, K, mutant)
    B = row_ptr.numel() - 1
    n = (row_ptr.long()[1:] - row_ptr.long()[:-1]).double()
    f = fids.long()
    x = torch.where(keep, vals.double(), torch.zeros(1, dtype=torch.float64))
    wx = W.double()[f] * x
    vx = V.double()[f] * x.unsqueeze(1)
    z1 = lambda: torch.zeros(B, dtype=torch.float64)  # noqa: E731
    zk = lambda: torch.zeros(B, K, dtype=torch.float64)  # noqa: E731
    s = zk().index_add_(0, row, vx)
    A = zk().index_add_(0, row, vx.abs())
    q = zk().index_add_(0, row, vx * vx)
    lin = z1().index_add_(0, row, wx)
    alin = z1().index_add_(0, row, wx.abs())
    if mutant == "droplane":
        s[:, K - 1] = 0
        q[:, K - 1] = 0
    T, Q = (s * s).sum(1), q.sum(1)
    half = 1.0 if mutant == "nohalf" else 0.5
    if mutant == "noG":
        T = T * G
    if mutant == "lin_all":
        lin = lin * K
    pred = lin + half * (T - Q)
    nk = n.unsqueeze(1)
    has = (n > 0).double()
    pred_b = (n * U23 * (s.abs() * A + q).sum(1)
              + has * 64 * U23 * 0.5 * (T + Q)
              + (n + 64) * has * U23 * alin
              + has * 2 * U24 * (alin + 0.5 * (T + Q)))
    return {"pred": (pred, pred_b), "sumVX": (s, nk * U23 * A),
            "T": T, "Q": Q, "alin": alin}


def fm_emit_ref(row_ptr, fids, vals, V, sumVX, dpred, mutant=None):
    """Per-entry gw_j = d x_j and gv_jk = d (sumVX_k - v_jk x_j) x_j in
    float64 from the sumVX and dpred handed to the kernel.

    gw is one fp32 multiply: on the float set it is compared bit for bit
    with that multiply. gv has four roundings (v x, the subtraction, two
    multiplies), 2^-24 each to first order: the first two are absolute,
    u|vx| and u(|s| + |vx|), scaled by |d x|; the multiplies add
    2u|gv| <= 2u|d x|(|s| + |vx|). Bound 4u |d x| (|s| + |vx|).
    mutant 'noself' omits -v x."""
    row, _, _ = rows_pos(row_ptr)
    x = vals.double()
    d = dpred.double()[row]
    vx = V.double()[fids.long()] * x.unsqueeze(1)
    sv = sumVX.double()[row]
    inner = sv if mutant == "noself" else sv - vx
    dx = (d * x).unsqueeze(1)
    gw = d * x
    gv = dx * inner
    bound = 4 * U24 * dx.abs() * (sv.abs() + vx.abs())
    return gw, gv, bound


def fid_totals(fids, gw, gv, F, gv_bound=None):
    """Per-fid totals of per-entry gradients in float64: (gradW [F],
    gradV [F, K], bounds or None). Float set: the entries' own bounds add
    up, and m once-rounded terms accumulated in any order (atomics, scans,
    pieces) add m 2^-23 sum|term| (sum rule)."""
    f = fids.long()
    K = gv.shape[1]
    gW = torch.zeros(F, dtype=torch.float64).index_add_(0, f, gw.double())
    gV = torch.zeros(F, K, dtype=torch.float64).index_add_(0, f, gv.double())
    if gv_bound is None:
        return gW, gV, None
    m = torch.zeros(F, dtype=torch.float64).index_add_(
        0, f, torch.ones(f.numel(), dtype=torch.float64))
    aW = torch.zeros(F, dtype=torch.float64).index_add_(
        0, f, gw.double().abs())
    aV = torch.zeros(F, K, dtype=torch.float64).index_add_(
        0, f, gv.double().abs())
    eV = torch.zeros(F, K, dtype=torch.float64).index_add_(0, f, gv_bound)
    # gw_j is rounded once (u|gw_j|) before it is summed
    return gW, gV, (m * U23 * aW + U24 * aW,
                    eV + m.unsqueeze(1) * U23 * aV)


# ---------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------
def logloss_ref(z, y, scale, mutant=None):
    """loss = max(z, 0) - z y + log(1 + exp(-|z|)) and
    dpred = (sigmoid(clamp(z, +-16)) - y) scale in float64 with bounds, for
    z exact in fp32 and y in {0, 1} (then max(z, 0) - z y is exact).

    loss: the kernel's __logf(1 + __expf(-|z|)) is the composition
    -__logf(1 / (1 + __expf(-dot))) whose deviation W2V_INTRINSIC_REL bounds
    in this project; it enters as the absolute error of the log term L.
    The two fp32 additions add 2^-24 of |a| and of |a| + L, a = max(z, 0)
    - z y.
    dpred: the clamped-sigmoid bound of ``gemm_epilogue_ref``,
    (|zc| + 3) 2^-23 sigma, one rounding for sigma - y and one for the
    product with the fp32 scale.
    mutants: 'noscale' (dpred without the scale); 'clamped_loss' forms the
    loss from z clamped to +-16 as dpred's sigmoid is (the kernel's loss has
    no clamp: at |z| = 20 the two differ by 4)."""
    scale = f32(scale)
    z, y = z.double(), y.double()
    zl = z.clamp(-16, 16) if mutant == "clamped_loss" else z
    a = zl.clamp(min=0) - zl * y
    L = torch.log1p(torch.exp(-zl.abs()))
    loss = a + L
    loss_b = W2V_INTRINSIC_REL + U24 * a.abs() + U24 * (a.abs() + L)
    zc = z.clamp(-16, 16)
    sig = torch.sigmoid(zc)
    sc = 1.0 if mutant == "noscale" else scale
    d = (sig - y) * sc
    d_b = scale * ((zc.abs() + 3) * U23 * sig + U24 * (sig - y).abs()) \
        + U24 * d.abs()
    return {"loss": (loss, loss_b), "dpred": (d, d_b)}


LOSS_SCALE = 1.0 / 278


def loss_sweep():
    """z = -17, -16.75, ..., 17 and +-20, each with y = 0 and y = 1, as
    (z, y) and as the one-entry rows that make the forward produce them:
    row i holds fid i with W = z_i, x = 1 and V = 0, so pred = z exactly."""
    zs = torch.cat([torch.arange(-68, 69).float() / 4,
                    torch.tensor([-20.0, 20.0])])
    z = zs.repeat_interleave(2)
    y = torch.tensor([0.0, 1.0]).repeat(zs.numel())
    B = z.numel()
    return {
        "z": z, "y": y, "scale": LOSS_SCALE,
        "row_ptr": torch.arange(B + 1, dtype=torch.int32),
        "fids": torch.arange(B, dtype=torch.int32),
        "vals": torch.ones(B),
        "W": torch.cat([z, torch.tensor([float("nan")])]),
    }


# ---------------------------------------------------------------------------
# exact and float row cases
# ---------------------------------------------------------------------------
def row_case(K, lengths, seed, exact=True, s=3, small=False, dup_row=None,
             common=False, boost=1.0):
    """One CSR batch with its tables. exact: V in {-2..2}, W in {-3..3},
    x in {1, 2}, dpred = +-2^-s (small: V in {-1, 0, 1}, x = 1, for rows
    of a thousand entries). float: V ~ 0.1 N(0, 1), W ~ N(0, 1), x in
    [0.5, 1.5], dpred ~ N(0, 1) / B; `boost` scales x of the last entry and
    of the entry at position 4G of every row (see float_boost).
    Fids are below F-1; row F-1 of W and V is NaN (the padding around the
    fids view names it). dup_row repeats a fid inside that row; common puts
    fid 7 first in every non-empty row."""
    g = torch.Generator().manual_seed(seed)
    F = F_FM
    row_ptr, fids, vals = make_csr(lengths, F=F - 1, seed=seed,
                                   dup_row=dup_row)
    row, pos, counts = rows_pos(row_ptr)
    B, nnz = len(lengths), fids.numel()
    if common:
        fids[pos == 0] = 7
    if exact:
        hi = 1 if small else 2
        V = torch.randint(-hi, hi + 1, (F, K), generator=g).float()
        W = torch.randint(-3, 4, (F,), generator=g).float()
        vals = torch.ones(nnz) if small else \
            torch.randint(1, 3, (nnz,), generator=g).float()
        sign = torch.randint(0, 2, (B,), generator=g).float() * 2 - 1
        dpred = sign * 2.0 ** -s
    else:
        V = torch.randn(F, K, generator=g) * 0.1
        W = torch.randn(F, generator=g)
        edge = (pos == counts[row] - 1) | (pos == 4 * (64 // K))
        vals = torch.where(edge, vals * boost, vals)
        dpred = torch.randn(B, generator=g) / max(B, 1)
    V[F - 1] = float("nan")
    W[F - 1] = float("nan")
    label = torch.randint(0, 2, (B,), generator=g).float()
    return {"K": K, "F": F, "B": B, "row_ptr": row_ptr, "fids": fids,
            "vals": vals, "W": W, "V": V, "dpred": dpred, "label": label,
            "exact": exact, "s": s}


def row_cases(K):
    """The exact row cases of one K: the loop-edge lengths and the
    rows-per-block sweep of ``length_cases`` (empty rows first, in the
    middle, last), adjacent empty rows, one fid twice in a row, one fid in
    every row, and the long rows 130 / 1000 on the small value set."""
    G = 64 // K
    out = []
    for i, (ls, seed) in enumerate(length_cases(K, base=7000)):
        dup = ls.index(max(ls)) if i == 0 else None
        out.append(row_case(K, ls, seed, s=2 + i, dup_row=dup))
    out.append(row_case(K, [0, 0, G + 1, 0, 0, 39, 2, 0, 0], 7900 + K, s=5))
    out.append(row_case(K, [3, 1, 4 * G + 1, 0, 39, 2, G], 7950 + K, s=1,
                        common=True))
    out.append(row_case(K, [130, 0, 1000, 1, 130], 7990 + K, s=4,
                        small=True))
    return out


FLOAT_BOOST = 1.0


def float_row_case(K, boost=FLOAT_BOOST):
    from kernel_oracles import length_set
    return row_case(K, length_set(K) + [130, 1000], 8100 + K, exact=False,
                    boost=boost)


def case_sumvx32(c):
    """the sumVX a backward is handed: the float64 value cast to fp32
    (exact on the exact set)"""
    fw = fm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"], c["V"])
    return fw["sumVX"][0].float()


def _mx(t):
    return float(t.max()) if t.numel() else 0.0


def assert_exact(c):
    """Exactness conditions of one exact row case (see the module text).
    Per row, G = 64/K: G sum_k sumVX_k^2 < 2^24 (the wave butterfly adds
    every square G times before the 1/G), sum (v x)^2 < 2^24,
    sum |w x| < 2^24, and the final |lin| + |T - Q| < 2^24. Per fid and k:
    sum |term| / |d| < 2^24 for both totals."""
    assert c["exact"]
    K = c["K"]
    G = 64 // K
    fw = fm_forward_ref(c["row_ptr"], c["fids"], c["vals"], c["W"], c["V"])
    s = fw["sumVX"][0]
    assert _mx(G * fw["T"]) < EXACT_LIMIT, "G sum s^2"
    assert _mx(fw["Q"]) < EXACT_LIMIT, "sum (v x)^2"
    assert _mx(fw["alin"]) < EXACT_LIMIT, "sum |w x|"
    assert _mx(fw["alin"] + fw["T"] + fw["Q"]) \
        < EXACT_LIMIT, "pred"
    assert torch.equal(s.float().double(), s)
    gw, gv, _ = fm_emit_ref(c["row_ptr"], c["fids"], c["vals"], c["V"],
                            s.float(), c["dpred"])
    d = 2.0 ** -c["s"]
    aW, aV, _ = fid_totals(c["fids"], gw.abs(), gv.abs(), c["F"])
    assert _mx(aW) / d < EXACT_LIMIT, "gradW total"
    assert _mx(aV) / d < EXACT_LIMIT, "gradV total"
    for t in (gw, gv):
        assert torch.equal(t.float().double(), t)


# ---------------------------------------------------------------------------
# sorted streams built from run lengths
# ---------------------------------------------------------------------------
def runs_stream(runs, seed):
    """sorted_fids (int32) of distinct increasing fids with the given run
    lengths, and F: gaps of 1..3 between fids, fid 0 in use, F-1 unused."""
    g = torch.Generator().manual_seed(seed)
    runs = [r for r in runs if r > 0]
    gaps = torch.randint(1, 4, (len(runs),), generator=g)
    gaps[0] = 0
    ids = torch.cumsum(gaps, 0)
    sorted_fids = torch.repeat_interleave(
        ids, torch.tensor(runs, dtype=torch.int64)).to(torch.int32)
    return sorted_fids, int(ids[-1]) + 2


def place_at(units):
    """Runs that put, for every unit b in `units` (ascending), a run of 3
    ending exactly on a multiple of b followed by a run of 5 starting on
    it. Fillers are runs of their own fids."""
    runs, pos = [], 0
    for b in units:
        fill = (-(pos + 3)) % b
        if fill:
            runs.append(fill)
        runs += [3, 5]
        pos += fill + 8
    return runs


def _uniq_pos(xs):
    out = []
    for x in xs:
        if x > 0 and x not in out:
            out.append(x)
    return out


def walk_runs(K, chunk):
    """Run list of the walk at `chunk` entries per wave: every K-lane
    subgroup gets sub = ceil(chunk / G) consecutive entries and works in
    batches of 8 (16 for the two-deep body). Boundary placements first (a
    run ending on / starting on a sub-chunk and a chunk boundary, inside the
    first chunks), then 1, 2, 7, 8, 9, 15, 16, 17, sub-1, sub, sub+1,
    chunk-1, chunk, chunk+1, 2 chunk + 3 and one run of 4 chunk + 1, which
    leaves the four-wave block."""
    G = 64 // K
    sub = (chunk + G - 1) // G
    return place_at(sorted({sub, chunk})) + _uniq_pos(
        [1, 2, 7, 8, 9, 15, 16, 17, sub - 1, sub, sub + 1, chunk - 1, chunk,
         chunk + 1, 2 * chunk + 3, 4 * chunk + 1])


def scan_runs(epw):
    """Run list of the segmented scans, `epw` entries per wave."""
    return place_at([epw]) + _uniq_pos(
        [1, epw - 1, epw, epw + 1, 2 * epw + 1, 200])


def apply_units(K, chunk):
    """(kind, unit) of fm_sorted_apply's route at a chunk argument: the
    lane-per-entry scan (-1, K <= 16: 64 entries per wave), the quad scan
    (-2: 256 / K), otherwise the walk (0, -3, -4 and -1 at K = 32 / 64:
    chunk 384)."""
    if chunk == -2:
        return "scan", 256 // K
    if chunk == -1 and K <= 16:
        return "scan", 64
    return "walk", (chunk if chunk > 0 else 384)


APPLY_CHUNKS = (0, -3, -4, -1, -2, 8, 64, 384)


def apply_case(K, chunk, seed, nnz=None, with_perm=True):
    """Hand-built integer per-entry gradients (in {-3..3}) behind a sorted
    stream for fm_sorted_apply. nnz=None: the route's run list; otherwise a
    stream of that many entries in runs of 1..3. perm is a random
    permutation (gw / gv live in CSR order) or None (sorted order)."""
    kind, unit = apply_units(K, chunk)
    g = torch.Generator().manual_seed(seed)
    if nnz is None:
        runs = walk_runs(K, unit) if kind == "walk" else scan_runs(unit)
    else:
        runs, left = [], nnz
        while left > 0:
            r = min(left, 1 + len(runs) % 3)
            runs.append(r)
            left -= r
    sorted_fids, F = runs_stream(runs, seed)
    n = sorted_fids.numel()
    gw_s = torch.randint(-3, 4, (n,), generator=g).float()
    gv_s = torch.randint(-3, 4, (n, K), generator=g).float()
    c = {"K": K, "F": F, "sorted_fids": sorted_fids, "unit": unit,
         "kind": kind, "gw_sorted": gw_s, "gv_sorted": gv_s, "runs": runs}
    if with_perm:
        perm = torch.randperm(n, generator=g).to(torch.int32)
        gw = torch.empty(n)
        gv = torch.empty(n, K)
        gw[perm.long()] = gw_s
        gv[perm.long()] = gv_s
        c.update(perm=perm, gw=gw, gv=gv)
    else:
        c.update(perm=None, gw=gw_s, gv=gv_s)
    return c


def apply_nnz_cases(K, chunk):
    _, unit = apply_units(K, chunk)
    return _uniq_pos([1, 2, 63, 64, 65, unit - 1, unit + 1])


def run_bounds(sorted_fids):
    """(fid, start, end) of every run of a sorted stream, as int64 arrays"""
    f = sorted_fids.long().numpy()
    n = f.size
    heads = np.flatnonzero(np.r_[True, f[1:] != f[:-1]])
    ends = np.r_[heads[1:], n]
    return f[heads], heads, ends


def apply_totals(c, mutant=None, unit=None):
    """Exact float64 per-fid totals of an apply case: (gradW, gradV).
    mutants: 'noperm' reads gw / gv without the permutation; 'droplast'
    loses the last entry of every run; 'dropfirst' the first entry after
    every multiple of `unit` (a chunk, sub-chunk, cap or tile boundary);
    'head_owned' takes a run whose head lies in the previous unit as owned
    by the unit that holds its tail: the store overwrites what the earlier
    part added, and only the entries from the last boundary on remain."""
    sf = c["sorted_fids"]
    n, F = sf.numel(), c["F"]
    if mutant == "noperm":
        gw, gv = c["gw"], c["gv"]
    else:
        gw, gv = c["gw_sorted"], c["gv_sorted"]
    keep = torch.ones(n, dtype=torch.bool)
    idx = torch.arange(n)
    _, heads, ends = run_bounds(sf)
    if mutant == "droplast":
        keep[torch.from_numpy(ends - 1)] = False
    elif mutant == "dropfirst":
        keep = (idx % unit != 0) | (idx == 0)
    elif mutant == "head_owned":
        for a, b in zip(heads, ends):
            cut = ((b - 1) // unit) * unit
            if cut > a:
                keep[a:cut] = False
    gW, gV, _ = fid_totals(sf[keep], gw[keep], gv[keep], F)
    return gW, gV


# ---------------------------------------------------------------------------
# state, optimizer steps
# ---------------------------------------------------------------------------
def int_state(F, K, seed, ftrl):
    """Integer-valued parameters and optimizer state (n >= 0) plus NaN
    sentinels nowhere: every row may be read. zW / zV only under ftrl."""
    g = torch.Generator().manual_seed(seed)
    st = {"W": torch.randint(-3, 4, (F,), generator=g).float(),
          "V": torch.randint(-2, 3, (F, K), generator=g).float(),
          "nW": torch.randint(0, 5, (F,), generator=g).float(),
          "nV": torch.randint(0, 5, (F, K), generator=g).float()}
    if ftrl:
        st["zW"] = torch.randint(-2, 3, (F,), generator=g).float()
        st["zV"] = torch.randint(-2, 3, (F, K), generator=g).float()
    return st


def opt_step_ref(st, gW, gV, opt_mode, mutant=None):
    """One optimizer step of every row on the totals (gW [F], gV [F, K]):
    {name: (ref64, bound)} for W, V, nW, nV (+ zW, zV where the mode keeps
    them). opt_mode 1 = Adagrad, 2 = FTRL, 3 = FTRL on W + Adagrad on V with
    the V-side knobs; the arithmetic and bounds are ``adagrad_ref`` /
    ``ftrl_ref``."""
    out = {}
    if opt_mode == 1:
        r = adagrad_ref(st["W"], gW, st["nW"], **ADAGRAD, mutant=mutant)
        out["W"], out["nW"] = r["W"], r["n"]
    else:
        r = ftrl_ref(st["W"], st["zW"], st["nW"], gW, **FTRL, mutant=mutant)
        out["W"], out["zW"], out["nW"] = r["w"], r["z"], r["n"]
    if opt_mode == 2:
        r = ftrl_ref(st["V"], st["zV"], st["nV"], gV, **FTRL, mutant=mutant)
        out["V"], out["zV"], out["nV"] = r["w"], r["z"], r["n"]
    else:
        kn = ADAGRAD if opt_mode == 1 else V_ADAGRAD
        r = adagrad_ref(st["V"], gV, st["nV"], **kn, mutant=mutant)
        out["V"], out["nV"] = r["W"], r["n"]
    return out


def opt_args(opt_mode):
    """(p0, p1, p2, p3, v_lr, v_eps, v_l2) as the fused bindings take them"""
    if opt_mode == 1:
        p = (ADAGRAD["lr"], ADAGRAD["eps"], ADAGRAD["l2"], 0.0)
    else:
        p = (FTRL["alpha"], FTRL["beta"], FTRL["l1"], FTRL["l2"])
    return p + (V_ADAGRAD["lr"], V_ADAGRAD["eps"], V_ADAGRAD["l2"])


def ftrl_edge_gradients():
    """+-l1, +-l1/2, +-(1 + 2^-10) l1 in fp32: from zero state z' = g
    exactly, so the first four lie in the dead zone (w = +0 bit for bit, the
    first two exactly on its edge) and the last two just outside."""
    l1 = f32(FTRL["l1"])
    return torch.tensor([l1, -l1, 0.5 * l1, -0.5 * l1,
                         l1 * (1 + 2.0 ** -10), -l1 * (1 + 2.0 ** -10)])


SPARSE_F = 600


def sparse_case(K, n, seed, ftrl):
    """State for the sparse applies: n listed fids (0 and F-1 among them,
    the FTRL edge gradients on the first six when there are that many)
    followed by 5 more distinct fids behind the list view; gradients of
    1e-4 so that eps is visible."""
    g = torch.Generator().manual_seed(seed)
    F = SPARSE_F
    perm = torch.randperm(F - 2, generator=g) + 1
    body = perm[:max(n - 2, 0)]
    ends = torch.tensor([F - 1, 0])[:min(n, 2)]
    lst = torch.cat([body, ends])[:n]
    lst = lst[torch.randperm(n, generator=g)]
    tail = perm[n:n + 5]
    st = {"W": torch.randn(F, generator=g) * 0.1,
          "V": torch.randn(F, K, generator=g) * 0.1,
          "nW": torch.rand(F, generator=g) * 1e-8,
          "nV": torch.rand(F, K, generator=g) * 1e-8}
    gradW = torch.randn(F, generator=g) * 1e-4
    gradV = torch.randn(F, K, generator=g) * 1e-4
    if ftrl:
        st["zW"] = torch.zeros(F)
        st["zV"] = torch.zeros(F, K)
        st["W"].zero_()   # FTRL's closed form owns the weights
        if n >= 6:
            live = lst[:6]
            edge = ftrl_edge_gradients()
            for k in ("V", "nW", "nV"):
                st[k][live] = 0.0
            gradW[live] = edge
            gradV[live] = edge.unsqueeze(1).expand(6, K).contiguous()
    return {"K": K, "F": F, "list": lst.to(torch.int32),
            "tail": tail.to(torch.int32), "state": st, "gradW": gradW,
            "gradV": gradV}


def fused_case(K, seed, opt_mode):
    """fm_sorted_apply_fused input: the walk run list of chunk 384 (the
    chunk itself is not assumed by the test) behind six one-entry runs that
    carry the FTRL edge gradients onto zero state."""
    ftrl = opt_mode != 1
    c = apply_case(K, 0, seed, with_perm=True)
    edge = ftrl_edge_gradients()
    sf = c["sorted_fids"]
    last = int(sf[-1])
    extra = torch.arange(last + 1, last + 7, dtype=torch.int32)
    n0 = sf.numel()
    c["sorted_fids"] = torch.cat([sf, extra])
    c["F"] = last + 8
    F = c["F"]
    st = int_state(F, K, seed + 1, ftrl)
    for t in st.values():
        t[extra.long()] = 0.0
    gw_e = edge.clone()
    gv_e = edge.unsqueeze(1).expand(6, K).contiguous()
    c["gw_sorted"] = torch.cat([c["gw_sorted"], gw_e])
    c["gv_sorted"] = torch.cat([c["gv_sorted"], gv_e])
    c["gw"] = torch.cat([c["gw"], gw_e])
    c["gv"] = torch.cat([c["gv"], gv_e])
    c["perm"] = torch.cat([c["perm"],
                           torch.arange(n0, n0 + 6, dtype=torch.int32)])
    c["edge_fids"] = extra.long()
    c["state"] = st
    return c


# ---------------------------------------------------------------------------
# segment reduces: spill prediction, records
# ---------------------------------------------------------------------------
def segment_runs(cap):
    """Run list of the list-fed reduce at piece length `cap`: the head entry
    is added last and batches of D follow it. Placements at a multiple of
    cap first (a run ending there, one starting there), then 1, 2, 4, 5, 6,
    8, 9, 10 (around both depths), cap-1, cap, cap+1, 2 cap,
    2 cap + 1, 3 cap + 5."""
    return place_at([cap]) + _uniq_pos(
        [1, 2, 4, 5, 6, 8, 9, 10, cap - 1, cap, cap + 1, 2 * cap,
         2 * cap + 1, 3 * cap + 5])


def tile_runs(cap, T, S):
    """Run list of the tile reduce: tile T, longest unit S. Placements: a
    run starting on a multiple of S, one straddling the first tile
    boundary, a piece whose first unit ends exactly at the end of its cell
    (it starts off a multiple of S and crosses it: the odd slot), two
    multi-unit pieces in one tile; then 1, 2, 4, 5, S-1, S, S+1, 2S-1, 2S,
    2S+1, cap-1, cap+1, T-1, T, T+1, 2T+3."""
    runs = place_at([S])                       # ends on / starts on S
    pos = sum(runs)
    fill = (-(pos + 5)) % T                    # run of 11 straddles a tile
    runs += ([fill] if fill else []) + [11]
    # inside the second tile: two multi-unit pieces, the first starting off
    # a cell boundary (odd slot for its first unit)
    runs += [S - 9, 2 * S + 3, 2 * S]
    return runs + _uniq_pos(
        [1, 2, 4, 5, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 1, cap - 1,
         cap + 1, T - 1, T, T + 1, 2 * T + 3])


def spill_set(sorted_fids, cap):
    """Fids whose run has a multiple of cap strictly inside it: exactly the
    runs cut into more than one piece, which go to the slabs and the spill
    list; every other run is one whole piece and is updated in place.
    Sorted int64."""
    fid, a, b = run_bounds(sorted_fids)
    m = (a // cap + 1) * cap       # first multiple of cap after the head
    return torch.from_numpy(fid[m < b].astype(np.int64))


def record_case(K, runs, seed, s=3):
    """Recompute-reduce input for a run list: sorted_fids, records
    {row, bits of x} (x in {1, 2}, rows random), integer sumVX in {-8..8},
    dpred = +-2^-s, and the exact per-entry gradients they define for an
    integer V: gw = d x, gv = d (sumVX[row] - V[fid] x) x."""
    g = torch.Generator().manual_seed(seed)
    sorted_fids, F = runs_stream(runs, seed)
    n = sorted_fids.numel()
    B = 37
    rows = torch.randint(0, B, (n,), generator=g).to(torch.int32)
    x = torch.randint(1, 3, (n,), generator=g).float()
    rec = torch.stack([rows, x.view(torch.int32)], 1).contiguous()
    sumVX = torch.randint(-8, 9, (B, K), generator=g).float()
    sign = torch.randint(0, 2, (B,), generator=g).float() * 2 - 1
    dpred = sign * 2.0 ** -s
    return {"K": K, "F": F, "B": B, "sorted_fids": sorted_fids, "rec": rec,
            "rows": rows, "x": x, "sumVX": sumVX, "dpred": dpred, "s": s,
            "runs": runs}


def record_gradients(c, V):
    """float64 per-entry (gw, gv) of a record case under the V given"""
    d = c["dpred"].double()[c["rows"].long()]
    x = c["x"].double()
    sv = c["sumVX"].double()[c["rows"].long()]
    vx = V.double()[c["sorted_fids"].long()] * x.unsqueeze(1)
    return d * x, (d * x).unsqueeze(1) * (sv - vx)


def assert_exact_totals(fids, gw, gv, F, unit):
    """per fid and k, sum |term| / unit < 2^24, and every term a multiple of
    unit: any order of accumulation is exact"""
    aW, aV, _ = fid_totals(fids, gw.abs(), gv.abs(), F)
    assert _mx(aW) / unit < EXACT_LIMIT
    assert _mx(aV) / unit < EXACT_LIMIT
    for t in (gw, gv):
        q = t.double() / unit
        assert torch.equal(q, q.round())
