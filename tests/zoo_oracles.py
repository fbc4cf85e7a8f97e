"""Oracles, input builders, case lists, bounds and wrong references for the
codec, sparse-PS, AUC, GBM-histogram, conv, word2vec and compaction
kernels (the bindings production paths call that had one loose test).

Plain helper module in the pattern of ``kernel_oracles.py``, whose
tolerance rule (bit-exact / sum rule / short chain) and helpers it reuses.
Everything here runs on the CPU. ``test_zoo_oracles.py`` holds every oracle
to the project's own CPU path and shows that every wrong reference below
differs, or leaves the bound, on the inputs the GPU tests use;
``test_zoo_kernels_gpu.py`` runs the kernels against the oracles.

References are numpy / Python-int loops or float64. fp32 enters only where
the operation is *defined* in fp32: the codec midpoint
``0.5f * (t[j] + t[j+1])`` and the AUC bucket ``int(p * float(buckets-1))``.
Exactness conditions are asserted on the float64 side of every generated
case, so an inexact case fails instead of passing loosely.
"""

from __future__ import annotations

import math

import numpy as np
import torch

from kernel_oracles import (U23, U24, adagrad_ref, check_bits,  # noqa: F401
                            check_bound, differs, f32, poison)

F32 = np.float32
BF = torch.bfloat16


def _f32_next(v, up):
    return F32(np.nextafter(F32(v), F32(np.inf if up else -np.inf)))


# ---------------------------------------------------------------------------
# quantile codec: a pure selection
# ---------------------------------------------------------------------------
QUANT_SIZES = (1, 255, 256, 257, 513)  # a block is 256 values


def quantile_tables():
    """name -> fp32 table: uniform at every level count that changes the
    search depth, the three 256-level shapes, and an irregular one."""
    from lightctr_amd.utils.compress import QuantileCodec

    out = {}
    for levels in (1, 2, 3, 16, 255, 256):
        out[f"uniform{levels}"] = QuantileCodec(levels, "uniform").table
    for mode in ("log", "normal", "custom"):
        out[f"{mode}256"] = QuantileCodec(256, mode).table
    out["irregular"] = QuantileCodec.from_table(
        [-3.0, -1.0, -0.99999, 0.0, 1e-30, 0.5, 7.0, 1e20]).table
    return out


def quantile_midpoints(table):
    """the decision boundaries as the kernel forms them, in fp32"""
    t = table.numpy().astype(F32)
    return F32(0.5) * (t[:-1] + t[1:])


def quantile_inputs(table):
    """every entry; every midpoint and its two fp32 neighbours; values
    outside the table; +-inf, NaN, +-0"""
    t = table.numpy().astype(F32)
    m = quantile_midpoints(table)
    parts = [t, m, np.nextafter(m, F32(np.inf)), np.nextafter(m, F32(-np.inf)),
             np.array([t[0] - F32(1), t[0] * F32(4) - F32(1), t[-1] + F32(1),
                       t[-1] * F32(4) + F32(1), np.inf, -np.inf, np.nan,
                       0.0, -0.0], dtype=F32)]
    return torch.from_numpy(np.concatenate(parts).astype(F32))


def quantile_sized(table, n):
    """n values cycling through quantile_inputs, rotated so that the last
    block's tail does not always hold the same ones"""
    x = quantile_inputs(table)
    idx = (torch.arange(n) * 7 + n) % x.numel()
    return x[idx].clone()


def quantile_encode_ref(x, table, mutant=None):
    """code = number of fp32 midpoints strictly below x, by linear scan.
    A NaN is below no midpoint and not above one either; the search sends
    whatever fails ``x <= mid`` upwards, so NaN lands on levels-1, as the
    CPU path's searchsorted does. mutant 'lt' tests ``x < mid``."""
    xs = x.numpy().astype(F32)
    mids = quantile_midpoints(table)
    code = np.zeros(xs.shape, dtype=np.int64)
    for m in mids:
        below = (xs < m) if mutant == "lt" else (xs <= m)
        code += ~below
    return torch.from_numpy(code.astype(np.uint8))


def quantile_decode_ref(code, table):
    assert int(code.max()) < table.numel()  # the contract of decode
    return table[code.long()]


# ---------------------------------------------------------------------------
# low-bit codec
# ---------------------------------------------------------------------------
# 32 / bits values per word, 256 words per block
LOWBIT_SIZES = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097,
                8191, 8192, 8193)
LOWBIT_THRESH = 0.75


def lowbit_inputs(n, seed, thresh=LOWBIT_THRESH):
    """randn with +-0, NaN, +-inf, +-thresh and thresh's fp32 neighbours
    on both sides at the head and at the tail (the last word)"""
    th = F32(thresh)
    sp = [0.0, -0.0, np.nan, np.inf, -np.inf, th, -th,
          _f32_next(th, True), _f32_next(th, False),
          -_f32_next(th, True), -_f32_next(th, False)]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g).numpy().astype(F32)
    for i in range(n):
        if i < len(sp) or i >= n - len(sp):
            x[i] = sp[(i + seed) % len(sp)]
    return torch.from_numpy(x)


def lowbit_pack_ref(x, thresh, bits, mutant=None):
    """Python-int packing: value j sits at bit (j % per) * bits of word
    j // per; bit 0 of a code is ``v >= 0`` (+-0 both set it, NaN does
    not), bit 1 is ``|v| >= thresh``; padding bits are zero.
    mutants: 'droplast' leaves out the last partial word, 'padset' sets
    the padding bits."""
    th = F32(thresh)
    per = 32 // bits
    xs = x.numpy().astype(F32)
    n = xs.size
    nw = (n * bits + 31) // 32
    words = [0] * nw
    for j in range(n):
        v = xs[j]
        c = 1 if v >= 0 else 0
        if bits == 2 and abs(v) >= th:
            c |= 2
        words[j // per] |= c << ((j % per) * bits)
    used = n * bits - (nw - 1) * 32  # bits of the last word that hold data
    if used < 32 and nw:
        if mutant == "droplast":
            words[-1] = 0
        if mutant == "padset":
            words[-1] |= (0xFFFFFFFF >> used) << used
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.int32))


def lowbit_decode_ref(words, lo, hi, bits, n):
    """x[j] = (+1 or -1) * (hi if bit 1 else lo) as one fp32 product, so a
    negative sign over lo = 0 gives -0.0"""
    w = words.numpy().view(np.uint32)
    per = 32 // bits
    out = np.empty(n, dtype=F32)
    for j in range(n):
        c = (int(w[j // per]) >> ((j % per) * bits)) & ((1 << bits) - 1)
        sign = F32(1) if c & 1 else F32(-1)
        mag = F32(hi) if (bits == 2 and c & 2) else F32(lo)
        out[j] = sign * mag
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------
# ps_apply: the sparse PS shard's fused updaters
# ---------------------------------------------------------------------------
PS_F = 23
# lanes stride k = 0..K by 64: the W element k == K is lane K % 64 of trip
# K / 64
PS_KS = (1, 2, 8, 62, 63, 64, 65, 127, 128, 129)
PS_NS = (1, 3, 4, 5, 9)  # a block holds 4 keys
PS_UPDATERS = ("sgd", "adagrad", "dcasgd", "dcasgda")
PS_HYPER = dict(lr=0.05, lam=0.1, eps=1e-8)
PS_STATE = ("W", "V", "nW", "nV", "shW", "shV")
# what each updater may write (in the rows of the key list, and for the
# shadows in worker wi's copy only)
PS_OWNS = {"sgd": ("W", "V"), "adagrad": ("W", "V", "nW", "nV"),
           "dcasgd": ("W", "V", "shW", "shV"),
           "dcasgda": ("W", "V", "nW", "nV", "shW", "shV")}


def ps_keys(n, seed):
    """n distinct rows in a shuffled order that always hold row 0 and row
    F-1 (n = 1: one of the two, by seed)"""
    g = torch.Generator().manual_seed(seed)
    if n == 1:
        return torch.tensor([0 if seed % 2 else PS_F - 1])
    mid = (torch.randperm(PS_F - 2, generator=g)[:n - 2] + 1).tolist()
    keys = torch.tensor([0, PS_F - 1] + mid)
    return keys[torch.randperm(n, generator=g)]


def ps_inputs(K, n, seed, exact=False):
    """Float set: the magnitudes of test_ps_dense_gpu._state (params
    ~N(0,1), grads ~1e-2, accumulators in [0, 0.1], shadows ~0.1).
    Exact set: integers, for sgd at lr = 0.5."""
    g = torch.Generator().manual_seed(seed)
    F = PS_F
    if exact:
        ri = lambda *s: torch.randint(-8, 9, s, generator=g).float()
        st = {"W": ri(F), "V": ri(F, K), "nW": ri(F).abs(),
              "nV": ri(F, K).abs(), "shW": ri(2, F), "shV": ri(2, F, K),
              "gW": ri(n), "gV": ri(n, K)}
    else:
        rn = lambda *s: torch.randn(*s, generator=g)
        st = {"W": rn(F), "V": rn(F, K) * 0.1,
              "nW": torch.rand(F, generator=g) * 0.1,
              "nV": torch.rand(F, K, generator=g) * 0.1,
              "shW": rn(2, F) * 0.1, "shV": rn(2, F, K) * 0.1,
              "gW": rn(n) * 0.01, "gV": rn(n, K) * 0.01}
    st["lidx"] = ps_keys(n, seed)
    return st


def _ps_elem(p, acc, sh, g, updater, lr, lam, eps):
    """one element's update in float64 with its short-chain bound;
    returns {name: (ref, bound)} for p and whichever of acc / sh the
    updater owns.

      sgd      p' = p - lr g              u|lr g| + one ulp of p'
      adagrad  kernel_oracles.adagrad_ref with l2 = 0
      dcasgda  a' = c95 a + c05 g g       4 roundings on positive terms,
                                          each at most u a'
               l  = lam rsqrt(a' + eps)   half the radicand's relative
                                          error (a's, +u for the add), one
                                          ulp (2u) for __frsqrt_rn, +u for
                                          the product
      dcasgd   l  = lam                   exact
      d  = p - sh                         u|d|
      t  = ((l g) g) d                    |t| (rel(l) + 3u + u)
      s  = g + t                          err(t) + u(|g| + |t|)
      up = lr s                           lr err(s) + u|up|
      p' = p - up                         err(up) + one ulp of p'
      sh' = p'                            the same bits
    c95 / c05 are the fp32 values of 0.95f / 0.05f."""
    out = {}
    if updater == "sgd":
        p1 = p - lr * g
        out["p"] = (p1, U24 * (lr * g).abs() + U23 * p1.abs())
        return out
    if updater == "adagrad":
        r = adagrad_ref(p, g, acc, lr, eps, 0.0)
        out["p"], out["acc"] = r["W"], r["n"]
        return out
    rel_l = torch.zeros_like(p)
    lam_e = torch.full_like(p, lam)
    if updater == "dcasgda":
        c95, c05 = f32(0.95), f32(0.05)
        a1 = c95 * acc + c05 * g * g
        ea = 4 * U24 * a1
        rad = a1 + eps
        rel_l = 0.5 * (ea / rad + U24) + 3 * U24
        lam_e = lam / torch.sqrt(rad)
        out["acc"] = (a1, ea)
    d = p - sh
    t = lam_e * g * g * d
    et = t.abs() * (rel_l + 4 * U24)
    s = g + t
    es = et + U24 * (g.abs() + t.abs())
    up = lr * s
    p1 = p - up
    ep = lr * es + U24 * up.abs() + U23 * p1.abs()
    out["p"] = (p1, ep)
    out["sh"] = (p1, ep)
    return out


def ps_apply_ref(st, updater, wi, lr, lam, eps, mutant=None):
    """float64 tables after one ps_apply on the rows of st['lidx'] (distinct
    keys: duplicates are outside the contract), {name: (ref64, bound)}
    for all six state arrays; the bound is zero wherever the updater must
    not write.
    mutants: 'w_small_k' updates W only when K < 64; 'noshadow' leaves the
    shadow rows as they were."""
    lr, lam, eps = f32(lr), f32(lam), f32(eps)
    K = st["V"].shape[1]
    ref = {k: st[k].double().clone() for k in PS_STATE}
    bnd = {k: torch.zeros_like(ref[k]) for k in PS_STATE}
    rows = st["lidx"].long()
    assert rows.unique().numel() == rows.numel()
    for tab, acc, sh, grad in (("W", "nW", "shW", "gW"),
                               ("V", "nV", "shV", "gV")):
        if tab == "W" and mutant == "w_small_k" and K >= 64:
            continue
        r = _ps_elem(ref[tab][rows], ref[acc][rows], ref[sh][wi][rows],
                     st[grad].double(), updater, lr, lam, eps)
        ref[tab][rows], bnd[tab][rows] = r["p"]
        if "acc" in r:
            ref[acc][rows], bnd[acc][rows] = r["acc"]
        if "sh" in r and mutant != "noshadow":
            ref[sh][wi][rows], bnd[sh][wi][rows] = r["sh"]
    return {k: (ref[k], bnd[k]) for k in PS_STATE}


def ps_untouched(F, lidx):
    keep = torch.ones(F, dtype=torch.bool)
    keep[lidx.long()] = False
    return keep


# ---------------------------------------------------------------------------
# histogram AUC
# ---------------------------------------------------------------------------
AUC_ADD_BUCKETS = (1, 2, 3, 1000, 1024, 1 << 20)
# the grid is capped at 4096 blocks x 256 threads: 1 048 577 puts one
# element on the second grid-stride trip
AUC_ADD_NS = (1, 255, 256, 257, 1 << 20, (1 << 20) + 1)
AUC_SCAN_BUCKETS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049,
                    3079)  # the scan walks chunks of 1024 buckets


def auc_preds(buckets, n, seed):
    """(pred, label): bucket edges j / (buckets-1) with both fp32
    neighbours for a spread of j, 0, -0.0, 1, 1 - 2^-24, a subnormal,
    values outside [0, 1] and +-inf at the head and at the tail, uniform
    draws in between. No NaN (outside the contract)."""
    sp = [0.0, -0.0, 1.0, 1.0 - 2.0 ** -24, 1e-40, -0.5, 1.5, np.inf,
          -np.inf]
    if buckets > 1:
        B1 = buckets - 1
        for j in sorted({0, 1, 2, B1 // 3, B1 // 2, B1 - 2, B1 - 1, B1}):
            if 0 <= j <= B1:
                v = F32(j / B1)
                sp += [v, _f32_next(v, True), _f32_next(v, False)]
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(n, generator=g).numpy().astype(F32)
    for i in range(min(n, len(sp))):
        p[i] = sp[(i + seed) % len(sp)]
    for i in range(min(n, len(sp))):
        p[n - 1 - i] = sp[(i + 3 * seed + 1) % len(sp)]
    label = torch.randint(0, 2, (n,), generator=g).float()
    return torch.from_numpy(p), label


def auc_hist_ref(pred, label, buckets, mutant=None):
    """[2 * buckets] counts, negatives first. The bucket is *defined* in
    fp32: clamp to [0, 1], one fp32 product with float(buckets-1),
    truncation. mutant 'round' rounds to nearest instead."""
    p = np.clip(pred.numpy().astype(F32), F32(0), F32(1))
    assert not np.isnan(p).any()
    prod = p * F32(buckets - 1)
    assert prod.dtype == F32
    b = np.rint(prod) if mutant == "round" else np.floor(prod)
    b = np.clip(b.astype(np.int64), 0, buckets - 1)
    pos = label.numpy() > 0.5
    neg_h = np.bincount(b[~pos], minlength=buckets)
    pos_h = np.bincount(b[pos], minlength=buckets)
    return torch.from_numpy(np.concatenate([neg_h, pos_h]).astype(np.int64))


def _as_i32(counts):
    """Python-int counts below 2^32 stored as their int32 bit patterns"""
    return torch.from_numpy(
        np.array(counts, dtype=np.uint64).astype(np.uint32).view(np.int32))


def auc_scan_hists(buckets):
    """(name, neg counts, pos counts) as Python-int lists"""
    Z = lambda: [0] * buckets
    out = []
    neg, pos = Z(), Z()
    neg[0], pos[0] = 7, 5
    out.append(("first", neg, pos))
    neg, pos = Z(), Z()
    neg[-1], pos[-1] = 7, 5
    out.append(("last", neg, pos))
    rng = np.random.RandomState(buckets)
    out.append(("random", rng.randint(0, 6, buckets).tolist(),
                rng.randint(0, 6, buckets).tolist()))
    if buckets >= 2:
        neg, pos = Z(), Z()
        neg[0], pos[-1] = 11, 13
        out.append(("ends", neg, pos))
        neg, pos = Z(), Z()
        neg[-1], pos[0] = 11, 13
        out.append(("ends_mirror", neg, pos))
        # one count above 2^31 and totals above 2^32; the negatives stay
        # few so that 2 * correct stays below 2^53
        neg, pos = Z(), Z()
        pos[buckets // 2] = 3_000_000_000
        pos[0] += 2_000_000_000
        for j in rng.randint(0, buckets, 8):
            neg[j] += int(rng.randint(1, 4))
        out.append(("big", neg, pos))
    if buckets > 1024:
        # the running_s carry between the first two chunks
        neg, pos = Z(), Z()
        neg[1023], pos[1024] = 3, 9
        out.append(("carry", neg, pos))
        neg, pos = Z(), Z()
        neg[1024], pos[1023] = 3, 9
        out.append(("carry_mirror", neg, pos))
    return out


def auc_hist_tensor(neg, pos):
    return _as_i32(list(neg) + list(pos))


def auc_scan_ref(neg, pos, mutant=None):
    """(correct, P, N) as exact values from Python ints:
    2 * correct = sum_b neg_b (2 (P - cum_b) + pos_b), cum inclusive.
    mutants: 'nocarry' restarts cum at every 1024-bucket chunk, 'signed'
    reads the counts as int32, 'exclusive' uses the exclusive cum,
    'notie' omits the half-tie term."""
    if mutant == "signed":
        sg = lambda c: c - (1 << 32) if c >= (1 << 31) else c
        neg, pos = [sg(c) for c in neg], [sg(c) for c in pos]
    P, N = sum(pos), sum(neg)
    two, cum = 0, 0
    for b in range(len(neg)):
        if mutant == "nocarry" and b % 1024 == 0:
            cum = 0
        above = P - cum if mutant == "exclusive" else P - cum - pos[b]
        cum += pos[b]
        tie = 0 if mutant == "notie" else pos[b]
        two += neg[b] * (2 * above + tie)
    if mutant is None:
        # every partial sum of non-negative halves is exact in fp64
        assert 0 <= two < 2 ** 53 and P < 2 ** 53 and N < 2 ** 53
    return two / 2, float(P), float(N)


# ---------------------------------------------------------------------------
# gbm_hist
# ---------------------------------------------------------------------------
GBM_FB = 4  # features per block


def gbm_zsplit(D, n_nodes):
    """the launcher's row split: each z slice of the grid walks rows
    z * 256 + thread, stepping by zsplit * 256"""
    fb = (D + GBM_FB - 1) // GBM_FB
    return max(1, 2048 // max(1, fb * n_nodes))


def gbm_cases():
    """(N, D, n_nodes, placement): one axis at a time around
    (1000, 5, 3), then the placements."""
    base = (1000, 5, 3)
    cs = [base + ("random",)]
    cs += [(1000, D, 3, "random") for D in (1, 3, 4, 7, 8, 39)]
    cs += [(1000, 5, nn, "random") for nn in (1, 2, 64, 2048, 2049)]
    cs += [(N, 5, 3, "random") for N in (1, 255, 256, 257)]
    # the row loop's second trip, at each case's own zsplit
    cs += [(gbm_zsplit(5, 3) * 256 + 1, 5, 3, "random"),
           (gbm_zsplit(4, 2048) * 256 + 1, 4, 2048, "random")]
    assert gbm_zsplit(4, 2048) == 1
    cs += [base + (p,) for p in ("none", "onebin", "edgebins", "emptynode")]
    return cs


def gbm_inputs(N, D, n_nodes, placement, seed, exact):
    """bins u8 [N, D], grad, hess, node i32 in [-1, n_nodes). Exact set:
    grad integers in -3..3, hess multiples of 0.25 in [0, 3]."""
    g = torch.Generator().manual_seed(seed)
    bins = torch.randint(0, 256, (N, D), generator=g).to(torch.uint8)
    node = torch.randint(-1, n_nodes, (N,), generator=g).to(torch.int32)
    if exact:
        grad = torch.randint(-3, 4, (N,), generator=g).float()
        hess = torch.randint(0, 13, (N,), generator=g).float() * 0.25
    else:
        grad = torch.randn(N, generator=g)
        hess = torch.rand(N, generator=g) * 0.25 + 1e-3
    if placement == "none":
        node.fill_(-1)
    elif placement == "onebin":
        node.fill_(n_nodes - 1)
        bins.fill_(17)
    elif placement == "edgebins":
        bins = (bins & 1) * 255
    elif placement == "emptynode":
        assert n_nodes >= 2
        node[node == 1] = 0
    return bins, grad, hess, node


def gbm_hist_ref(bins, grad, hess, node, n_nodes, exact, mutant=None):
    """(hist64 [n_nodes, D, 256, 2], bound): np.add.at in float64. The sum
    rule gives n 2^-23 sum|term| per bin, n the bin's row count (the LDS
    and global atomics are one summation tree over those n terms). In the
    exact set every bin's sum of |term| is asserted below 2^24 units of
    0.25, so any order is exact and the bound is zero.
    mutants: 'dropfeat' leaves out the last D % 4 features, 'droptrip'
    the rows past the first trip of the row loop."""
    N, D = bins.shape
    assert int(node.max()) < n_nodes  # ids >= n_nodes are not fed
    hist = np.zeros((n_nodes, D, 256, 2))
    mag = np.zeros((n_nodes, D, 256, 2))
    cnt = np.zeros((n_nodes, D, 256, 1))
    act = (node >= 0).numpy()
    if mutant == "droptrip":
        act = act & (np.arange(N) < gbm_zsplit(D, n_nodes) * 256)
    rows = np.nonzero(act)[0]
    nd = node.numpy().astype(np.int64)[rows]
    b = bins.numpy().astype(np.int64)[rows]
    gh = np.stack([grad.numpy(), hess.numpy()], 1).astype(np.float64)[rows]
    nfeat = D - D % GBM_FB if mutant == "dropfeat" else D
    for f in range(nfeat):
        np.add.at(hist, (nd, f, b[:, f]), gh)
        np.add.at(mag, (nd, f, b[:, f]), np.abs(gh))
        np.add.at(cnt, (nd, f, b[:, f]), 1.0)
    hist, mag, cnt = (torch.from_numpy(a) for a in (hist, mag, cnt))
    if exact:
        assert float(mag.max()) * 4 < 2 ** 24
        return hist + 0.0, torch.zeros_like(hist)  # -0 folded to +0
    return hist, cnt * U23 * mag


# ---------------------------------------------------------------------------
# im2col_bf16 / col2im
# ---------------------------------------------------------------------------
# (B, C, H, W, k, s, p) around (2, 3, 7, 5, 3, 1, 1), H != W throughout
CONV_BASE = (2, 3, 7, 5, 3, 1, 1)


def conv_cases():
    B, C, H, W, k, s, p = CONV_BASE
    cs = [CONV_BASE]
    cs += [(B, C, H, W, kk, s, p) for kk in (1, 2, 5)]
    cs += [(B, C, H, W, k, ss, p) for ss in (2, 3, 4)]  # 4 > k: bare pixels
    cs += [(B, C, H, W, k, s, pp) for pp in (0, 2, 3, 4)]  # pad >= k too
    cs += [(B, C, H, W, 2, 3, 0), (B, C, H, W, 1, 4, 0)]  # s > k, no pad
    cs += [(B, C, 5, 7, 7, 1, 1),   # k = H + 2p: OH = 1
           (B, C, 7, 5, 7, 1, 1)]   # k = W + 2p: OW = 1
    cs += [(B, C, H, W, k, 4, 2)]   # (H + 2p - k) % s = 0 but W's is not
    cs += [(B, 1, H, W, k, s, p), (B, 8, H, W, k, s, p),
           (1, C, H, W, k, s, p), (5, C, H, W, k, s, p)]
    assert any((c[2] + 2 * c[6] - c[4]) % c[5] for c in cs)
    assert all(c[2] != c[3] for c in cs)
    return cs


# 2 211 840 col elements: more than the 8192 x 256 threads of the capped
# grid, so the grid-stride loop takes a second trip
CONV_BIG = (5, 16, 64, 48, 3, 1, 1)
# col2im's loop is over B C H W pixels: k = 1 keeps dcol the same size
COL2IM_BIG = (2, 16, 257, 256, 1, 1, 0)
assert 2 * 16 * 257 * 256 > 8192 * 256


def conv_out(H, W, k, s, p):
    return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def conv_x(B, C, H, W, seed, integer=False):
    """fp32 image. Float form: randn with exact bf16 rounding ties of both
    parities (1 + 2^-8 rounds down to even, 1 + 3 * 2^-8 up to even), -0.0
    and +-inf scattered in. Integer form: values in -3..3 (bf16-exact)."""
    g = torch.Generator().manual_seed(seed)
    if integer:
        return torch.randint(-3, 4, (B, C, H, W), generator=g).float()
    x = torch.randn(B, C, H, W, generator=g)
    sp = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8),
                       -(1 + 3 * 2.0 ** -8), -0.0, float("inf"),
                       -float("inf"), 0.0])
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:min(flat.numel(), 24)]
    flat[idx] = sp[torch.arange(idx.numel()) % sp.numel()]
    return x


def _taps(H, W, k, s, p):
    """(kh, kw, oh, h, ow range, w range) of every in-image tap, one
    output row at a time"""
    OH, OW = conv_out(H, W, k, s, p)
    for kh in range(k):
        for kw in range(k):
            ows = [ow for ow in range(OW) if 0 <= ow * s - p + kw < W]
            if not ows:
                continue
            o0, o1 = ows[0], ows[-1] + 1
            w0 = o0 * s - p + kw
            w1 = (o1 - 1) * s - p + kw + 1
            for oh in range(OH):
                h = oh * s - p + kh
                if 0 <= h < H:
                    yield kh, kw, oh, h, slice(o0, o1), slice(w0, w1, s)


def im2col_ref(x, k, s, p, mutant=None):
    """col[(b, oh, ow), (c, kh, kw)] = bf16(x[b, c, oh s - p + kh,
    ow s - p + kw]), +0 where the tap is in the padding: a selection and
    one round-to-nearest-even convert, bit-exact.
    mutants: 'hw_swap' reads the pixel at flat offset w * H + h,
    'k_swap' exchanges kh and kw in the column index, 'nopad' leaves the
    padding slots unwritten (NaN stands for what the allocator held)."""
    B, C, H, W = x.shape
    OH, OW = conv_out(H, W, k, s, p)
    xb = x.to(BF)
    if mutant == "hw_swap":
        xb = xb.reshape(B, C, W, H).transpose(2, 3)
    fill = float("nan") if mutant == "nopad" else 0.0
    col = torch.full((B, OH, OW, C, k, k), fill, dtype=BF)
    for kh, kw, oh, h, ows, ws in _taps(H, W, k, s, p):
        a, b = (kw, kh) if mutant == "k_swap" else (kh, kw)
        col[:, oh, ows, :, a, b] = xb[:, :, h, ws].permute(0, 2, 1)
    return col.view(B * OH * OW, C * k * k)


def col2im_ref(dcol, B, C, H, W, k, s, p, exact):
    """(dx64, bound): scatter-add of every in-image tap in float64. A
    pixel sums at most k^2 terms: the sum rule with n = its tap count;
    in the exact set (integers in -3..3) the sums are exact, the bound is
    zero and a pixel no patch covers is +0."""
    OH, OW = conv_out(H, W, k, s, p)
    d = dcol.double().view(B, OH, OW, C, k, k)
    dx = torch.zeros(B, C, H, W, dtype=torch.float64)
    mag = torch.zeros_like(dx)
    cnt = torch.zeros_like(dx)
    for kh, kw, oh, h, ows, ws in _taps(H, W, k, s, p):
        t = d[:, oh, ows, :, kh, kw].permute(0, 2, 1)
        dx[:, :, h, ws] += t
        mag[:, :, h, ws] += t.abs()
        cnt[:, :, h, ws] += 1
    if exact:
        assert float(mag.max()) < 2 ** 24
        return dx + 0.0, torch.zeros_like(dx)
    return dx, cnt * U23 * mag


def conv_uncovered(B, C, H, W, k, s, p):
    """[B, C, H, W] mask of the pixels no patch covers (s > k, or a last
    row / column the stride steps over)"""
    seen = torch.zeros(B, C, H, W, dtype=torch.bool)
    for _, _, _, h, _, ws in _taps(H, W, k, s, p):
        seen[:, :, h, ws] = True
    return ~seen


def col2im_gather_ref(dcol, B, C, H, W, k, s, p, mutant=None):
    """The gather form, pixel by pixel (small shapes only).
    mutants: 'nomod' drops the stride-modulo skip, 'noguard' the
    ``oh >= OH`` / ``ow >= OW`` guards (a read past the buffer counts as
    NaN), 'k_swap' exchanges kh and kw, 'hw_swap' writes the pixel at
    flat offset w * H + h."""
    OH, OW = conv_out(H, W, k, s, p)
    flat = dcol.double().reshape(-1)
    kk = k * k
    dx = torch.zeros(B * C * H * W, dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            for h in range(H):
                for w in range(W):
                    acc = 0.0
                    for kh in range(k):
                        on = h + p - kh
                        if on < 0 or (on % s and mutant != "nomod"):
                            continue
                        oh = on // s
                        if oh >= OH and mutant != "noguard":
                            continue
                        for kw in range(k):
                            wn = w + p - kw
                            if wn < 0 or (wn % s and mutant != "nomod"):
                                continue
                            ow = wn // s
                            if ow >= OW and mutant != "noguard":
                                continue
                            a, bb = (kw, kh) if mutant == "k_swap" \
                                else (kh, kw)
                            i = ((b * OH * OW + oh * OW + ow) * (C * kk)
                                 + (c * k + a) * k + bb)
                            acc += float(flat[i]) if i < flat.numel() \
                                else float("nan")
                    pix = w * H + h if mutant == "hw_swap" else h * W + w
                    dx[(b * C + c) * H * W + pix] = acc
    return dx.view(B, C, H, W)


def conv_dcol(B, C, H, W, k, s, p, seed, exact):
    OH, OW = conv_out(H, W, k, s, p)
    g = torch.Generator().manual_seed(seed)
    shape = (B * OH * OW, C * k * k)
    if exact:
        return torch.randint(-3, 4, shape, generator=g).float()
    return torch.randn(shape, generator=g)


# ---------------------------------------------------------------------------
# w2v_negsample_step
# ---------------------------------------------------------------------------
W2V_DS = (1, 2, 16, 63, 64)   # lane == dimension, masked at D < 64
W2V_CS = (1, 4)
W2V_NS = (0, 1, 3, 5)
W2V_BS = (1, 3, 4, 5, 9)      # a block holds 4 examples
W2V_LR, W2V_SCALE = 0.1, 0.5

# Accuracy of the part nobody can derive: p = 1 / (1 + __expf(-dot)) and
# the __logf behind the loss. Measured on the MI355X through loss[ex] of
# N = 0 examples with exactly representable dots sweeping [-17, 17] (there
# loss = -log p, so the relative deviation of p is the absolute deviation
# of the loss): the largest |loss - loss64| of w2v_sweep_inputs() was
# 1.49006e-06 = 2^-19.36, at dot -13.5 (where one ulp of the fp32 loss
# itself is 9.5e-07, so the figure is not far above what any fp32 loss
# could show).
W2V_INTRINSIC_MEASURED = 1.4901e-06
# one run samples few arguments of an intrinsic whose error varies with
# the argument: allow 4x
W2V_INTRINSIC_REL = 4 * W2V_INTRINSIC_MEASURED


def w2v_sweep_inputs():
    """137 examples, D = C = 1, N = 0: E[i] = -17 + i / 4, O[i] = 1, so
    every dot is exact in fp32"""
    n = 137
    E = (torch.arange(n).float() * 0.25 - 17.0).view(n, 1)
    O = torch.ones(n, 1)
    idx = torch.arange(n)
    return {"E": E, "O": O, "centers": idx.clone(), "ctx": idx.view(n, 1),
            "negs": torch.zeros(n, 0, dtype=torch.long)}


def w2v_inputs(D, C, N, B, seed):
    """Pairwise disjoint word sets per example (the Hogwild updates cannot
    meet). Inside an example: a context word twice (C >= 2), a negative
    equal to the centre (N >= 1, odd examples), one negative twice
    (N >= 3). Example 0's centre row is set against x so that its dot is
    about -20, past the clamp. Word ids are spread over a table with
    unused rows in between."""
    g = torch.Generator().manual_seed(seed)
    per = C + 1 + N
    V = 2 * per * B + 3
    E = torch.rand(V, D, generator=g) - 0.5
    O = (torch.rand(V, D, generator=g) - 0.5) * 0.2
    ids = torch.randperm(V, generator=g)[:per * B].view(B, per)
    ctx = ids[:, :C].clone()
    centers = ids[:, C].clone()
    negs = ids[:, C + 1:].clone()
    if C >= 2:
        ctx[:, C - 1] = ctx[:, 0]
    if N >= 1:
        negs[1::2, 0] = centers[1::2]
    if N >= 3:
        negs[:, 2] = negs[:, 1]
    x = E[ctx[0]].double().mean(0)
    O[centers[0]] = (-20.0 / float((x * x).sum()) * x).float()
    return {"E": E, "O": O, "centers": centers, "ctx": ctx, "negs": negs}


def w2v_ref(inp, lr, scale, mutant=None):
    """The sequential float64 definition, example by example:

      x = (sum_c E[ctx_c]) / C
      for t in [centre] + negatives:          y = 1 for the centre
          o = O[t]                            read before its own update
          p = sigmoid(clamp(x . o, -16, 16))
          loss += -(y log p + (1 - y) log(1 - p))
          g = (p - y) scale;  gx += g o;  O[t] -= lr g x
      E[ctx_c] -= lr gx / C  for every context slot, last

    and the first-order bound of the fp32 chain, carried per element
    through the sequence (eE, eO start at zero):

      x       C 2^-23 sum|E| / C (sum rule) + u|x|
      dot     sum(|o| ex + |x| eo) + D 2^-23 sum|x o|; the clamp is a
              contraction
      p       sigmoid' err(dot) + REL p, REL = W2V_INTRINSIC_REL and
              sigmoid' <= min(1/4, p (1 - p) e^err)
      loss    y = 1: err(p)/p;  y = 0: q = 1 - p carries err(p) + u q and
              the term err(q) / (q - err(q)) + REL for the logarithm;
              (N + 1) 2^-23 sum|term| for the running sum. Asserted:
              p - err(p) and q - 4 err(q) stay above the 1e-7 floor, so
              the floor is inactive and first order holds.
      g       scale (err(p) + u|p - y|) + u|g|
      gx      sum(|o| eg + |g| eo) + (N + 1) 2^-23 sum|g o|
      O[t]    lr (|x| eg + |g| ex) + 2u|lr g x| + one ulp of the new O
      E[w]    lr/C err(gx) + 2u|lr gx / C| + one ulp of the new E, per
              context slot

    Returns {E, O, loss: (ref64, bound)}.
    mutants: 'no_inv_c' omits 1/C in the mean, 'neg_y1' labels negatives
    1, 'gx_updated' forms gx from the updated O row, 'noclamp',
    'drop_ctx' leaves the last context word out of the sum, 'drop_dim'
    leaves dimension D-1 out of the dot."""
    lr, scale = f32(lr), f32(scale)
    REL = W2V_INTRINSIC_REL
    E, O = inp["E"].double().clone(), inp["O"].double().clone()
    eE, eO = torch.zeros_like(E), torch.zeros_like(O)
    B, C = inp["ctx"].shape
    N = inp["negs"].shape[1]
    D = E.shape[1]
    inv_c = f32(1.0 / C)
    loss = torch.zeros(B, dtype=torch.float64)
    eloss = torch.zeros(B, dtype=torch.float64)
    for ex in range(B):
        ws = inp["ctx"][ex].tolist()
        rows = E[ws]
        if mutant == "drop_ctx":
            rows = rows[:-1]
        xs, xa = rows.sum(0), rows.abs().sum(0)
        mean_c = 1.0 if mutant == "no_inv_c" else inv_c
        x = xs * mean_c
        ex_ = C * U23 * xa * inv_c + U24 * x.abs()
        gx, egx, gxa = (torch.zeros(D, dtype=torch.float64)
                        for _ in range(3))
        la = 0.0
        tgts = [int(inp["centers"][ex])] + inp["negs"][ex].tolist()
        for ti, t in enumerate(tgts):
            y = 1.0 if (ti == 0 or mutant == "neg_y1") else 0.0
            o, eo = O[t].clone(), eO[t].clone()
            prod = x * o
            if mutant == "drop_dim":
                prod = prod[:-1]
            dot = float(prod.sum())
            edot = float((o.abs() * ex_ + x.abs() * eo).sum()
                         + D * U23 * prod.abs().sum())
            dc = dot if mutant == "noclamp" else min(16.0, max(-16.0, dot))
            p = 1.0 / (1.0 + math.exp(-dc))
            q = 1.0 / (1.0 + math.exp(dc))
            ep = min(0.25, p * q * math.exp(edot)) * edot + REL * p
            if y == 1.0:
                term, eterm = -math.log(p), ep / p
                if mutant is None:
                    assert p - ep > 1e-7, (p, ep)
            else:
                eq = ep + U24 * q
                if mutant is None:
                    assert q - 4 * eq > 1e-7, (q, eq)
                term, eterm = -math.log(q), eq / max(q - eq, 1e-300) + REL
            loss[ex] += term
            la += abs(term)
            eloss[ex] += eterm
            gz = (p - y) * scale
            eg = scale * (ep + U24 * abs(p - y)) + U24 * abs(gz)
            onew = o - lr * gz * x
            eonew = eo + lr * (x.abs() * eg + abs(gz) * ex_) \
                + 2 * U24 * (lr * gz * x).abs() + U23 * onew.abs()
            O[t], eO[t] = onew, eonew
            osrc = onew if mutant == "gx_updated" else o
            gx += gz * osrc
            gxa += (gz * osrc).abs()
            egx += o.abs() * eg + abs(gz) * eo
        eloss[ex] += (N + 1) * U23 * la
        egx += (N + 1) * U23 * gxa
        ge = lr * gx * inv_c
        ege = lr * inv_c * egx + 2 * U24 * ge.abs()
        for w in ws:
            E[w] = E[w] - ge
            eE[w] = eE[w] + ege + U23 * E[w].abs()
    return {"E": (E, eE), "O": (O, eO), "loss": (loss, eloss)}


def w2v_used(inp):
    """(rows of E, rows of O) an example may write"""
    return (inp["ctx"].reshape(-1).unique(),
            torch.cat([inp["centers"], inp["negs"].reshape(-1)]).unique())


# ---------------------------------------------------------------------------
# bitmap_compact / inv_perm_i32
# ---------------------------------------------------------------------------
BITMAP_NWORDS = (1, 63, 64, 65, 1023, 1024, 1025, 2049)  # 1024 words/block
BITMAP_PATTERNS = ("empty", "bit0", "bit63_last", "full_block", "p01",
                   "p50")
INV_PERM_NS = (1, 255, 256, 257, 4097)


def bitmap_fids(nwords, pattern, seed):
    """the fids that set the bits, duplicates included (int64)"""
    F = nwords * 64
    g = torch.Generator().manual_seed(seed)
    if pattern == "empty":
        return torch.zeros(0, dtype=torch.long)
    if pattern == "bit0":
        return torch.tensor([0, 0])
    if pattern == "bit63_last":
        return torch.tensor([F - 1])
    if pattern == "full_block":
        # every bit of the last whole 1024-word block (or of the whole
        # bitmap when it is shorter), plus one repeat
        w0 = (nwords // 1024 - 1) * 1024 if nwords >= 1024 else 0
        w1 = w0 + 1024 if nwords >= 1024 else nwords
        r = torch.arange(w0 * 64, w1 * 64)
        return torch.cat([r, r[:1]])
    frac = 0.01 if pattern == "p01" else 0.5
    m = max(1, int(F * frac))
    return torch.randint(0, F, (2 * m,), generator=g)


def bitmap_words(nwords, fids):
    """int64 words with bit f % 64 of word f // 64 set"""
    w = np.zeros(nwords, dtype=np.uint64)
    f = fids.numpy().astype(np.uint64)
    np.bitwise_or.at(w, (f >> np.uint64(6)).astype(np.int64),
                     np.uint64(1) << (f & np.uint64(63)))
    return torch.from_numpy(w.view(np.int64).copy())


def bitmap_set_bits(words, mutant=None):
    """ascending list of set bits, by a loop over words and bits.
    mutant 'nobit63' never reports bit 63."""
    w = words.numpy().view(np.uint64)
    top = 63 if mutant == "nobit63" else 64
    out = []
    for i in np.nonzero(w)[0]:
        v = int(w[i])
        if v == (1 << 64) - 1:
            out += range(int(i) * 64, int(i) * 64 + top)
            continue
        out += [int(i) * 64 + b for b in range(top) if (v >> b) & 1]
    return out


def bitmap_compact_ref(words, start, cap, mutant=None):
    """(slots [cap] with -1 where nothing is written, count) for blocks
    appending in ascending order from `start`.
    mutant 'nobase' forgets to add the base of every block after the
    first, so later blocks write over the first one's slots."""
    slots = [-1] * cap
    off = start
    for blk in range((words.numel() + 1023) // 1024):
        bits = bitmap_set_bits(words[blk * 1024:(blk + 1) * 1024])
        base = start if (mutant == "nobase" and blk > 0) else off
        for j, b in enumerate(bits):
            if base + j < cap:
                slots[base + j] = blk * 65536 + b
        off += len(bits)
    return slots, off
