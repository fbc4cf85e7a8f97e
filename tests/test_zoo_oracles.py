"""CPU tier for ``zoo_oracles.py``: every oracle is held to the project's
own CPU path (equal on the exact sets, within the bound on the float
sets), and every wrong reference is shown to differ from its oracle, or
to leave the bound, on the inputs ``test_zoo_kernels_gpu.py`` uses. A
kernel that made one of those mistakes would therefore fail there.
"""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import zoo_oracles as zo

BF = torch.bfloat16


# ---------------------------------------------------------------------------
# quantile codec
# ---------------------------------------------------------------------------
def test_quantile_oracle_matches_cpu_codec():
    from lightctr_amd.utils.compress import QuantileCodec

    for name, table in zo.quantile_tables().items():
        codec = QuantileCodec.from_table(table) if name == "irregular" \
            else None
        if codec is None:
            codec = QuantileCodec.__new__(QuantileCodec)
            codec.levels, codec.table = table.numel(), table
        xs = [zo.quantile_inputs(table)]
        xs += [zo.quantile_sized(table, n) for n in zo.QUANT_SIZES]
        for x in xs:
            code = zo.quantile_encode_ref(x, table)
            assert torch.equal(code, codec.encode(x)), name
            assert int(code.max()) < table.numel()
            zo.check_bits(name, zo.quantile_decode_ref(code, table),
                          codec.decode(code))
        nan = torch.tensor([float("nan")])
        assert int(zo.quantile_encode_ref(nan, table)) == table.numel() - 1


def test_quantile_log_table_midpoints():
    """the 256-level log table at every midpoint and its fp32 neighbours"""
    from lightctr_amd.utils.compress import QuantileCodec

    codec = QuantileCodec(256, "log")
    m = zo.quantile_midpoints(codec.table)
    x = torch.from_numpy(np.concatenate(
        [m, np.nextafter(m, np.float32(np.inf)),
         np.nextafter(m, np.float32(-np.inf))]))
    code = zo.quantile_encode_ref(x, codec.table)
    assert torch.equal(code, codec.encode(x))
    # a value on a midpoint belongs to the lower level, its upper
    # neighbour to the next one
    assert torch.equal(code[:255].long(), torch.arange(255))
    assert torch.equal(code[255:510].long(), torch.arange(255) + 1)


def test_quantile_wrong_reference():
    for name, table in zo.quantile_tables().items():
        if table.numel() == 1:
            continue
        x = zo.quantile_inputs(table)
        assert zo.differs(zo.quantile_encode_ref(x, table),
                          zo.quantile_encode_ref(x, table, "lt")), name


# ---------------------------------------------------------------------------
# low-bit codec
# ---------------------------------------------------------------------------
def test_lowbit_oracle_matches_cpu_codec():
    from lightctr_amd.utils.compress import LowBitCodec

    for bits in (1, 2):
        codec = LowBitCodec(bits)
        for n in zo.LOWBIT_SIZES:
            x = zo.lowbit_inputs(n, seed=n + bits)
            # the CPU codec takes its threshold from mean|x|: finite input
            x = torch.where(torch.isfinite(x), x, torch.full_like(x, 2.0))
            words, meta, _ = codec.encode(x)
            lo, hi, th = meta
            th = 0.0 if bits == 1 else th
            want = zo.lowbit_pack_ref(x, th, bits)
            assert torch.equal(words, want), (bits, n)
            for lo_, hi_ in ((lo, hi), (0.0, 1.5)):
                zo.check_bits("lowbit_decode",
                              zo.lowbit_decode_ref(want, lo_, hi_, bits, n),
                              codec.decode(want, (lo_, hi_, th), n))


def test_lowbit_special_values():
    """+-0 both encode as positive, NaN as negative and small, +-thresh is
    large, the neighbour below it small"""
    th = np.float32(0.75)
    x = torch.from_numpy(np.array(
        [0.0, -0.0, np.nan, np.inf, -np.inf, th, -th,
         np.nextafter(th, np.float32(0)), np.nextafter(th, np.float32(1))],
        dtype=np.float32))
    codes2 = [1, 1, 0, 3, 2, 3, 2, 1, 3]
    w = zo.lowbit_pack_ref(x, 0.75, 2)
    assert w.tolist() == [sum(c << (2 * j) for j, c in enumerate(codes2))]
    w = zo.lowbit_pack_ref(x, 0.75, 1)
    assert w.tolist() == [sum((c & 1) << j for j, c in enumerate(codes2))]
    dec = zo.lowbit_decode_ref(zo.lowbit_pack_ref(x, 0.75, 2), 0.0, 1.5, 2, 9)
    assert math.copysign(1.0, float(dec[2])) == -1.0 and float(dec[2]) == 0.0
    assert dec.tolist()[3:7] == [1.5, -1.5, 1.5, -1.5]
    # the specials are present in the GPU test's own inputs
    xs = zo.lowbit_inputs(4097, seed=4098)
    assert xs.isnan().any() and xs.isinf().any()
    assert (xs == 0).any() and (xs.abs() == 0.75).any()


def test_lowbit_wrong_references():
    for bits in (1, 2):
        hit = {"droplast": 0, "padset": 0}
        for n in zo.LOWBIT_SIZES:
            x = zo.lowbit_inputs(n, seed=n + bits)
            ref = zo.lowbit_pack_ref(x, zo.LOWBIT_THRESH, bits)
            for m in hit:
                bad = zo.lowbit_pack_ref(x, zo.LOWBIT_THRESH, bits, m)
                hit[m] += not torch.equal(bad, ref)
        assert all(v >= 5 for v in hit.values()), hit


# ---------------------------------------------------------------------------
# ps_apply
# ---------------------------------------------------------------------------
def _shard_apply(st, updater, wi, lr, lam, eps):
    """PSShard._apply's CPU math on copies of st"""
    from lightctr_amd.parallel.ps import PSConfig, PSShard

    sh = PSShard.__new__(PSShard)
    sh.cfg = PSConfig(num_features=zo.PS_F, k=st["V"].shape[1],
                      updater=updater, lr=lr, dc_lambda=lam, eps=eps)
    sh.device = torch.device("cpu")
    sh.W, sh.V = st["W"].clone(), st["V"].clone()
    sh.nW, sh.nV = st["nW"].clone(), st["nV"].clone()
    sh.shadowW, sh.shadowV = st["shW"].clone(), st["shV"].clone()
    sh._apply(wi, st["lidx"], st["gW"], st["gV"])
    return {"W": sh.W, "V": sh.V, "nW": sh.nW, "nV": sh.nV,
            "shW": sh.shadowW, "shV": sh.shadowV}


@pytest.mark.parametrize("updater", zo.PS_UPDATERS)
def test_ps_oracle_matches_cpu_shard(updater):
    h = zo.PS_HYPER
    for K in zo.PS_KS:
        for n in zo.PS_NS:
            wi = (K + n) % 2
            st = zo.ps_inputs(K, n, seed=K * 10 + n)
            ref = zo.ps_apply_ref(st, updater, wi, **h)
            out = _shard_apply(st, updater, wi, **h)
            for name in zo.PS_STATE:
                zo.check_bound(f"ps.{updater}.{name}", out[name], *ref[name])
            # rows outside the key list carry a zero bound
            keep = zo.ps_untouched(zo.PS_F, st["lidx"])
            assert not ref["W"][1][keep].any()
            assert ref["W"][1][st["lidx"]].all()
            assert {0, zo.PS_F - 1} & set(st["lidx"].tolist())


def test_ps_exact_set_is_exact():
    for K in zo.PS_KS:
        for n in zo.PS_NS:
            st = zo.ps_inputs(K, n, seed=K * 10 + n, exact=True)
            ref = zo.ps_apply_ref(st, "sgd", 0, 0.5, 0.0, 0.0)
            out = _shard_apply(st, "sgd", 0, 0.5, 0.0, 0.0)
            for name in zo.PS_STATE:
                assert torch.equal(ref[name][0], out[name].double())


def test_ps_wrong_references():
    h = zo.PS_HYPER
    for updater in zo.PS_UPDATERS:
        for K in zo.PS_KS:
            st = zo.ps_inputs(K, 5, seed=K * 10 + 5)
            ref = zo.ps_apply_ref(st, updater, 1, **h)
            bad = zo.ps_apply_ref(st, updater, 1, mutant="w_small_k", **h)
            assert zo.differs(bad["W"][0], ref["W"][0], ref["W"][1]) \
                == (K >= 64), (updater, K)
            if updater.startswith("dcasgd"):
                bad = zo.ps_apply_ref(st, updater, 1, mutant="noshadow", **h)
                for name in ("shW", "shV"):
                    assert zo.differs(bad[name][0], ref[name][0],
                                      ref[name][1])
    # the exact set sees the W mistake too
    st = zo.ps_inputs(64, 3, seed=643, exact=True)
    assert zo.differs(
        zo.ps_apply_ref(st, "sgd", 0, 0.5, 0, 0)["W"][0],
        zo.ps_apply_ref(st, "sgd", 0, 0.5, 0, 0, mutant="w_small_k")["W"][0])


# ---------------------------------------------------------------------------
# histogram AUC
# ---------------------------------------------------------------------------
def test_auc_hist_oracle_matches_cpu_and_round_differs():
    from lightctr_amd.utils.metrics import HistAUC

    for buckets in zo.AUC_ADD_BUCKETS:
        n = 257
        pred, label = zo.auc_preds(buckets, n, seed=buckets % 97 + n % 89)
        want = zo.auc_hist_ref(pred, label, buckets)
        cpu = HistAUC(buckets)
        cpu.add(pred, label)
        cpu.add(pred, label)
        assert torch.equal(torch.cat([cpu.neg, cpu.pos]).long(), 2 * want)
        if buckets > 1:
            assert zo.differs(zo.auc_hist_ref(pred, label, buckets, "round"),
                              want), buckets
    pred, _ = zo.auc_preds(1000, 257, seed=1)
    assert pred.isinf().any() and (pred < 0).any() and (pred > 1).any()
    assert ((pred > 0) & (pred < 1e-38)).any()  # the subnormal


def test_auc_scan_oracle_matches_cpu_and_wrong_references():
    from lightctr_amd.utils.metrics import HistAUC

    hit = {"nocarry": 0, "signed": 0, "exclusive": 0, "notie": 0}
    names = set()
    for buckets in zo.AUC_SCAN_BUCKETS:
        for name, neg, pos in zo.auc_scan_hists(buckets):
            names.add(name)
            correct, P, N = zo.auc_scan_ref(neg, pos)
            cpu = HistAUC(buckets)
            cpu.neg = torch.tensor(neg, dtype=torch.float64)
            cpu.pos = torch.tensor(pos, dtype=torch.float64)
            want = correct / (P * N) if P and N else 0.5
            assert cpu.compute() == want, (buckets, name)
            t = zo.auc_hist_tensor(neg, pos)
            assert t.dtype == torch.int32 and t.numel() == 2 * buckets
            for m in hit:
                hit[m] += zo.auc_scan_ref(neg, pos, m) != (correct, P, N)
            if name == "big":
                assert max(pos) > 2 ** 31 and P > 2 ** 32
                assert int(t.min()) < 0  # stored as its int32 bit pattern
    assert all(v > 0 for v in hit.values()), hit
    assert {"carry", "carry_mirror", "big", "first", "last"} <= names


# ---------------------------------------------------------------------------
# gbm_hist
# ---------------------------------------------------------------------------
def test_gbm_oracle_matches_cpu_model():
    from lightctr_amd.models.gbm import GBMHyper, GBMModel

    m = GBMModel(GBMHyper())
    for i, (N, D, nn, place) in enumerate(zo.gbm_cases()):
        inp = zo.gbm_inputs(N, D, nn, place, seed=100 + i, exact=True)
        ref, _ = zo.gbm_hist_ref(*inp, nn, exact=True)
        assert torch.equal(m._hist(*inp, nn).double(), ref), (N, D, nn)
        inp = zo.gbm_inputs(N, D, nn, place, seed=200 + i, exact=False)
        ref, bound = zo.gbm_hist_ref(*inp, nn, exact=False)
        zo.check_bound("gbm_hist.cpu", m._hist(*inp, nn), ref, bound)


def test_gbm_wrong_references():
    for i, (N, D, nn, place) in enumerate(zo.gbm_cases()):
        if place in ("none",):
            continue
        second_trip = N > zo.gbm_zsplit(D, nn) * 256
        for exact, seed in ((True, 100 + i), (False, 200 + i)):
            inp = zo.gbm_inputs(N, D, nn, place, seed=seed, exact=exact)
            ref, bound = zo.gbm_hist_ref(*inp, nn, exact=exact)
            bad = zo.gbm_hist_ref(*inp, nn, exact=exact, mutant="dropfeat")[0]
            if N >= 255:
                assert zo.differs(bad, ref, bound) == (D % 4 != 0), (N, D)
            if second_trip and int(inp[3][-1]) >= 0:
                bad = zo.gbm_hist_ref(*inp, nn, exact=exact,
                                      mutant="droptrip")[0]
                assert zo.differs(bad, ref, bound), (N, D, nn)
    trips = [c for c in zo.gbm_cases() if c[0] > zo.gbm_zsplit(c[1], c[2])
             * 256]
    assert len(trips) >= 2


# ---------------------------------------------------------------------------
# im2col / col2im
# ---------------------------------------------------------------------------
def _unfold(x, k, s, p):
    B, C = x.shape[:2]
    u = Fn.unfold(x, k, padding=p, stride=s)  # [B, C k k, L]
    return u.transpose(1, 2).reshape(-1, C * k * k)


def test_im2col_oracle_matches_unfold():
    for i, c in enumerate(zo.conv_cases() + [zo.CONV_BIG]):
        B, C, H, W, k, s, p = c
        x = zo.conv_x(B, C, H, W, seed=300 + i)
        want = _unfold(x.to(BF).float(), k, s, p).to(BF)
        zo.check_bits(f"im2col.{c}", zo.im2col_ref(x, k, s, p), want)
    x = zo.conv_x(*zo.CONV_BASE[:4], seed=300)
    bits = x.view(torch.int32)
    ties = (bits & 0xFFFF) == 0x8000
    assert (ties & ((bits >> 16) & 1 == 0)).any()   # rounds down to even
    assert (ties & ((bits >> 16) & 1 == 1)).any()   # rounds up to even
    assert x.isinf().any() and not x.isnan().any()
    assert ((x == 0) & torch.signbit(x)).any()


def test_col2im_oracle_matches_fold():
    for i, c in enumerate(zo.conv_cases() + [zo.CONV_BIG, zo.COL2IM_BIG]):
        B, C, H, W, k, s, p = c
        L = zo.conv_out(H, W, k, s, p)
        for exact, seed in ((True, 400 + i), (False, 600 + i)):
            dcol = zo.conv_dcol(*c, seed=seed, exact=exact)
            ref, bound = zo.col2im_ref(dcol, *c, exact=exact)
            cols = dcol.double().view(B, L[0] * L[1], C * k * k)
            fold = Fn.fold(cols.transpose(1, 2), (H, W), k, padding=p,
                           stride=s)
            if exact:
                assert torch.equal(fold, ref), c
            else:
                zo.check_bound("col2im.fold", fold, ref, bound)
        if B * C * H * W < 5000:
            g = zo.col2im_gather_ref(dcol, *c)
            assert not zo.differs(g, ref, bound), c


def test_conv_adjoint_identity_in_integers():
    for i, c in enumerate(zo.conv_cases()):
        B, C, H, W, k, s, p = c
        x = zo.conv_x(B, C, H, W, seed=500 + i, integer=True)
        dcol = zo.conv_dcol(*c, seed=400 + i, exact=True)
        col = zo.im2col_ref(x, k, s, p).double()
        dx = zo.col2im_ref(dcol, *c, exact=True)[0]
        assert int((col * dcol.double()).sum()) == int((x.double() * dx).sum())


def test_conv_wrong_references():
    hit = {m: 0 for m in ("hw_swap", "k_swap", "nopad")}
    hit2 = {m: 0 for m in ("hw_swap", "k_swap", "nomod", "noguard")}
    for i, c in enumerate(zo.conv_cases()):
        B, C, H, W, k, s, p = c
        x = zo.conv_x(B, C, H, W, seed=300 + i)
        ref = zo.im2col_ref(x, k, s, p).float()
        for m in hit:
            hit[m] += zo.differs(zo.im2col_ref(x, k, s, p, m).float(), ref)
        dcol = zo.conv_dcol(*c, seed=400 + i, exact=True)
        dref = zo.col2im_ref(dcol, *c, exact=True)[0]
        for m in hit2:
            hit2[m] += zo.differs(zo.col2im_gather_ref(dcol, *c, mutant=m),
                                  dref)
    n = len(zo.conv_cases())
    assert hit["hw_swap"] == n, hit     # shows everywhere: H != W
    assert hit2["hw_swap"] == n, hit2
    assert hit["k_swap"] >= n - 4 and hit2["k_swap"] >= n - 4  # k >= 2
    assert hit["nopad"] >= 10           # every case with padding
    assert hit2["nomod"] >= 5           # every case with s >= 2
    assert hit2["noguard"] >= 3, hit2
    assert any(bool(zo.conv_uncovered(*c).any()) for c in zo.conv_cases())


# ---------------------------------------------------------------------------
# w2v_negsample_step
# ---------------------------------------------------------------------------
W2V_CASES = [(D, 4, 3, 5) for D in zo.W2V_DS] \
    + [(16, C, N, 5) for C in zo.W2V_CS for N in zo.W2V_NS] \
    + [(16, 4, 3, B) for B in zo.W2V_BS] + [(64, 1, 5, 9)]


def _w2v_seed(D, C, N, B):
    return D * 1000 + C * 100 + N * 10 + B


def _torch_loop(inp, lr, scale):
    """the loop of test_w2v_negsample_kernel_single_example_parity, in
    float64, one example after the other"""
    E2, O2 = inp["E"].double().clone(), inp["O"].double().clone()
    B, C = inp["ctx"].shape
    N = inp["negs"].shape[1]
    loss = []
    for b in range(B):
        ctx = inp["ctx"][b]
        x = E2[ctx].mean(dim=0)
        tgts = torch.cat([inp["centers"][b:b + 1], inp["negs"][b]])
        ys = torch.tensor([1.0] + [0.0] * N, dtype=torch.float64)
        gx = torch.zeros(E2.shape[1], dtype=torch.float64)
        ref_loss = 0.0
        for t, y in zip(tgts, ys):
            dot = (x * O2[t]).sum().clamp(-16, 16)
            p = torch.sigmoid(dot)
            ref_loss += float(-(y * p.log() + (1 - y) * (1 - p).log()))
            gz = (p - y) * scale
            gx += gz * O2[t]
            O2[t] -= lr * gz * x
        for c in ctx:
            E2[c] -= lr * gx / C
        loss.append(ref_loss)
    return E2, O2, torch.tensor(loss, dtype=torch.float64)


def test_w2v_oracle_matches_torch_loop():
    lr, scale = zo.f32(zo.W2V_LR), zo.f32(zo.W2V_SCALE)
    for D, C, N, B in W2V_CASES:
        inp = zo.w2v_inputs(D, C, N, B, seed=_w2v_seed(D, C, N, B))
        ref = zo.w2v_ref(inp, lr, scale)
        E2, O2, loss = _torch_loop(inp, lr, scale)
        for name, got in (("E", E2), ("O", O2), ("loss", loss)):
            r = ref[name][0]
            assert torch.allclose(got, r, rtol=1e-12, atol=1e-13), name
            # the kernel's bound dwarfs the float64 noise between the two
            assert (ref[name][1] >= 0).all()
        # structure the GPU test relies on
        e_used, o_used = zo.w2v_used(inp)
        sets = [set(inp["ctx"][b].tolist()) | {int(inp["centers"][b])}
                | set(inp["negs"][b].tolist()) for b in range(B)]
        assert sum(len(s) for s in sets) == len(set().union(*sets))
        assert e_used.numel() < inp["E"].shape[0]
        if C >= 2:
            assert int(inp["ctx"][0, 0]) == int(inp["ctx"][0, C - 1])
        if N >= 1 and B >= 2:
            assert int(inp["negs"][1, 0]) == int(inp["centers"][1])
        if N >= 3:
            assert int(inp["negs"][0, 1]) == int(inp["negs"][0, 2])
        x = inp["E"][inp["ctx"][0]].double().mean(0)
        assert float((x * inp["O"][inp["centers"][0]].double()).sum()) < -17


def test_w2v_sweep_dots_are_exact():
    inp = zo.w2v_sweep_inputs()
    d = inp["E"].view(-1)
    assert float(d.min()) == -17.0 and float(d.max()) == 17.0
    assert torch.equal(d * 4, (d * 4).round())
    assert (inp["O"] == 1).all() and inp["negs"].shape == (137, 0)


def test_w2v_wrong_references_leave_the_bound():
    muts = ("no_inv_c", "neg_y1", "gx_updated", "noclamp", "drop_ctx",
            "drop_dim")
    hit = {m: 0 for m in muts}
    for D, C, N, B in W2V_CASES:
        inp = zo.w2v_inputs(D, C, N, B, seed=_w2v_seed(D, C, N, B))
        ref = zo.w2v_ref(inp, zo.W2V_LR, zo.W2V_SCALE)
        for m in muts:
            bad = zo.w2v_ref(inp, zo.W2V_LR, zo.W2V_SCALE, mutant=m)
            hit[m] += any(zo.differs(bad[k][0], ref[k][0], ref[k][1])
                          for k in ("E", "O", "loss"))
    n = len(W2V_CASES)
    assert hit["noclamp"] == n, hit            # example 0's dot is ~ -20
    assert hit["no_inv_c"] >= n - 5, hit       # every C = 4 case
    assert hit["drop_ctx"] >= n - 5, hit
    assert hit["neg_y1"] >= n - 3, hit         # every N >= 1 case
    assert hit["gx_updated"] >= n - 3, hit
    assert hit["drop_dim"] >= n - 2, hit       # every D >= 2 case


# ---------------------------------------------------------------------------
# bitmap_compact / inv_perm
# ---------------------------------------------------------------------------
def test_bitmap_oracle_matches_unique_and_wrong_references():
    hit = {"nobit63": 0, "nobase": 0}
    for nwords in zo.BITMAP_NWORDS:
        for pat in zo.BITMAP_PATTERNS:
            fids = zo.bitmap_fids(nwords, pat, seed=nwords)
            words = zo.bitmap_words(nwords, fids)
            assert words.dtype == torch.int64 and words.numel() == nwords
            bits = zo.bitmap_set_bits(words)
            assert bits == torch.unique(fids).tolist(), (nwords, pat)
            slots, count = zo.bitmap_compact_ref(words, 0, len(bits))
            assert slots == bits and count == len(bits)
            hit["nobit63"] += zo.bitmap_set_bits(words, "nobit63") != bits
            bad, _ = zo.bitmap_compact_ref(words, 0, len(bits), "nobase")
            hit["nobase"] += sorted(bad) != bits
            if pat == "full_block":
                assert len(bits) == min(nwords, 1024) * 64
    assert hit["nobit63"] >= 16 and hit["nobase"] >= 4, hit


def test_inv_perm_definition():
    for n in zo.INV_PERM_NS:
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(n))
        inv = torch.empty(n, dtype=torch.long)
        inv[perm] = torch.arange(n)
        assert torch.equal(inv, torch.argsort(perm))
