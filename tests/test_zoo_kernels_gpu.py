"""Parity of the codec, sparse-PS, AUC, GBM-histogram, conv, word2vec and
compaction kernels with the oracles of ``zoo_oracles.py``, at the shapes
each kernel's own loop constants make interesting, plus the host-side
checks of their bindings.

Every ``at::empty`` output is produced right after ``poison`` of a block of
its exact shape and dtype; every state tensor is compared bit for bit
outside the rows an op may touch. Each test loops over its cases.
"""

import numpy as np
import pytest
import torch

import zoo_oracles as zo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def poison(shape, dtype):
    zo.poison(shape, dtype, DEV)


def poison_int(n, dtype):
    """the integer form of poison: all-ones bytes"""
    fill = 255 if dtype == torch.uint8 else -1
    p = torch.full((n,), fill, dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    del p


# ---------------------------------------------------------------------------
# quantile codec
# ---------------------------------------------------------------------------
def test_quantile_codec():
    """codes equal the linear-scan oracle; decode is table[code] bit for
    bit. Decode is fed only the codes encode produced (< levels)."""
    for name, table in zo.quantile_tables().items():
        tab = table.to(DEV)
        xs = [zo.quantile_inputs(table)]
        xs += [zo.quantile_sized(table, n) for n in zo.QUANT_SIZES]
        for x in xs:
            want = zo.quantile_encode_ref(x, table)
            xd = x.to(DEV)
            poison_int(x.numel(), torch.uint8)
            code = ops().quantile_encode(xd, tab)
            assert torch.equal(code.cpu(), want), (name, x.numel())
            poison((x.numel(),), torch.float32)
            dec = ops().quantile_decode(code, tab)
            zo.check_bits(f"quantile_decode.{name}", dec,
                          zo.quantile_decode_ref(want, table))
        # a contiguous view that starts at element 1
        x = zo.quantile_sized(table, 258)
        view = x.to(DEV)[1:]
        assert view.is_contiguous() and view.storage_offset() == 1
        code = ops().quantile_encode(view, tab)
        assert torch.equal(code.cpu(), zo.quantile_encode_ref(x[1:], table))
        dec = ops().quantile_decode(code.clone()[1:], tab)
        zo.check_bits("quantile_decode.view", dec,
                      table[zo.quantile_encode_ref(x[2:], table).long()])


# ---------------------------------------------------------------------------
# low-bit codec
# ---------------------------------------------------------------------------
def test_lowbit_codec():
    """words equal Python-int packing with zero padding bits; decode is
    bit-exact, with lo = 0 (negative sign gives -0.0), lo != hi, and a
    words tensor longer than needed."""
    th = zo.LOWBIT_THRESH
    for bits in (1, 2):
        for n in zo.LOWBIT_SIZES:
            x = zo.lowbit_inputs(n, seed=n + bits)
            want = zo.lowbit_pack_ref(x, th, bits)
            xd = x.to(DEV)
            poison_int(want.numel(), torch.int32)
            words = ops().lowbit_encode(xd, th, bits)
            assert words.dtype == torch.int32
            assert torch.equal(words.cpu(), want), (bits, n)
            for lo, hi in ((0.0, 1.5), (0.25, 1.5)):
                poison((n,), torch.float32)
                dec = ops().lowbit_decode(words, lo, hi, bits, n)
                zo.check_bits(f"lowbit_decode.b{bits}.n{n}", dec,
                              zo.lowbit_decode_ref(want, lo, hi, bits, n))
            longer = torch.cat([words, torch.full((3,), -1, dtype=torch.int32,
                                                  device=DEV)])
            poison((n,), torch.float32)
            dec = ops().lowbit_decode(longer, 0.25, 1.5, bits, n)
            zo.check_bits("lowbit_decode.longer", dec,
                          zo.lowbit_decode_ref(want, 0.25, 1.5, bits, n))


# ---------------------------------------------------------------------------
# ps_apply
# ---------------------------------------------------------------------------
def _ps_run(st, updater, wi, lr, lam, eps):
    """run the kernel on copies of st the way PSShard._apply calls it;
    returns the six state arrays on the CPU"""
    d = {k: st[k].to(DEV) for k in zo.PS_STATE}
    upd = zo.PS_UPDATERS.index(updater)
    acc = updater in ("adagrad", "dcasgda")
    sh = updater.startswith("dcasgd")
    ops().ps_apply(st["lidx"].to(DEV), st["gW"].to(DEV), st["gV"].to(DEV),
                   d["W"], d["V"],
                   d["nW"] if acc else None, d["nV"] if acc else None,
                   d["shW"][wi] if sh else None,
                   d["shV"][wi] if sh else None, upd, lr, lam, eps)
    return {k: v.cpu() for k, v in d.items()}


def _ps_check_untouched(out, st, updater, wi, tag):
    keep = zo.ps_untouched(zo.PS_F, st["lidx"])
    for name in zo.PS_STATE:
        if name not in zo.PS_OWNS[updater]:
            zo.check_bits(f"{tag}.{name}.notowned", out[name], st[name])
        elif name.startswith("sh"):
            zo.check_bits(f"{tag}.{name}.other", out[name][1 - wi],
                          st[name][1 - wi])
            zo.check_bits(f"{tag}.{name}.rows", out[name][wi][keep],
                          st[name][wi][keep])
        else:
            zo.check_bits(f"{tag}.{name}.rows", out[name][keep],
                          st[name][keep])


def test_ps_apply_exact_sgd():
    """lr = 0.5 on integer state and gradients: every value is exact"""
    for K in zo.PS_KS:
        for n in zo.PS_NS:
            for wi in (0, 1):
                st = zo.ps_inputs(K, n, seed=K * 10 + n, exact=True)
                ref = zo.ps_apply_ref(st, "sgd", wi, 0.5, 0.0, 0.0)
                out = _ps_run(st, "sgd", wi, 0.5, 0.0, 0.0)
                tag = f"ps_apply.sgd.K{K}.n{n}"
                for name in zo.PS_STATE:
                    exp = ref[name][0]
                    assert torch.equal(exp, exp.float().double())
                    zo.check_bits(f"{tag}.{name}", out[name], exp.float())
                assert not torch.equal(out["W"], st["W"])


@pytest.mark.parametrize("updater", zo.PS_UPDATERS)
def test_ps_apply_float(updater):
    h = zo.PS_HYPER
    for K in zo.PS_KS:
        for n in zo.PS_NS:
            wi = (K + n) % 2
            st = zo.ps_inputs(K, n, seed=K * 10 + n)
            ref = zo.ps_apply_ref(st, updater, wi, **h)
            out = _ps_run(st, updater, wi, **h)
            tag = f"ps_apply.{updater}"
            for name in zo.PS_OWNS[updater]:
                zo.check_bound(f"{tag}.{name}", out[name], *ref[name])
            _ps_check_untouched(out, st, updater, wi, f"{tag}.K{K}.n{n}")
            if updater.startswith("dcasgd"):
                rows = st["lidx"]
                zo.check_bits(f"{tag}.shW==W", out["shW"][wi][rows],
                              out["W"][rows])
                zo.check_bits(f"{tag}.shV==V", out["shV"][wi][rows],
                              out["V"][rows])


# ---------------------------------------------------------------------------
# histogram AUC
# ---------------------------------------------------------------------------
def test_auc_hist_add():
    from lightctr_amd.utils.metrics import HistAUC

    cases = [(b, 257) for b in zo.AUC_ADD_BUCKETS]
    cases += [(1000, n) for n in zo.AUC_ADD_NS]
    cases += [(1 << 20, (1 << 20) + 1)]
    for buckets, n in cases:
        pred, label = zo.auc_preds(buckets, n, seed=buckets % 97 + n % 89)
        want = zo.auc_hist_ref(pred, label, buckets)
        assert int(want.sum()) == n
        hist = torch.zeros(2 * buckets, dtype=torch.int32, device=DEV)
        pd, ld = pred.to(DEV), label.to(DEV)
        ops().auc_hist_add(pd, ld, hist)
        assert torch.equal(hist.cpu().long(), want), (buckets, n)
        # a second call accumulates
        ops().auc_hist_add(pd, ld, hist)
        assert torch.equal(hist.cpu().long(), 2 * want), (buckets, n)
        # the project's CPU path on the same fp32 tensor
        cpu = HistAUC(buckets)
        cpu.add(pred, label)
        assert torch.equal(torch.cat([cpu.neg, cpu.pos]).long(), want)


def test_auc_scan():
    from lightctr_amd.utils.metrics import HistAUC

    for buckets in zo.AUC_SCAN_BUCKETS:
        for name, neg, pos in zo.auc_scan_hists(buckets):
            correct, P, N = zo.auc_scan_ref(neg, pos)
            hist = zo.auc_hist_tensor(neg, pos).to(DEV)
            poison((3,), torch.float64)
            out = ops().auc_scan(hist).cpu()
            assert out.dtype == torch.float64
            assert out.tolist() == [correct, P, N], (buckets, name)
            m = HistAUC(buckets, DEV)
            m.hist = hist
            want = correct / (P * N) if P and N else 0.5
            assert m.compute() == want, (buckets, name)


# ---------------------------------------------------------------------------
# gbm_hist
# ---------------------------------------------------------------------------
def _gbm_run(bins, grad, hess, node, n_nodes):
    return ops().gbm_hist(bins.to(DEV), grad.to(DEV), hess.to(DEV),
                          node.to(DEV), n_nodes).cpu()


def test_gbm_hist_exact():
    for i, (N, D, nn, place) in enumerate(zo.gbm_cases()):
        inp = zo.gbm_inputs(N, D, nn, place, seed=100 + i, exact=True)
        ref, _ = zo.gbm_hist_ref(*inp, nn, exact=True)
        out = _gbm_run(*inp, nn)
        assert out.shape == (nn, D, 256, 2)
        assert torch.equal(out.double(), ref), (N, D, nn, place)
        if place == "none":
            assert not out.any()


def test_gbm_hist_float():
    for i, (N, D, nn, place) in enumerate(zo.gbm_cases()):
        inp = zo.gbm_inputs(N, D, nn, place, seed=200 + i, exact=False)
        ref, bound = zo.gbm_hist_ref(*inp, nn, exact=False)
        zo.check_bound("gbm_hist.float", _gbm_run(*inp, nn), ref, bound)


# ---------------------------------------------------------------------------
# im2col_bf16 / col2im
# ---------------------------------------------------------------------------
def test_im2col_bf16():
    for i, (B, C, H, W, k, s, p) in enumerate(zo.conv_cases()
                                              + [zo.CONV_BIG]):
        x = zo.conv_x(B, C, H, W, seed=300 + i)
        want = zo.im2col_ref(x, k, s, p)
        xd = x.to(DEV)
        poison(tuple(want.shape), BF)
        col = ops().im2col_bf16(xd, k, s, p)
        zo.check_bits(f"im2col.{(B, C, H, W, k, s, p)}", col, want)


def test_col2im_exact_and_adjoint():
    """integer dcol: value equality with the scatter-add oracle, +0 over
    poisoned memory at pixels no patch covers, and
    <im2col(x), dcol> == <x, col2im(dcol)> in integers"""
    saw_bare = False
    for i, c in enumerate(zo.conv_cases() + [zo.CONV_BIG, zo.COL2IM_BIG]):
        B, C, H, W, k, s, p = c
        dcol = zo.conv_dcol(*c, seed=400 + i, exact=True)
        ref, _ = zo.col2im_ref(dcol, *c, exact=True)
        dd = dcol.to(DEV)
        poison((B, C, H, W), torch.float32)
        dx = ops().col2im(dd, B, C, H, W, k, s, p).cpu()
        assert torch.equal(dx.double(), ref), c
        bare = zo.conv_uncovered(*c)
        saw_bare |= bool(bare.any())
        zo.check_bits(f"col2im.bare.{c}", dx[bare],
                      torch.zeros(int(bare.sum())))
        x = zo.conv_x(B, C, H, W, seed=500 + i, integer=True)
        col = ops().im2col_bf16(x.to(DEV), k, s, p).cpu()
        lhs = int((col.double() * dcol.double()).sum())
        rhs = int((x.double() * dx.double()).sum())
        assert lhs == rhs, c
    assert saw_bare


def test_col2im_float():
    for i, c in enumerate(zo.conv_cases() + [zo.CONV_BIG]):
        B, C, H, W, k, s, p = c
        dcol = zo.conv_dcol(*c, seed=600 + i, exact=False)
        ref, bound = zo.col2im_ref(dcol, *c, exact=False)
        dd = dcol.to(DEV)
        poison((B, C, H, W), torch.float32)
        zo.check_bound("col2im.float", ops().col2im(dd, B, C, H, W, k, s, p),
                       ref, bound)


# ---------------------------------------------------------------------------
# w2v_negsample_step
# ---------------------------------------------------------------------------
def _w2v_run(inp, lr, scale):
    E, O = inp["E"].to(DEV), inp["O"].to(DEV)
    idx = [inp[k].to(DEV) for k in ("centers", "ctx", "negs")]
    poison((inp["centers"].numel(),), torch.float32)
    loss = ops().w2v_negsample_step(E, O, *idx, lr, scale)
    return E.cpu(), O.cpu(), loss.cpu()


def test_w2v_intrinsic_sweep():
    """N = 0, exact dots over [-17, 17]: loss = -log p, so |loss - loss64|
    is the relative deviation of p through __expf, the reciprocal and
    __logf. It must stay within 4x the deviation measured on the MI355X
    (W2V_INTRINSIC_MEASURED, see docs/TESTING.md)."""
    inp = zo.w2v_sweep_inputs()
    _, _, loss = _w2v_run(inp, 0.0, 1.0)
    dots = inp["E"].double().view(-1).clamp(-16, 16)
    ref = torch.log1p(torch.exp(-dots))
    dev = (loss.double() - ref).abs()
    print(f"W2V_INTRINSIC worst |loss - loss64| = {float(dev.max()):.6g} "
          f"= 2^{np.log2(max(float(dev.max()), 1e-300)):.2f} at dot "
          f"{float(dots[dev.argmax()])}")
    assert float(dev.max()) <= zo.W2V_INTRINSIC_REL


def test_w2v_negsample_step():
    cases = [(D, 4, 3, 5) for D in zo.W2V_DS]
    cases += [(16, C, N, 5) for C in zo.W2V_CS for N in zo.W2V_NS]
    cases += [(16, 4, 3, B) for B in zo.W2V_BS] + [(64, 1, 5, 9)]
    for D, C, N, B in cases:
        inp = zo.w2v_inputs(D, C, N, B, seed=D * 1000 + C * 100 + N * 10 + B)
        ref = zo.w2v_ref(inp, zo.W2V_LR, zo.W2V_SCALE)
        E, O, loss = _w2v_run(inp, zo.W2V_LR, zo.W2V_SCALE)
        tag = f"w2v.D{D}.C{C}.N{N}.B{B}"
        zo.check_bound("w2v.loss", loss, *ref["loss"])
        zo.check_bound("w2v.O", O, *ref["O"])
        zo.check_bound("w2v.E", E, *ref["E"])
        e_used, o_used = zo.w2v_used(inp)
        keep = torch.ones(E.shape[0], dtype=torch.bool)
        keep[e_used] = False
        zo.check_bits(f"{tag}.E.unused", E[keep], inp["E"][keep])
        keep = torch.ones(O.shape[0], dtype=torch.bool)
        keep[o_used] = False
        zo.check_bits(f"{tag}.O.unused", O[keep], inp["O"][keep])
        assert not torch.equal(E, inp["E"]) and not torch.equal(O, inp["O"])


# ---------------------------------------------------------------------------
# bitmap_compact / inv_perm_i32
# ---------------------------------------------------------------------------
SENT = -7


def _compact(words, start, cap, extra=0):
    """run bitmap_compact with out_fids a [cap] view of a sentinel-filled
    buffer `extra` longer; returns (buffer, count, bitmap after)"""
    buf = torch.full((cap + extra,), SENT, dtype=torch.int32, device=DEV)
    count = torch.tensor([start], dtype=torch.int32, device=DEV)
    bm = words.to(DEV)
    ret = ops().bitmap_compact(bm, buf[:cap], count)
    assert ret.data_ptr() == count.data_ptr()
    return buf.cpu(), int(count.cpu()), bm.cpu()


def _check_block_order(lst):
    """each 1024-word block appends one ascending, contiguous run"""
    blocks = [f // 65536 for f in lst]
    runs = [b for i, b in enumerate(blocks) if i == 0 or b != blocks[i - 1]]
    assert len(runs) == len(set(runs)), "a block's run is split"
    for i in range(1, len(lst)):
        if blocks[i] == blocks[i - 1]:
            assert lst[i] > lst[i - 1], "not ascending inside a block"


def test_bitmap_compact():
    for nwords in zo.BITMAP_NWORDS:
        for pat in zo.BITMAP_PATTERNS:
            fids = zo.bitmap_fids(nwords, pat, seed=nwords)
            words = zo.bitmap_words(nwords, fids)
            bits = zo.bitmap_set_bits(words)
            total = len(bits)
            tag = (nwords, pat)
            for start in (0, 5):
                cap = start + total + 3
                buf, count, after = _compact(words, start, cap, extra=4)
                assert count == start + total, tag
                assert not after.any(), tag
                lst = buf[start:start + total].tolist()
                assert sorted(lst) == bits, tag
                _check_block_order(lst)
                assert (buf[:start] == SENT).all(), tag
                assert (buf[start + total:] == SENT).all(), tag
            if total >= 2:
                cap = total // 2
                buf, count, after = _compact(words, 0, cap, extra=64)
                assert count == total, tag   # the true total
                assert not after.any(), tag
                got = buf[:cap].tolist()
                assert len(set(got)) == cap and set(got) <= set(bits), tag
                assert (buf[cap:] == SENT).all(), tag


def test_inv_perm_i32():
    for n in zo.INV_PERM_NS:
        g = torch.Generator().manual_seed(n)
        for dtype in (torch.int32, torch.int64):
            perm = torch.randperm(n, generator=g).to(dtype)
            pd = perm.to(DEV)
            poison_int(n, torch.int32)
            inv = ops().inv_perm_i32(pd).cpu()
            assert inv.dtype == torch.int32
            assert torch.equal(inv[perm.long()].long(), torch.arange(n))


# ---------------------------------------------------------------------------
# host-side checks: each fails before anything is launched
# ---------------------------------------------------------------------------
def _f(*shape):
    return torch.zeros(*shape, device=DEV)


def test_empty_inputs_launch_nothing():
    """n = 0 returns without a launch and leaves no error behind for the
    next checked binding to report"""
    tab = zo.quantile_tables()["uniform16"].to(DEV)
    code = ops().quantile_encode(_f(0), tab)
    assert code.shape == (0,) and code.dtype == torch.uint8
    assert ops().quantile_decode(code, tab).shape == (0,)
    for bits in (1, 2):
        w = ops().lowbit_encode(_f(0), 0.5, bits)
        assert w.shape == (0,) and w.dtype == torch.int32
        assert ops().lowbit_decode(w, 0.0, 1.0, bits, 0).shape == (0,)
    h = ops().gbm_hist(torch.zeros(0, 5, dtype=torch.uint8, device=DEV),
                       _f(0), _f(0),
                       torch.zeros(0, dtype=torch.int32, device=DEV), 3)
    assert h.shape == (3, 5, 256, 2) and not h.any()
    W, V = _f(4) + 1, _f(4, 8) + 1
    ops().ps_apply(torch.zeros(0, dtype=torch.long, device=DEV), _f(0),
                   _f(0, 8), W, V, None, None, None, None, 0, 0.5, 0.0, 0.0)
    assert (W == 1).all() and (V == 1).all()
    hist = torch.zeros(8, dtype=torch.int32, device=DEV)
    ops().auc_hist_add(_f(0), _f(0), hist)
    assert not hist.any()
    assert ops().inv_perm_i32(
        torch.zeros(0, dtype=torch.int32, device=DEV)).shape == (0,)
    # the next checked launch reports nothing
    assert ops().auc_scan(hist).tolist() == [0.0, 0.0, 0.0]
    torch.cuda.synchronize()


def test_codec_binding_checks():
    tab = zo.quantile_tables()["uniform16"].to(DEV)
    x = _f(8)
    code = torch.zeros(8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="1 or 2"):
        ops().lowbit_encode(x, 0.5, 0)
    with pytest.raises(RuntimeError, match="1 or 2"):
        ops().lowbit_encode(x, 0.5, 3)
    words = torch.zeros(1, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="1 or 2"):
        ops().lowbit_decode(words, 0.0, 1.0, 4, 8)
    with pytest.raises(RuntimeError, match="int32"):
        ops().lowbit_decode(words.long(), 0.0, 1.0, 1, 8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops().lowbit_decode(words.cpu(), 0.0, 1.0, 1, 8)
    with pytest.raises(RuntimeError, match="words"):
        ops().lowbit_decode(words, 0.0, 1.0, 1, 33)   # needs 2 words
    with pytest.raises(RuntimeError, match="words"):
        ops().lowbit_decode(words, 0.0, 1.0, 2, 17)   # needs 2 words
    with pytest.raises(RuntimeError, match=">= 0"):
        ops().lowbit_decode(words, 0.0, 1.0, 1, -1)
    with pytest.raises(RuntimeError, match="uint8"):
        ops().quantile_decode(code.int(), tab)
    with pytest.raises(RuntimeError, match="GPU"):
        ops().quantile_decode(code.cpu(), tab)
    for bad in (_f(0), _f(257)):
        with pytest.raises(RuntimeError, match="1..256"):
            ops().quantile_encode(x, bad)
        with pytest.raises(RuntimeError, match="1..256"):
            ops().quantile_decode(code, bad)


def test_ps_apply_binding_checks():
    F, K, n = 6, 8, 3
    lidx = torch.tensor([0, 2, 5], device=DEV)
    ok = dict(lidx=lidx, gW=_f(n), gV=_f(n, K), W=_f(F), V=_f(F, K),
              nW=_f(F), nV=_f(F, K), shW=_f(F), shV=_f(F, K))

    def call(updater=3, **kw):
        a = dict(ok, **kw)
        ops().ps_apply(a["lidx"], a["gW"], a["gV"], a["W"], a["V"], a["nW"],
                       a["nV"], a["shW"], a["shV"], updater, 0.05, 0.1, 1e-8)

    call()  # the well-formed call passes
    for updater in (-1, 4):
        with pytest.raises(RuntimeError, match="updater"):
            call(updater=updater)
    # the state each updater needs
    with pytest.raises(RuntimeError, match="nW and nV"):
        call(updater=1, nW=None)
    with pytest.raises(RuntimeError, match="nW and nV"):
        call(updater=3, nV=None)
    with pytest.raises(RuntimeError, match="shadowW and shadowV"):
        call(updater=2, shW=None)
    with pytest.raises(RuntimeError, match="shadowW and shadowV"):
        call(updater=3, shV=None)
    # dtype, device, contiguity, shape of every array
    with pytest.raises(RuntimeError, match="lidx"):
        call(lidx=lidx.int())
    with pytest.raises(RuntimeError, match="lidx"):
        call(lidx=lidx.cpu())
    with pytest.raises(RuntimeError, match="lidx"):
        call(lidx=torch.arange(6, device=DEV)[::2])
    for name in ("gW", "gV", "W", "V", "nW", "nV", "shW", "shV"):
        with pytest.raises(RuntimeError, match="fp32"):
            call(**{name: ok[name].double()})
        with pytest.raises(RuntimeError, match="GPU"):
            call(**{name: ok[name].cpu()})
        with pytest.raises(RuntimeError):
            call(**{name: torch.cat([ok[name], ok[name][:1]])})
    with pytest.raises(RuntimeError, match="contiguous"):
        call(V=_f(K, F).t())
    with pytest.raises(RuntimeError, match="contiguous"):
        call(gV=_f(K, n).t())
    with pytest.raises(RuntimeError, match="contiguous"):
        call(shV=_f(K, F).t())
    with pytest.raises(RuntimeError):
        call(V=_f(F, K + 1))


def test_gbm_hist_binding_checks():
    N, D = 10, 5
    bins = torch.zeros(N, D, dtype=torch.uint8, device=DEV)
    node = torch.zeros(N, dtype=torch.int32, device=DEV)
    g = _f(N)
    for nn in (0, -1, 65536):
        with pytest.raises(RuntimeError, match="n_nodes"):
            ops().gbm_hist(bins, g, g, node, nn)
    with pytest.raises(RuntimeError, match="bins"):
        ops().gbm_hist(bins.view(-1), g, g, node, 2)
    with pytest.raises(RuntimeError, match="bins"):
        ops().gbm_hist(torch.zeros(D, N, dtype=torch.uint8, device=DEV).t(),
                       g, g, node, 2)
    with pytest.raises(RuntimeError, match="N = 10"):
        ops().gbm_hist(bins, _f(N - 1), g, node, 2)
    with pytest.raises(RuntimeError, match="N = 10"):
        ops().gbm_hist(bins, g, _f(N + 1), node, 2)
    with pytest.raises(RuntimeError, match="N = 10"):
        ops().gbm_hist(bins, g, g, node[:-1], 2)


def test_bitmap_and_conv_binding_checks():
    buf = torch.zeros(8, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    for dtype in (torch.int32, torch.float64, torch.uint8):
        with pytest.raises(RuntimeError, match="int64"):
            ops().bitmap_compact(torch.zeros(4, dtype=dtype, device=DEV),
                                 buf, cnt)
    x = _f(2, 3, 7, 5)
    for k, s, p in ((0, 1, 1), (3, 0, 1), (3, 1, -1), (-1, 1, 4),
                    (8, 1, 0),    # OH = 0, OW < 0
                    (6, 1, 0),    # OH = 2, OW = 0
                    (10, 2, 1)):  # k > H + 2p
        with pytest.raises(RuntimeError, match="conv"):
            ops().im2col_bf16(x, k, s, p)
        with pytest.raises(RuntimeError, match="conv"):
            ops().col2im(_f(4, 4), 2, 3, 7, 5, k, s, p)
    with pytest.raises(RuntimeError, match="dcol shape"):
        ops().col2im(_f(70, 26), 2, 3, 7, 5, 3, 1, 1)
