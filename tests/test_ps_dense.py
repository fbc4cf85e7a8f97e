"""Dense-tensor PS tables (CPU): sharding helpers, DenseTable semantics,
exact equivalence of async-PS Wide&Deep with a one-process replay, async
smoke over updater x wire, and the custom-CDF / caller-table codecs."""

import os

import pytest
import torch
import torch.multiprocessing as mp

NF, K, HIDDEN = 4, 4, (8,)
DIMS = [NF * K, *HIDDEN, 1]


# ---------------------------------------------------------------- a. helpers
@pytest.mark.parametrize("total", [1, 7, 8, 9, 1000])
@pytest.mark.parametrize("ps_shards", [1, 2, 3])
def test_dense_range_covers_once(total, ps_shards):
    from lightctr_amd.parallel.ps_dense import dense_range

    covered = torch.zeros(total, dtype=torch.int32)
    prev_hi, seen_empty = 0, False
    for s in range(ps_shards):
        lo, hi = dense_range(total, ps_shards, s)
        assert 0 <= lo <= hi <= total
        assert lo == prev_hi  # contiguous, in shard order
        if hi > lo:
            assert not seen_empty  # only TRAILING shards may be empty
            assert lo % 8 == 0
        else:
            seen_empty = True
        covered[lo:hi] += 1
        prev_hi = hi
    assert prev_hi == total
    assert bool((covered == 1).all())


def test_dense_spec_flat_roundtrip_bit_exact():
    from lightctr_amd.models.mlp import MLP
    from lightctr_amd.parallel.ps_dense import (dense_offsets,
                                                mlp_dense_spec)

    a = MLP(DIMS, seed=1)
    b = MLP(DIMS, seed=2)
    spec = mlp_dense_spec(DIMS)
    offs, total = dense_offsets(spec)
    flat = a.flat_params()
    assert flat.numel() == total == 16 * 8 + 8 + 8 + 1
    # the spec's offsets address the layers' tensors inside the flat slab
    for i, la in enumerate(a.layers):
        for nm, p in ((f"layer{i}.W", la.W), (f"layer{i}.b", la.b)):
            off, shape = offs[nm]
            assert shape == tuple(p.shape)
            assert torch.equal(flat[off:off + p.numel()].view(shape), p)
    assert not torch.equal(b.flat_params(), flat)
    b.load_flat(flat)
    assert torch.equal(b.flat_params(), flat)
    for la, lb in zip(a.layers, b.layers):
        assert torch.equal(la.W, lb.W) and torch.equal(la.b, lb.b)


@pytest.mark.parametrize("delta", [-1, 1])
def test_load_flat_wrong_size_leaves_layers_untouched(delta):
    from lightctr_amd.models.mlp import MLP

    m = MLP(DIMS, seed=1)
    flat = m.flat_params()
    with pytest.raises(AssertionError):
        m.load_flat(torch.zeros(flat.numel() + delta))
    assert torch.equal(m.flat_params(), flat)


def test_flat_grads_order():
    from lightctr_amd.models.mlp import MLP

    m = MLP(DIMS, seed=4)
    x = torch.randn(5, DIMS[0], generator=torch.Generator().manual_seed(0))
    m.backward(torch.ones_like(m.forward(x)))
    g = m.flat_grads()
    off = 0
    for la in m.layers:
        for t in (la._dW, la._db):
            assert torch.equal(g[off:off + t.numel()], t.reshape(-1))
            off += t.numel()
    assert off == g.numel() == m.flat_params().numel()


# ------------------------------------------------- b. DenseTable semantics
def test_dense_table_dcasgd_shadows_are_per_worker():
    from lightctr_amd.parallel.ps_dense import DenseTable

    n, lr, lam = 37, 0.05, 0.1
    g = torch.Generator().manual_seed(2)
    s = torch.randn(n, generator=g)
    g0 = torch.randn(n, generator=g)
    g1 = torch.randn(n, generator=g)
    t = DenseTable(n, "dcasgd", lr=lr, dc_lambda=lam, n_workers=2, init=s)
    assert torch.equal(t.pack(0), s) and torch.equal(t.pack(1), s)
    t.apply(0, g0, "fp32")
    t.apply(1, g1, "fp32")
    # by hand: worker 0 sees no delay (shadow == slab); worker 1's shadow
    # is still the slab it pulled, one update behind
    w1 = s - lr * (g0 + lam * g0 * g0 * (s - s))
    w2 = w1 - lr * (g1 + lam * g1 * g1 * (w1 - s))
    assert torch.allclose(t.slab, w2, atol=1e-7, rtol=0)
    assert torch.allclose(t.shadow[0], w1, atol=1e-7, rtol=0)
    assert torch.allclose(t.shadow[1], w2, atol=1e-7, rtol=0)
    # a single shared shadow would have compensated against w1 (-> no term)
    assert not torch.allclose(t.slab, w1 - lr * g1, atol=1e-7, rtol=0)
    assert t.dropped == 0


@pytest.mark.parametrize("updater,expect", [
    ("sgd", lambda w, a, g: (w - 0.05 * g, None)),
    ("adagrad", lambda w, a, g: (
        w - 0.05 * g / (a + g * g + 1e-8).sqrt(), a + g * g)),
])
def test_dense_table_sgd_adagrad_formula(updater, expect):
    from lightctr_amd.parallel.ps_dense import DenseTable

    gen = torch.Generator().manual_seed(3)
    w = torch.randn(19, generator=gen)
    g = torch.randn(19, generator=gen) * 0.1
    t = DenseTable(19, updater, lr=0.05, eps=1e-8, init=w)
    a = None
    if t.acc is not None:
        t.acc.copy_(torch.rand(19, generator=gen) * 0.1)
        a = t.acc.clone()
    t.apply(0, g.to(torch.float16), "fp16")
    g16 = g.to(torch.float16).float()
    w_exp, a_exp = expect(w, a, g16)
    assert torch.allclose(t.slab, w_exp, atol=1e-7, rtol=0)
    if a_exp is not None:
        assert torch.allclose(t.acc, a_exp, atol=1e-7, rtol=0)


def test_dense_table_default_init_is_seeded():
    from lightctr_amd.parallel.ps_dense import DenseTable

    a = DenseTable(1000, "sgd", init_sigma=0.01, seed=7)
    b = DenseTable(1000, "sgd", init_sigma=0.01, seed=7)
    c = DenseTable(1000, "sgd", init_sigma=0.01, seed=8)
    assert torch.equal(a.slab, b.slab) and not torch.equal(a.slab, c.slab)
    assert 0.008 < float(a.slab.std()) < 0.012


@pytest.mark.parametrize("case", ["nan_fp32", "inf_fp16", "inf_int8_scale",
                                  "int8_product_overflow"])
def test_dense_table_drop_rule_cpu(case):
    from lightctr_amd.parallel.ps_dense import DenseTable

    n = 33
    gen = torch.Generator().manual_seed(5)
    t = DenseTable(n, "dcasgda", n_workers=2,
                   init=torch.randn(n, generator=gen))
    t.acc.copy_(torch.rand(n, generator=gen) * 0.1)
    t.shadow.copy_(torch.randn(2, n, generator=gen))
    before = (t.slab.clone(), t.acc.clone(), t.shadow.clone())
    g = torch.randn(n, generator=gen) * 0.01
    scale = None
    if case == "nan_fp32":
        g[n // 2] = float("nan")
        payload, wire = g, "fp32"
    elif case == "inf_fp16":
        payload, wire = g.to(torch.float16), "fp16"
        payload[3] = float("inf")
    elif case == "int8_product_overflow":
        # finite scale x finite table entry (|t| > 1) overflows to inf
        from lightctr_amd.utils.compress import QuantileCodec

        t._codec = QuantileCodec.from_table([-4.0, -1.0, 0.0, 1.0, 4.0])
        payload, wire = torch.full((n,), 4, dtype=torch.uint8), "int8"
        scale = torch.tensor([1e38])
    else:
        s = g.abs().max().reshape(1)
        payload, wire = t.codec.encode(g / s), "int8"
        scale = torch.tensor([float("inf")])
    t.apply(1, payload, wire, scale)
    assert t.dropped == 1
    assert torch.equal(t.slab, before[0])
    assert torch.equal(t.acc, before[1])
    assert torch.equal(t.shadow, before[2])
    # a following clean push still applies
    t.apply(1, torch.full((n,), 0.01), "fp32")
    assert t.dropped == 1
    assert not torch.equal(t.slab, before[0])


def test_dense_table_int8_mode_selects_codec():
    from lightctr_amd.parallel.ps_dense import DenseTable, dense_codec
    from lightctr_amd.utils.compress import QuantileCodec

    n = 64
    gen = torch.Generator().manual_seed(6)
    w = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.01
    scale = g.abs().max().reshape(1)
    for mode in ("log", "custom"):
        t = DenseTable(n, "sgd", lr=0.05, init=w, int8_mode=mode)
        codec = dense_codec(mode)
        assert torch.equal(t.codec.table, codec.table)
        codes = codec.encode(g / scale)
        t.apply(0, codes, "int8", scale)
        assert torch.equal(t.slab, w - 0.05 * (codec.table[codes.long()]
                                               * scale))
    assert torch.equal(
        dense_codec("custom").table,
        QuantileCodec(mode="custom", mu=0.0, sigma=0.25).table)
    assert not torch.equal(dense_codec("custom").table,
                           dense_codec("log").table)


# --------------------------------------- c. exact equivalence (2 PS + 1 w)
def _wd_cfg(updater, wire, ps_shards, F, lr=0.05):
    from lightctr_amd.models.wide_deep import WideDeepHyper
    from lightctr_amd.parallel.ps import PSConfig
    from lightctr_amd.parallel.ps_widedeep import widedeep_dense_spec

    hyper = WideDeepHyper(num_features=F, num_fields=NF, k=K, hidden=HIDDEN,
                          seed=9)
    cfg = PSConfig(num_features=F, k=K, ps_shards=ps_shards,
                   updater=updater, lr=lr, wire=wire, staleness=10,
                   dense_spec=widedeep_dense_spec(hyper))
    return cfg, hyper


def _dense_init():
    from lightctr_amd.models.mlp import MLP

    return MLP(DIMS, seed=5).flat_params()


def _equiv_proc(rank, port, q):
    try:
        import torch.distributed as dist

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=3)
        from lightctr_amd.parallel.ps import PSShard, setup_pair_groups
        from lightctr_amd.parallel.ps_widedeep import ps_train_widedeep
        from conftest import make_random_csr

        cfg, hyper = _wd_cfg("sgd", "fp32", 2, 200)
        groups = setup_pair_groups(cfg)
        if rank < 2:
            shard = PSShard(cfg, device="cpu", dense_init=_dense_init())

            def snap():
                return {"W": shard.W.tolist(), "V": shard.V.tolist(),
                        "D": shard.dense.slab.tolist(),
                        "range": (shard.dense_lo, shard.dense_hi)}

            before = snap()
            shard.serve(groups)
            q.put(("shard", rank, before, snap(), shard.dense.dropped))
        else:
            def gen(step):
                return make_random_csr(B=16, F_total=200, min_f=NF,
                                       max_f=NF, seed=step)

            losses = ps_train_widedeep(cfg, groups[rank], gen, steps=5,
                                       hyper=hyper, device="cpu")
            q.put(("losses", rank, losses))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put(("error", rank, traceback.format_exc()))
        raise


def _assemble(snaps, F):
    """shard snapshots {rank: dict} -> global (W [F], E [F,K], D [total])."""
    W = torch.zeros(F)
    E = torch.zeros(F, K)
    parts = []
    for s in sorted(snaps):
        ids = torch.arange(s, F, len(snaps))
        W[ids] = torch.tensor(snaps[s]["W"])[: ids.numel()]
        E[ids] = torch.tensor(snaps[s]["V"])[: ids.numel()]
        parts.append(torch.tensor(snaps[s]["D"]))
    return W, E, torch.cat(parts)


def test_ps_widedeep_matches_single_process_replay():
    from conftest import make_random_csr
    from lightctr_amd.models.mlp import MLP
    from lightctr_amd.parallel.ps_dense import dense_range
    from lightctr_amd.parallel.ps_widedeep import widedeep_grads

    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    mp.start_processes(_equiv_proc, args=(29711, q), nprocs=3, join=True,
                       start_method="spawn")
    before, after, losses = {}, {}, None
    while not q.empty():
        msg = q.get()
        assert msg[0] != "error", f"worker error: {msg}"
        if msg[0] == "shard":
            before[msg[1]], after[msg[1]] = msg[2], msg[3]
            assert msg[4] == 0  # nothing dropped
        else:
            losses = msg[2]
    assert sorted(before) == [0, 1] and losses is not None
    F, lr = 200, 0.05
    total = 16 * 8 + 8 + 8 + 1
    for s in (0, 1):
        assert tuple(before[s]["range"]) == dense_range(total, 2, s)
    W, E, D = _assemble(before, F)
    assert torch.equal(D, _dense_init())
    mlp = MLP(DIMS, seed=0)
    ref_losses = []
    for step in range(5):
        row_ptr, fids, vals, labels = make_random_csr(
            B=16, F_total=F, min_f=NF, max_f=NF, seed=step)
        uniq, inv = torch.unique(fids.long(), return_inverse=True)
        mlp.load_flat(D)
        loss, gW, gE = widedeep_grads(row_ptr, inv.to(torch.int32), vals,
                                      labels, W[uniq], E[uniq], mlp, NF)
        W[uniq] -= lr * gW
        E[uniq] -= lr * gE
        D = D - lr * mlp.flat_grads()
        ref_losses.append(float(loss.mean()))
    Wa, Ea, Da = _assemble(after, F)
    assert not torch.equal(Da, _dense_init())  # the dense slab trained
    assert torch.allclose(Wa, W, atol=1e-5)
    assert torch.allclose(Ea, E, atol=1e-5)
    assert torch.allclose(Da, D, atol=1e-5)
    assert torch.allclose(torch.tensor(losses), torch.tensor(ref_losses),
                          atol=1e-5)


# ------------------------------------------------ d. async smoke (1 PS + 2)
def _async_proc(rank, port, q, updater, wire):
    try:
        import torch.distributed as dist

        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=3)
        from lightctr_amd.parallel.ps import PSShard, setup_pair_groups
        from lightctr_amd.parallel.ps_widedeep import ps_train_widedeep
        from conftest import make_random_csr

        cfg, hyper = _wd_cfg(updater, wire, 1, 500, lr=0.1)
        groups = setup_pair_groups(cfg)
        if rank == 0:
            shard = PSShard(cfg, device="cpu", dense_init=_dense_init())
            init = shard.dense.slab.clone()
            shard.serve(groups)
            slab = shard.dense.slab
            q.put(("shard", bool(torch.isfinite(slab).all()),
                   bool(not torch.equal(slab, init)), shard.dense.dropped,
                   bool(torch.isfinite(shard.W).all()
                        and torch.isfinite(shard.V).all())))
        else:
            def gen(step):
                return make_random_csr(B=32, F_total=500, min_f=NF,
                                       max_f=NF, seed=step * 7 + rank,
                                       binary_vals=False)

            losses = ps_train_widedeep(cfg, groups[rank], gen, steps=8,
                                       hyper=hyper, device="cpu")
            q.put(("losses", all(l == l and abs(l) != float("inf")
                                 for l in losses), len(losses)))
        dist.destroy_process_group()
    except Exception:  # pragma: no cover
        import traceback

        q.put(("error", rank, traceback.format_exc()))
        raise


@pytest.mark.parametrize("i,updater,wire", [(0, "dcasgd", "fp32"),
                                            (1, "adagrad", "fp16"),
                                            (2, "dcasgda", "int8"),
                                            (3, "sgd", "fp32")])
def test_ps_widedeep_async_trains(i, updater, wire):
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    mp.start_processes(_async_proc, args=(29720 + i, q, updater, wire),
                       nprocs=3, join=True, start_method="spawn")
    msgs = []
    while not q.empty():
        msgs.append(q.get())
    assert all(m[0] != "error" for m in msgs), f"worker error: {msgs}"
    shard = [m for m in msgs if m[0] == "shard"]
    workers = [m for m in msgs if m[0] == "losses"]
    assert len(shard) == 1 and len(workers) == 2
    _, finite, moved, dropped, sparse_finite = shard[0]
    assert finite and moved and sparse_finite
    assert dropped == 0
    for _, ok, nsteps in workers:
        assert ok and nsteps == 8


def test_default_config_has_no_dense_table():
    from lightctr_amd.parallel.ps import PSConfig
    from lightctr_amd.parallel.ps_dense import dense_total

    cfg = PSConfig(num_features=10)
    assert cfg.dense_spec == () and cfg.dense_int8_mode == "log"
    assert dense_total(cfg.dense_spec) == 0


# ------------------------------------------------------------------ e. codec
def test_quantile_codec_custom_mode():
    from lightctr_amd.utils.compress import QuantileCodec

    for lo, hi, mu, sigma in ((-1.0, 1.0, 0.0, 0.25), (-0.5, 2.0, 0.3, 0.7)):
        c = QuantileCodec(levels=256, mode="custom", lo=lo, hi=hi, mu=mu,
                          sigma=sigma)
        t = c.table
        assert t.numel() == 256
        assert bool((t[1:] > t[:-1]).all())  # strictly increasing
        assert float(t[0]) >= lo and float(t[-1]) <= hi
        # equal CDF steps: levels are densest around mu
        gaps = t[1:] - t[:-1]
        assert abs(float(t[int(gaps.argmin())]) - mu) < sigma
        g = torch.Generator().manual_seed(3)
        x = (torch.randn(10000, generator=g) * sigma + mu).clamp(lo, hi)
        code = c.encode(x)
        assert code.dtype == torch.uint8
        y = c.decode(code)
        d_direct = (x - y).abs()
        dists = (x.unsqueeze(1) - t.unsqueeze(0)).abs().min(dim=1).values
        assert torch.allclose(d_direct, dists, atol=1e-6)


def test_quantile_codec_from_table():
    from lightctr_amd.utils.compress import QuantileCodec

    table = [-1.0, -0.125, 0.0, 0.25, 2.0]  # exact in fp32
    c = QuantileCodec.from_table(table)
    assert c.levels == 5 and c.table.tolist() == table
    # midpoints: -0.5625, -0.0625, 0.125, 1.125
    x = torch.tensor([-5.0, -0.5, -0.07, -0.04, 0.1, 0.2, 1.0, 1.2, 9.0])
    code = c.encode(x)
    assert code.tolist() == [0, 1, 1, 2, 2, 3, 3, 4, 4]
    assert c.decode(code).tolist() == [table[i] for i in code.tolist()]
    # every table entry round-trips to itself
    t = torch.tensor(table)
    assert torch.equal(c.decode(c.encode(t)), t)
    with pytest.raises(AssertionError):
        QuantileCodec.from_table([0.0, 0.0, 1.0])
