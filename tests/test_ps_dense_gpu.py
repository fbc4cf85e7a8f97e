"""Dense-tensor PS tables on the GPU: ps_dense_check / ps_dense_apply /
ps_dense_pack against the CPU DenseTable, the device drop rule, and a
one-process Wide&Deep loopback through a DenseTable."""

import pytest
import torch

DEV = "cuda:0"
LR, LAM, EPS = 0.05, 0.1, 1e-8
UPDATERS = ["sgd", "adagrad", "dcasgd", "dcasgda"]
WIRES = ["fp32", "fp16", "int8"]
# empty vector body / tail only / block edges / many blocks in one trip
SIZES = [1, 3, 4, 5, 255, 256, 257, 1027, (1 << 20) + 3]
# One trip of the capped grid is 2048 blocks x 256 lanes: 2,097,152
# elements in the 4-per-lane body, 524,288 in the 1-per-lane body that a
# misaligned base selects. These sizes clamp the grid and take a partial
# second trip of the grid-stride loop, plus a tail in the vector body.
MULTI_PASS_VEC = (1 << 21) + (1 << 19) + 5
MULTI_PASS_SCALAR = (1 << 19) + (1 << 17) + 3
# (n, slab view offset in elements)
APPLY_CASES = [(n, 0) for n in SIZES] + [
    (1027, 1), (MULTI_PASS_VEC, 0), (MULTI_PASS_SCALAR, 1)]


def _state(n, seed):
    """Input magnitudes of test_ps_apply_kernel_parity: params ~N(0,1),
    grads ~1e-2, accumulators in [0, 0.1]."""
    g = torch.Generator().manual_seed(seed)
    return {"slab": torch.randn(n, generator=g),
            "acc": torch.rand(n, generator=g) * 0.1,
            "shadow": torch.randn(2, n, generator=g) * 0.1,
            "grad": torch.randn(n, generator=g) * 0.01}


def _table(st, updater, device, view_offset=0):
    from lightctr_amd.parallel.ps_dense import DenseTable

    n = st["slab"].numel()
    t = DenseTable(n, updater, lr=LR, dc_lambda=LAM, eps=EPS, n_workers=2,
                   device=device, init=st["slab"])
    if view_offset:
        # slab as a view that is only element-aligned
        big = torch.zeros(n + view_offset, device=device)
        big[view_offset:] = st["slab"].to(device)
        t.slab = big[view_offset:]
    if t.acc is not None:
        t.acc.copy_(st["acc"])
    if t.shadow is not None:
        t.shadow.copy_(st["shadow"])
    return t


def _payload(st, wire, codec):
    g = st["grad"]
    if wire == "fp32":
        return g.clone(), None
    if wire == "fp16":
        return g.to(torch.float16), None
    scale = g.abs().max().reshape(1)
    return codec.encode(g / scale), scale


def _assert_parity(gpu, cpu, tag):
    assert torch.allclose(gpu.slab.cpu(), cpu.slab, atol=1e-5, rtol=1e-5), tag
    if cpu.acc is not None:
        assert torch.allclose(gpu.acc.cpu(), cpu.acc, atol=1e-6), tag
    if cpu.shadow is not None:
        assert torch.allclose(gpu.shadow.cpu(), cpu.shadow, atol=1e-5,
                              rtol=1e-5), tag


# ------------------------------------------------------------ f. apply parity
@pytest.mark.gpu
@pytest.mark.parametrize("wire", WIRES)
@pytest.mark.parametrize("updater", UPDATERS)
def test_ps_dense_apply_parity(updater, wire):
    for n, off in APPLY_CASES:
        st = _state(n, seed=n)
        cpu = _table(st, updater, "cpu")
        gpu = _table(st, updater, DEV, view_offset=off)
        assert gpu.slab.data_ptr() % 16 == (4 * off) % 16
        payload, scale = _payload(st, wire, cpu.codec)
        cpu.apply(1, payload, wire, scale)
        gpu.apply(1, payload.to(DEV), wire,
                  None if scale is None else scale.to(DEV))
        tag = f"{updater} {wire} n={n} off={off}"
        _assert_parity(gpu, cpu, tag)
        assert not torch.equal(cpu.slab, st["slab"]), tag
        if cpu.shadow is not None:  # other worker's shadow untouched
            assert torch.equal(gpu.shadow[0].cpu(), st["shadow"][0]), tag
        assert gpu.dropped == 0 and cpu.dropped == 0, tag


# -------------------------------------------------------------- g. drop rule
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["fp32_nan_first", "fp32_inf_last",
                                  "fp16_inf_first", "fp16_nan_last",
                                  "int8_inf_scale", "int8_nan_scale"])
def test_ps_dense_drop_rule_gpu(case):
    from lightctr_amd.parallel.ps_dense import dense_codec

    n = 1027
    st = _state(n, seed=11)
    t = _table(st, "dcasgda", DEV)
    before = (t.slab.clone(), t.acc.clone(), t.shadow.clone())
    wire, kind, where = case.split("_")
    bad = float("nan") if kind == "nan" else float("inf")
    payload, scale = _payload(st, wire, dense_codec("log"))
    payload = payload.to(DEV)
    if wire == "int8":
        scale = torch.tensor([bad], device=DEV)
    else:
        payload[0 if where == "first" else n - 1] = bad
    t.apply(1, payload, wire, scale)
    assert t.dropped == 1
    assert torch.equal(t.slab, before[0])
    assert torch.equal(t.acc, before[1])
    assert torch.equal(t.shadow, before[2])
    # a following clean push still applies, and matches the CPU table
    cpu = _table(st, "dcasgda", "cpu")
    clean, _ = _payload(st, "fp32", None)
    cpu.apply(1, clean, "fp32")
    t.apply(1, clean.to(DEV), "fp32")
    assert t.dropped == 1
    assert not torch.equal(t.slab, before[0])
    _assert_parity(t, cpu, case)


@pytest.mark.gpu
@pytest.mark.parametrize("wire", ["fp32", "fp16"])
@pytest.mark.parametrize("n,pay_off,bad_at", [
    (MULTI_PASS_VEC, 0, MULTI_PASS_VEC - 6),       # vector body, 2nd trip
    (MULTI_PASS_SCALAR, 1, MULTI_PASS_SCALAR - 1),  # scalar body, 2nd trip
])
def test_ps_dense_drop_rule_second_trip(wire, n, pay_off, bad_at):
    """The one non-finite value sits where only a second trip of the
    check kernel's grid-stride loop reaches it; pay_off=1 makes the payload
    base element-aligned only, which selects the 1-per-lane bodies."""
    st = _state(n, seed=13)
    t = _table(st, "dcasgda", DEV)
    before = (t.slab.clone(), t.acc.clone(), t.shadow.clone())
    clean, _ = _payload(st, wire, None)
    buf = torch.zeros(n + pay_off, dtype=clean.dtype, device=DEV)
    payload = buf[pay_off:]
    assert payload.data_ptr() % 16 == (pay_off * clean.element_size()) % 16
    payload.copy_(clean)
    payload[bad_at] = float("inf")
    t.apply(1, payload, wire)
    assert t.dropped == 1
    assert torch.equal(t.slab, before[0])
    assert torch.equal(t.acc, before[1])
    assert torch.equal(t.shadow, before[2])
    payload.copy_(clean)
    cpu = _table(st, "dcasgda", "cpu")
    cpu.apply(1, clean, wire)
    t.apply(1, payload, wire)
    assert t.dropped == 1
    _assert_parity(t, cpu, f"{wire} n={n} pay_off={pay_off}")


@pytest.mark.gpu
def test_ps_dense_drop_rule_int8_product_overflow():
    """A finite scale times a finite table entry can overflow: the push is
    judged on table * scale, on both the CPU and the GPU path."""
    from lightctr_amd.utils.compress import QuantileCodec

    n = 1027
    st = _state(n, seed=17)
    codes = torch.randint(1, 4, (n,), dtype=torch.uint8,
                          generator=torch.Generator().manual_seed(1))
    for dev in ("cpu", DEV):
        t = _table(st, "dcasgda", dev)
        t._codec = QuantileCodec.from_table([-4.0, -1.0, 0.0, 1.0, 4.0],
                                            device=dev)
        before = (t.slab.clone(), t.acc.clone(), t.shadow.clone())
        t.apply(1, codes.to(dev), "int8",
                torch.tensor([1e38], device=dev))  # 4 * 1e38 = inf
        assert t.dropped == 1, dev
        assert torch.equal(t.slab, before[0]), dev
        assert torch.equal(t.acc, before[1]), dev
        assert torch.equal(t.shadow, before[2]), dev
        t.apply(1, codes.to(dev), "int8", torch.tensor([1e-2], device=dev))
        assert t.dropped == 1, dev
        assert not torch.equal(t.slab, before[0]), dev


# -------------------------------------------------------------------- h. pack
@pytest.mark.gpu
@pytest.mark.parametrize("wire", ["fp32", "fp16"])
def test_ps_dense_pack(wire):
    from lightctr_amd.parallel.ps_dense import DenseTable

    # (n, slab view offset): the issue's sizes, then a clamped grid with a
    # partial second trip in the 4-per-lane and in the 1-per-lane body
    for n, off in ((1, 0), (5, 0), (257, 0), (1027, 0), (1027, 1),
                   (MULTI_PASS_VEC, 0), (MULTI_PASS_SCALAR, 1)):
        g = torch.Generator().manual_seed(n)
        slab = torch.randn(n, generator=g)
        slab[0] = 1e-6  # fp16-subnormal range
        t = DenseTable(n, "dcasgd", n_workers=3, device=DEV, init=slab)
        if off:
            big = torch.zeros(n + off, device=DEV)
            big[off:] = slab.to(DEV)
            t.slab = big[off:]
        assert t.slab.data_ptr() % 16 == (4 * off) % 16
        sh0 = torch.randn(3, n, generator=g)
        t.shadow.copy_(sh0)
        out = t.pack(1, wire)
        if wire == "fp16":
            assert out.dtype == torch.float16
            assert torch.equal(out.cpu(), slab.to(torch.float16))
        else:
            assert out.dtype == torch.float32
            assert torch.equal(out.cpu(), slab)
            assert out.data_ptr() != t.slab.data_ptr()  # a copy
        assert torch.equal(t.slab.cpu(), slab)
        assert torch.equal(t.shadow[1].cpu(), slab)
        assert torch.equal(t.shadow[0].cpu(), sh0[0])
        assert torch.equal(t.shadow[2].cpu(), sh0[2])
    # no shadows without delay compensation; int8 wire pulls go as fp32
    t = DenseTable(257, "sgd", device=DEV, init=torch.arange(257.0))
    out = t.pack(0, "int8")
    assert out.dtype == torch.float32
    assert torch.equal(out.cpu(), torch.arange(257.0))


# ---------------------------------------------------- i. one-process loopback
@pytest.mark.gpu
def test_ps_dense_widedeep_loopback_gpu():
    from conftest import make_random_csr
    from lightctr_amd.models.mlp import MLP
    from lightctr_amd.parallel.ps_dense import DenseTable
    from lightctr_amd.parallel.ps_widedeep import widedeep_grads

    F, NF, K, lr = 200, 4, 4, 0.1
    dims = [NF * K, 8, 1]
    row_ptr, fids, vals, labels = make_random_csr(
        B=16, F_total=F, min_f=NF, max_f=NF, seed=0, device=DEV)
    g = torch.Generator().manual_seed(1)
    W = torch.zeros(F, device=DEV)
    E = (torch.randn(F, K, generator=g) * 0.01).to(DEV)
    mlp = MLP(dims, seed=3, device=DEV)
    table = DenseTable(mlp.flat_params().numel(), "sgd", lr=lr, device=DEV,
                       init=MLP(dims, seed=5).flat_params())
    uniq, inv = torch.unique(fids.long(), return_inverse=True)
    fids_local = inv.to(torch.int32)
    losses = []
    for _ in range(20):
        mlp.load_flat(table.pack(0, "fp32"))
        loss, gW, gE = widedeep_grads(row_ptr, fids_local, vals, labels,
                                      W[uniq], E[uniq], mlp, NF)
        W[uniq] -= lr * gW
        E[uniq] -= lr * gE
        table.apply(0, mlp.flat_grads(), "fp32")
        losses.append(float(loss.mean()))
    assert table.dropped == 0
    assert all(l == l and abs(l) != float("inf") for l in losses)
    for t in (W, E, table.slab):
        assert bool(torch.isfinite(t).all())
    assert losses[-1] < losses[0], losses


@pytest.mark.gpu
def test_widedeep_grads_gpu_matches_cpu():
    """GPU branch of widedeep_grads vs the CPU branch on the same pulled
    parameters. Embeddings, MLP weights and batch values are chosen
    bf16-representable, so the first layer's pre-activations agree to fp32
    summation order (no ReLU flips) and the GPU's only extra error is the
    bf16 rounding of intermediate operands (layer-0 output, dZ of layer 1,
    dZ of layer 0), each <= 2^-9 relative, plus the forward perturbation
    of dpred: at most 4 roundings in any product chain, 4 * 2^-9 = 0.8% of
    the summed |terms|. Allowing the summed |terms| of an element to be 3x
    the tensor's largest |value| gives the bound used: 2.5% of max|cpu|."""
    from conftest import make_random_csr
    from lightctr_amd.models.mlp import MLP
    from lightctr_amd.parallel.ps_widedeep import widedeep_grads

    F, NF, K = 200, 4, 4
    dims = [NF * K, 8, 1]
    row_ptr, fids, vals, labels = make_random_csr(
        B=16, F_total=F, min_f=NF, max_f=NF, seed=2)
    g = torch.Generator().manual_seed(3)
    W = torch.randn(F, generator=g) * 0.1
    E = (torch.randn(F, K, generator=g) * 0.5).to(torch.bfloat16).float()
    flat = MLP(dims, seed=5).flat_params().to(torch.bfloat16).float()
    uniq, inv = torch.unique(fids.long(), return_inverse=True)
    fl = inv.to(torch.int32)
    res = {}
    for dev in ("cpu", DEV):
        mlp = MLP(dims, seed=0, device=dev)
        mlp.load_flat(flat.to(dev))
        loss, gW, gE = widedeep_grads(
            row_ptr.to(dev), fl.to(dev), vals.to(dev), labels.to(dev),
            W[uniq].to(dev), E[uniq].to(dev), mlp, NF)
        res[dev] = [loss.cpu(), gW.cpu(), gE.cpu()] + [
            t.cpu() for la in mlp.layers for t in (la._dW, la._db)]
    names = ["loss", "gWl", "gEl", "dW0", "db0", "dW1", "db1"]
    for nm, c, d in zip(names, res["cpu"], res[DEV]):
        assert c.shape == d.shape, nm
        err = float((c - d).abs().max())
        bound = 2.5e-2 * float(c.abs().max())
        print(f"{nm}: max|cpu|={float(c.abs().max()):.3e} err={err:.3e} "
              f"bound={bound:.3e}")
        assert float(c.abs().max()) > 0, nm
        assert err <= bound, (nm, err, bound)
