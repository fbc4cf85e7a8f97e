"""fwfm_forward / fwfm_backward_emit (ops/csrc/fwfm_kernels.hip) against
the float64 entry-pair reference of test_fwfm.py.

Exact set: V in {-1, 0, 1}, x in {1, 2}, W and R in {-1, 0, 1, 2}, d in
{-2..2}; the sum of the absolute values of the terms of every output is
asserted to stay below 2^24, so every quantity is exact in fp32 in any
summation order and the comparison is bit equality. Float set: randn inputs
under the derived bound (additions + 2) * 2^-23 * sum |terms| per element.
"""

import pytest
import torch

import kernel_oracles as ko
from test_fwfm import csr, pair_ref, random_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = 256
KS = (4, 8, 16, 32, 64)


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def exact_batch(rows, nf, K, seed):
    """rows: one (length, kind) per row. kind: "rand" draws fields from
    [0, nf), "perm" gives every entry another field while they last, "one"
    puts all in field nf - 1, "absent" leaves field 0 out, "dup" repeats a
    fid, "bad" gives one entry field nf and one field -1."""
    g = torch.Generator().manual_seed(seed)
    fields, fids = [], []
    for n, kind in rows:
        a = torch.randint(0, nf, (n,), generator=g)
        f = torch.randint(0, F, (n,), generator=g)
        if kind == "perm":
            a = torch.cat([torch.randperm(nf, generator=g), a])[:n]
        elif kind == "one":
            a[:] = nf - 1
        elif kind == "absent":
            a = torch.where(a == 0, torch.tensor(nf - 1 if nf > 1 else -1), a)
        elif kind == "dup":
            f[n // 2] = f[0]
        elif kind == "bad":
            a[1], a[n - 2] = nf, -1
        fields.append(a), fids.append(f)
    row_ptr = torch.tensor([0] + [n for n, _ in rows]).cumsum(0).int()
    nnz, B = int(row_ptr[-1]), len(rows)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    R = ri(-1, 2, nf, nf)
    R = R.triu() + 7.0 * torch.ones(nf, nf).tril(-1)   # must not matter
    return {"row_ptr": row_ptr,
            "fields": torch.cat(fields + [torch.zeros(0).long()]).int(),
            "fids": torch.cat(fids + [torch.zeros(0).long()]).int(),
            "vals": ri(1, 2, nnz), "W": ri(-1, 2, F), "V": ri(-1, 1, F, K),
            "R": R, "dpred": ri(-2, 2, B)}


def batches(nf, K):
    G = 64 // K
    sp = 4 * G + 3
    return [
        [(0, "rand"), (0, "rand"), (1, "rand"), (G - 1, "rand"), (G, "rand"),
         (G + 1, "rand"), (4 * G, "rand"), (4 * G + 1, "rand"), (0, "rand")],
        [(39, "perm"), (sp, "one"), (sp, "absent"), (sp, "dup"), (sp, "bad")],
        [(G + 1, "perm"), (0, "rand"), (4 * G + 1, "rand")],
        [(1, "rand"), (G, "perm"), (39, "rand"), (4 * G, "perm")],
        [(130, "rand")],          # alone: keeps the dR sums below 2^24
        [],
    ]


def run(c):
    """(pred, gw, gv, dR) of the kernels, every output over poisoned memory"""
    g = {k: v.to(DEV) for k, v in c.items()}
    B, nnz, K, nf = c["dpred"].numel(), c["fids"].numel(), c["V"].shape[1], \
        c["R"].shape[0]
    ko.poison((B,), torch.float32, DEV)
    pred = ops().fwfm_forward(*csr(g), g["W"], g["V"], g["R"])
    for shape in ((nnz,), (nnz, K), (nf, nf)):
        ko.poison(shape, torch.float32, DEV)
    gw, gv, dR = ops().fwfm_backward_emit(*csr(g), g["V"], g["R"],
                                          g["dpred"])
    return g, {"pred": pred, "gw": gw, "gv": gv, "dR": dR}


@pytest.mark.parametrize("nf", (1, 2, 5, 39))
@pytest.mark.parametrize("K", KS)
def test_exact(K, nf):
    for i, rows in enumerate(batches(nf, K)):
        c = exact_batch(rows, nf, K, seed=100 * K + 10 * nf + i)
        ref = pair_ref(*csr(c), c["W"], c["V"], c["R"], c["dpred"])
        g, out = run(c)
        for name, o in out.items():
            assert not (ref[name][1] >= 2 ** 24).any(), (name, i)
            ko.check_bits(f"{name}[{i}]", o, ref[name][0].float())
        assert not out["dR"].tril(-1).any()
        # R == 1 is FM, against the kernel that already exists
        ok = ((c["fields"] >= 0) & (c["fields"] < nf)).all()
        if ok and rows:  # an entry outside [0, nf) is in FM's pairs only
            fm, _ = ops().fm_forward(g["row_ptr"], g["fids"], g["vals"],
                                     g["W"], g["V"])
            one = ops().fwfm_forward(*csr(g), g["W"], g["V"],
                                     torch.ones_like(g["R"]))
            ko.check_bits(f"fm[{i}]", one, fm.cpu())


@pytest.mark.parametrize("K", KS)
def test_float_bound_and_determinism(K):
    nf = 39
    c = random_batch(9, nf, K, F=F, seed=K, lo=39, hi=60)
    ref = pair_ref(*csr(c), c["W"], c["V"], c["R"], c["dpred"])
    _, out = run(c)
    for name, o in out.items():
        val, mag, cnt = ref[name]
        ko.check_bound(name, o, val, (cnt.clamp(min=1) + 1) * ko.U23 * mag)
    # several blocks' partials: two runs agree bit for bit
    c = random_batch(257, nf, K, F=F, seed=K + 1, lo=0, hi=50)
    g = {k: v.to(DEV) for k, v in c.items()}
    dRs = [ops().fwfm_backward_emit(*csr(g), g["V"], g["R"], g["dpred"])[2]
           for _ in range(2)]
    ko.check_bits("dR twice", dRs[0], dRs[1].cpu())
    assert dRs[0].triu().any()


BAD = {"R shape": dict(R=torch.ones(5, 6)),
       "R dtype": dict(R=torch.ones(5, 5, dtype=torch.float64)),
       "fields length": dict(fields=torch.zeros(3, dtype=torch.int32)),
       "fields dtype": dict(fields=None)}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(what):
    c = random_batch(4, 5, 8, F=F)
    c.update(BAD[what])
    if c["fields"] is None:
        c["fields"] = random_batch(4, 5, 8, F=F)["fields"].long()
    g = {k: v.to(DEV) for k, v in c.items()}
    with pytest.raises(RuntimeError):
        ops().fwfm_forward(*csr(g), g["W"], g["V"], g["R"])
    with pytest.raises(RuntimeError):
        ops().fwfm_backward_emit(*csr(g), g["V"], g["R"], g["dpred"])


def test_lds_limit_names_the_bytes():
    o = ops()
    assert o.fwfm_lds_bytes(39, 64) <= o.ffm_max_lds_per_block()
    assert o.fwfm_lds_bytes(64, 16) <= o.ffm_max_lds_per_block()
    c = random_batch(2, 64, 64, F=F)
    g = {k: v.to(DEV) for k, v in c.items()}
    msg = f"needs {o.fwfm_lds_bytes(64, 64)} bytes of LDS per block, the " \
          f"device gives {o.ffm_max_lds_per_block()}"
    with pytest.raises(RuntimeError, match=msg):
        o.fwfm_forward(*csr(g), g["W"], g["V"], g["R"])
    with pytest.raises(RuntimeError, match=msg):
        o.fwfm_backward_emit(*csr(g), g["V"], g["R"], g["dpred"])


@pytest.mark.parametrize("optimizer", ("adagrad", "ftrl"))
@pytest.mark.parametrize("K", (4, 16, 64))
def test_model_twins(K, optimizer):
    from lightctr_amd.models.fwfm import FwFMHyper, FwFMModel

    # Default hyper, as the FM twins of test_fm_overlap_gpu.py whose atol
    # this is. Adagrad's first step lr g / sqrt(g^2 + eps) turns a gradient
    # difference e into up to e lr / sqrt(eps) = 1000 e, so 1e-5 asks for
    # gradients equal to 1e-8 absolute; at init_sigma = 0.01 their rounding
    # (about 40 u |d x| sum |terms|, terms of 1e-2) is near 1e-9.
    nf, B = 39, 6
    h = FwFMHyper(num_features=F, num_fields=nf, k=K, optimizer=optimizer,
                  seed=K)
    cpu, gpu = FwFMModel(h, device="cpu"), FwFMModel(h, device=DEV)
    for step in range(3):
        c = random_batch(B, nf, K, F=F, seed=step, lo=39, hi=39)
        c["fields"] = torch.arange(nf, dtype=torch.int32).repeat(B)
        g = {k: v.to(DEV) for k, v in c.items()}
        lc = cpu.train_step(*csr(c), c["labels"])
        lg = gpu.train_step(*csr(g), g["labels"])
        torch.testing.assert_close(lg.cpu(), lc, rtol=0, atol=1e-5)
        for name in ("W", "V", "R"):
            torch.testing.assert_close(getattr(gpu, name).cpu(),
                                       getattr(cpu, name), rtol=0, atol=1e-5,
                                       msg=lambda m: f"{name} step {step} {m}")
