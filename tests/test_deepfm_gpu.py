"""DeepFM model-level GPU tests: the GPU score against the CPU model on a
ragged batch, the fused step against the composed one (the bindings that
predate the fused kernels), convergence, and an empty batch."""

import pytest
import torch

import kernel_oracles as ko
from lightctr_amd.data.synthetic import SyntheticCriteo
from lightctr_amd.models.deepfm import DeepFMHyper, DeepFMModel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def test_deepfm_ragged_batch_gpu_matches_cpu():
    """Rows of 0..45 entries at nf = 39 (shorter, equal, longer): the GPU
    score must be finite and match the CPU model on copied weights at the
    atol=0.08, rtol=0.05 of test_widedeep_ragged_batch_gpu_matches_cpu (the
    bf16 MLP forward), applied to the pre-sigmoid score."""
    F = ko.F_TABLE
    h = DeepFMHyper(num_features=F, num_fields=39, k=16, hidden=(64, 32),
                    init_sigma=0.1)
    cpu = DeepFMModel(h, device="cpu")
    g = torch.Generator().manual_seed(5)
    cpu.W.copy_(torch.randn(F, generator=g) * 0.1)
    row_ptr, fids, vals = ko.make_csr(list(range(46)), seed=6)
    s_cpu, _ = cpu._forward_cpu(row_ptr, fids, vals, train=False)
    for impl in ("fused", "composed"):
        gpu = DeepFMModel(h, device=DEV, forward_impl=impl)
        gpu.W.copy_(cpu.W)
        gpu.E.copy_(cpu.E)
        for lc, lg in zip(cpu.mlp.layers, gpu.mlp.layers):
            lg.W.copy_(lc.W)
            lg.b.copy_(lc.b)
            lg.Wbf.copy_(lg.W.to(torch.bfloat16))
            lg.Wtbf.copy_(lg.W.t().contiguous().to(torch.bfloat16))
        ko.poison((46, 39 * 16), torch.bfloat16, DEV)
        s_gpu, _ = gpu._forward_gpu(row_ptr.to(DEV), fids.to(DEV),
                                    vals.to(DEV), train=False)
        s_gpu = s_gpu.cpu()
        assert torch.isfinite(s_gpu).all(), (impl, s_gpu)
        assert torch.allclose(s_gpu, s_cpu, atol=0.08, rtol=0.05), \
            (impl, (s_gpu - s_cpu).abs().max())
        ko.poison((46, 39 * 16), torch.bfloat16, DEV)
        p = gpu.predict_proba(row_ptr.to(DEV), fids.to(DEV),
                              vals.to(DEV)).cpu()
        assert torch.isfinite(p).all()
        assert ((p > 0) & (p < 1)).all()


def _twin_batches(which, nf, F):
    g = torch.Generator().manual_seed(21)
    if which == "small":
        lengths = [nf, 0, 3, nf + 6, 1, nf]
    else:
        lengths = [nf] * 320
    out = []
    for step in range(3):
        row_ptr, fids, vals = ko.make_csr(lengths, F=F, seed=30 + step)
        labels = torch.randint(0, 2, (len(lengths),), generator=g).float()
        out.append((row_ptr.to(DEV), fids.to(DEV), vals.to(DEV),
                    labels.to(DEV)))
    return out


@pytest.mark.parametrize("which", ["small", "hot"])
@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
@pytest.mark.parametrize("K", [4, 16, 64])
def test_deepfm_fused_step_matches_composed(K, opt, which):
    """Twins on the same seed, three steps each: a 6-row ragged batch, and
    B = 320 x 39 over 64 fids (every fid hot). Losses and every sparse
    tensor agree to atol=1e-5, the tolerance test_fm_overlap_gpu.py uses
    where summation order may differ (here: the order of fm's reduction and
    (D + d b) x against d b x + D x).

    The first MLP layer starts at 1/32 of its He initialisation. The twins'
    E differ in the last fp32 bits after the first step, and the concat is
    bf16(E x): of the 320 x 39 x K elements a few land on the other side of
    a bf16 rounding boundary and move by a whole bf16 ulp, 2^-8 |E x| ~ 1e-4.
    Through He-scale weights (gain ~ 0.1 to the score) one such element
    shifts a row's loss by ~1e-5, the tolerance itself (measured: 1.2e-5 at
    K = 16 on the hot batch). At 1/32 the same event stays under 1e-6,
    while dDeep still reaches E's update well above the tolerance: ~3e-2 of
    the FM part of gv, hence ~3e-2 lr = 6e-5 of an Adagrad step. lr = 0.002
    keeps the pair term, which grows with the square of E's moves, of order
    one at K = 64, where an fp32 ulp of the score is ~1e-7."""
    F, nf = 64, 39
    h = DeepFMHyper(num_features=F, num_fields=nf, k=K, hidden=(32, 16),
                    optimizer=opt, lr=0.002)
    twins = {impl: DeepFMModel(h, device=DEV, forward_impl=impl)
             for impl in ("fused", "composed")}
    for m in twins.values():
        la = m.mlp.layers[0]
        la.W.mul_(1.0 / 32)
        la.Wbf.copy_(la.W.to(torch.bfloat16))
        la.Wtbf.copy_(la.W.t().contiguous().to(torch.bfloat16))
    for step, (rp, fi, v, lb) in enumerate(_twin_batches(which, nf, F)):
        losses = {impl: m.train_step(rp, fi, v, lb)
                  for impl, m in twins.items()}
        print(f"LOSSDIFF K{K} {opt} {which} step{step} "
              f"{float((losses['fused'] - losses['composed']).abs().max())}")
        assert torch.isfinite(losses["fused"]).all()
        assert torch.allclose(losses["fused"], losses["composed"],
                              atol=1e-5, rtol=0), \
            (losses["fused"] - losses["composed"]).abs().max()
    a, b = twins["fused"], twins["composed"]
    names = ["W", "E", "nW", "nE"] + (["zW", "zE"] if opt == "ftrl" else [])
    for n in names:
        ta, tb = getattr(a, n), getattr(b, n)
        print(f"STATEDIFF K{K} {opt} {which} {n} "
              f"{float((ta - tb).abs().max())}")
        assert torch.isfinite(ta).all(), n
        assert torch.allclose(ta, tb, atol=1e-5, rtol=0), \
            (n, (ta - tb).abs().max())
    assert float(a.nE.abs().max()) > 0  # the steps did move the table


def test_deepfm_gpu_convergence():
    gen = SyntheticCriteo(num_features=1 << 15, seed=43, device=DEV)
    h = DeepFMHyper(num_features=1 << 15, num_fields=39, k=16,
                    hidden=(256, 128))
    model = DeepFMModel(h, device=DEV)
    losses = []
    for _ in range(25):
        row_ptr, fields, fids, vals, labels = gen.batch(4096)
        loss = model.train_step(row_ptr, fids, vals, labels)
        losses.append(float(loss.mean()))
    assert losses[-1] < losses[0] * 0.99, losses[:3] + losses[-3:]


def test_deepfm_empty_batch_gpu():
    for impl in ("fused", "composed"):
        m = DeepFMModel(DeepFMHyper(num_features=64, num_fields=3, k=4,
                                    hidden=(8,)), device=DEV,
                        forward_impl=impl)
        rp = torch.zeros(1, dtype=torch.int32, device=DEV)
        fi = torch.zeros(0, dtype=torch.int32, device=DEV)
        v = torch.zeros(0, device=DEV)
        assert m.predict_proba(rp, fi, v).shape == (0,)
        assert m.train_step(rp, fi, v, torch.zeros(0, device=DEV)).shape \
            == (0,)
