"""Wide&Deep and DeepFM with layout="field" on the GPU against the CPU path:
one train step and one predict_proba, both pooling modes, fused and composed
DeepFM; BatchPredictor over a field-layout model.

B = 9, nf = 5, K = 16, hidden (16, 8), multi-hot rows with missing fields.
Tolerances are those of test_deepfm_ragged_batch_gpu_matches_cpu for the
same comparison (the bf16 concat and bf16 MLP against the fp32 CPU model):
atol = 0.08, rtol = 0.05 on the pre-sigmoid score. The per-row loss and the
probability are functions of the score with slope at most 1 and 1/4, so the
same atol holds for them.
"""

import pytest
import torch

from lightctr_amd.data import LibffmDataset
from lightctr_amd.data.synthetic import SyntheticMultiHot
from lightctr_amd.models.deepfm import DeepFMHyper, DeepFMModel
from lightctr_amd.models.wide_deep import WideDeepHyper, WideDeepModel
from lightctr_amd.predict.predictor import BatchPredictor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F, NF, K = 512, 5, 16
ATOL, RTOL = 0.08, 0.05

CONFIGS = [("widedeep", None), ("deepfm", "fused"), ("deepfm", "composed")]


def make(name, impl, pooling, device):
    kw = dict(num_features=F, num_fields=NF, k=K, hidden=(16, 8),
              init_sigma=0.1, layout="field", pooling=pooling)
    if name == "widedeep":
        return WideDeepModel(WideDeepHyper(**kw), device=device)
    return DeepFMModel(DeepFMHyper(**kw), device=device, forward_impl=impl)


def batch(seed, rows=9):
    return SyntheticMultiHot(num_features=F, num_fields=NF, multi=(1, 3),
                             max_multi=4, p_missing=0.3,
                             seed=seed).batch(rows)


def twin(name, impl, pooling):
    cpu = make(name, impl, pooling, "cpu")
    g = torch.Generator().manual_seed(5)
    cpu.W.copy_(torch.randn(F, generator=g) * 0.1)
    gpu = make(name, impl, pooling, DEV)
    gpu.W.copy_(cpu.W)
    gpu.E.copy_(cpu.E)
    for lc, lg in zip(cpu.mlp.layers, gpu.mlp.layers):
        lg.W.copy_(lc.W)
        lg.b.copy_(lc.b)
        lg.Wbf.copy_(lg.W.to(torch.bfloat16))
        lg.Wtbf.copy_(lg.W.t().contiguous().to(torch.bfloat16))
    return cpu, gpu


@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("name,impl", CONFIGS)
def test_step_and_predict_match_cpu(name, impl, pooling):
    rp, fl, fi, v, lb = batch(17)
    lens = rp[1:] - rp[:-1]
    assert int(lens.max()) > NF and int(lens.min()) < NF  # multi-hot, missing
    cpu, gpu = twin(name, impl, pooling)
    d = [t.to(DEV) for t in (rp, fi, v, lb, fl)]
    s_cpu, _ = cpu._forward_cpu(rp, fi, v, train=False, fields=fl)
    s_gpu, _ = gpu._forward_gpu(d[0], d[1], d[2], train=False, fields=d[4])
    assert torch.isfinite(s_gpu).all()
    assert torch.allclose(s_gpu.cpu(), s_cpu, atol=ATOL, rtol=RTOL), \
        (s_gpu.cpu() - s_cpu).abs().max()
    l_cpu = cpu.train_step(rp, fi, v, lb, fields=fl)
    l_gpu = gpu.train_step(d[0], d[1], d[2], d[3], fields=d[4])
    assert torch.allclose(l_gpu.cpu(), l_cpu, atol=ATOL, rtol=RTOL), \
        (l_gpu.cpu() - l_cpu).abs().max()
    assert float(gpu.nE.abs().max()) > 0  # the step reached the table
    rp2, fl2, fi2, v2, _ = batch(18)
    p_cpu = cpu.predict_proba(rp2, fi2, v2, fields=fl2)
    p_gpu = gpu.predict_proba(rp2.to(DEV), fi2.to(DEV), v2.to(DEV),
                              fields=fl2.to(DEV)).cpu()
    assert torch.isfinite(p_gpu).all()
    assert torch.allclose(p_gpu, p_cpu, atol=ATOL, rtol=RTOL), \
        (p_gpu - p_cpu).abs().max()


def test_fields_none_raises_on_gpu():
    rp, fl, fi, v, lb = (t.to(DEV) for t in batch(3))
    for name, impl in CONFIGS:
        m = make(name, impl, "sum", DEV)
        with pytest.raises(ValueError, match="fields"):
            m.predict_proba(rp, fi, v)
        with pytest.raises(ValueError, match="fields"):
            m.train_step(rp, fi, v, lb)


def test_models_refuse_what_the_lds_cannot_hold():
    """an (nf, K) pair past the per-block LDS is refused at construction"""
    from lightctr_amd.ops import hip_ops

    nf = hip_ops.ffm_max_lds_per_block() // (16 * (64 + 1)) + 1
    for H, M in ((WideDeepHyper, WideDeepModel), (DeepFMHyper, DeepFMModel)):
        with pytest.raises(ValueError, match="LDS"):
            M(H(num_features=64, num_fields=nf, k=64, hidden=(8,),
                layout="field"), device=DEV)
        M(H(num_features=64, num_fields=nf, k=64, hidden=(8,)), device=DEV)


@pytest.mark.parametrize("name,impl", CONFIGS)
def test_batch_predictor_passes_fields(name, impl):
    rp, fl, fi, v, lb = batch(23, rows=37)
    m = make(name, impl, "mean", DEV)
    ds = LibffmDataset(rp, fl, fi, v, lb).to(torch.device(DEV))
    whole = m.predict_proba(ds.row_ptr, ds.fids, ds.vals, fields=ds.fields)
    got = BatchPredictor(m, batch_size=8).predict_csr(ds)
    assert torch.equal(got.cpu(), whole.cpu())
