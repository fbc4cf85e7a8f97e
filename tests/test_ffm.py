"""FFM: CPU reference math checks + convergence; GPU parity in test_ffm_gpu."""

import pytest
import torch

from lightctr_amd.data import LibffmDataset
from lightctr_amd.data.synthetic import SyntheticCriteo
from lightctr_amd.models.ffm import FFMHyper, FFMModel, FFMTrainer
from lightctr_amd.ops import ffm_ref, fm_ref

from conftest import make_random_csr


def _fieldify(fids, nfields, seed=0):
    """Assign each feature a stable field (fid % nfields)."""
    return (fids.long() % nfields).int()


def test_ffm_forward_matches_bruteforce():
    row_ptr, fids, vals, _ = make_random_csr(B=8, F_total=200, min_f=2,
                                             max_f=10, seed=3,
                                             binary_vals=False)
    nf, K = 5, 4
    fields = _fieldify(fids, nf)
    g = torch.Generator().manual_seed(0)
    W = torch.randn(200, generator=g)
    V = torch.randn(200, nf, K, generator=g) * 0.1
    pred = ffm_ref.ffm_forward_ref(row_ptr, fields, fids, vals, W, V)
    for r in range(8):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        f = fids[lo:hi].long()
        fl = fields[lo:hi].long()
        x = vals[lo:hi]
        expect = float((W[f] * x).sum())
        for a in range(len(f)):
            for b in range(a + 1, len(f)):
                expect += float(V[f[a], fl[b]] @ V[f[b], fl[a]] * x[a] * x[b])
        assert abs(float(pred[r]) - expect) < 1e-4


def test_ffm_backward_matches_autograd():
    row_ptr, fids, vals, labels = make_random_csr(B=16, F_total=100, min_f=2,
                                                  max_f=8, seed=5,
                                                  binary_vals=False)
    nf, K = 4, 4
    fields = _fieldify(fids, nf)
    g = torch.Generator().manual_seed(1)
    W = torch.randn(100, generator=g).requires_grad_(True)
    V = (torch.randn(100, nf, K, generator=g) * 0.1).requires_grad_(True)
    pred = ffm_ref.ffm_forward_ref(row_ptr, fields, fids, vals, W, V)
    loss, _ = fm_ref.logloss_grad_ref(pred, labels, 1.0)
    (loss.sum() / 16).backward()
    with torch.no_grad():
        pred2 = ffm_ref.ffm_forward_ref(row_ptr, fields, fids, vals,
                                        W.detach(), V.detach())
        _, dpred = fm_ref.logloss_grad_ref(pred2, labels, 1.0 / 16)
        gW, gV = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                          V.detach(), dpred)
    assert torch.allclose(gW, W.grad, atol=1e-5)
    assert torch.allclose(gV, V.grad, atol=1e-5)


def test_ffm_cpu_convergence():
    gen = SyntheticCriteo(num_features=1 << 12, seed=13)
    row_ptr, fields, fids, vals, labels = gen.batch(512)
    ds = LibffmDataset(row_ptr, fields, fids, vals, labels)
    h = FFMHyper(num_features=1 << 12, num_fields=39, k=4, lr=0.05)
    tr = FFMTrainer(ds, h, device="cpu", batch_size=128, epochs=2)
    m0 = tr.evaluate()
    tr.train(log=None)
    m1 = tr.evaluate()
    assert m1["logloss"] < m0["logloss"]


@pytest.mark.gpu
class TestFFMGpu:
    def test_forward_parity(self):
        from lightctr_amd.ops import hip_ops

        row_ptr, fids, vals, _ = make_random_csr(B=64, F_total=5000, min_f=2,
                                                 max_f=30, seed=7,
                                                 device="cuda:0",
                                                 binary_vals=False)
        nf, K = 7, 8
        fields = (fids.long() % nf).int()
        g = torch.Generator().manual_seed(2)
        W = torch.randn(5000, generator=g).cuda()
        V = (torch.randn(5000, nf, K, generator=g) * 0.1).cuda()
        pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, V)
        pred_ref = ffm_ref.ffm_forward_ref(row_ptr, fields, fids, vals, W, V)
        assert torch.allclose(pred, pred_ref, atol=1e-3, rtol=1e-4)

    def test_backward_parity(self):
        from lightctr_amd.ops import hip_ops

        row_ptr, fids, vals, labels = make_random_csr(B=64, F_total=5000,
                                                      min_f=2, max_f=30,
                                                      seed=8, device="cuda:0",
                                                      binary_vals=False)
        nf, K = 7, 8
        fields = (fids.long() % nf).int()
        g = torch.Generator().manual_seed(3)
        W = torch.randn(5000, generator=g).cuda()
        V = (torch.randn(5000, nf, K, generator=g) * 0.1).cuda()
        pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, V)
        _, dpred = hip_ops.logloss_grad(pred, labels, 1.0 / 64)
        gradW = torch.zeros(5000).cuda()
        gradV = torch.zeros(5000, nf, K).cuda()
        touched = torch.zeros((5000 + 63) // 64, dtype=torch.int64).cuda()
        hip_ops.ffm_backward(row_ptr, fields, fids, vals, V, dpred, gradW,
                             gradV, touched)
        gW_ref, gV_ref = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                                  V, dpred)
        assert torch.allclose(gradW, gW_ref, atol=1e-5, rtol=1e-4)
        assert torch.allclose(gradV, gV_ref, atol=1e-5, rtol=1e-4)

    def test_train_convergence(self):
        from lightctr_amd.data.synthetic import SyntheticCriteo

        gen = SyntheticCriteo(num_features=1 << 14, seed=23, device="cuda:0")
        h = FFMHyper(num_features=1 << 14, num_fields=39, k=8)
        model = FFMModel(h, device="cuda:0")
        losses = []
        for _ in range(20):
            row_ptr, fields, fids, vals, labels = gen.batch(2048)
            loss = model.train_step(row_ptr, fields, fids, vals, labels)
            losses.append(float(loss.mean()))
        assert losses[-1] < losses[0] * 0.99, losses[:3] + losses[-3:]


@pytest.mark.gpu
def test_fm_sorted_backward_parity():
    """sorted (emit+sort+segment-reduce) backward == dense reference grads."""
    from lightctr_amd.ops import hip_ops

    row_ptr, fids, vals, labels = make_random_csr(
        B=512, F_total=2000, seed=9, device="cuda:0", binary_vals=False)
    F, K = 2000, 16
    g = torch.Generator().manual_seed(11)
    W = torch.randn(F, generator=g).cuda()
    V = (torch.randn(F, K, generator=g) * 0.1).cuda()
    pred, sumVX = hip_ops.fm_forward(row_ptr, fids, vals, W, V)
    _, dpred = hip_ops.logloss_grad(pred, labels, 1.0 / 512)
    gw, gv = hip_ops.fm_backward_emit(row_ptr, fids, vals, V, sumVX, dpred)
    sorted_fids, perm = torch.sort(fids)
    gradW = torch.zeros(F).cuda()
    gradV = torch.zeros(F, K).cuda()
    touched = torch.zeros((F + 63) // 64, dtype=torch.int64).cuda()
    hip_ops.fm_sorted_apply(sorted_fids, perm, gw, gv, gradW, gradV, touched)
    from lightctr_amd.ops import fm_ref as fr

    gW_ref, gV_ref = fr.fm_backward_ref(row_ptr, fids, vals, V, sumVX, dpred)
    assert torch.allclose(gradW, gW_ref, atol=1e-5, rtol=1e-4)
    assert torch.allclose(gradV, gV_ref, atol=1e-5, rtol=1e-4)
    # bitmap marks exactly the unique fids
    uniq = torch.zeros(F, dtype=torch.int32).cuda()
    count = torch.zeros(1, dtype=torch.int32).cuda()
    hip_ops.bitmap_compact(touched, uniq, count)
    n = int(count.item())
    assert n == torch.unique(fids).numel()


@pytest.mark.gpu
def test_ffm_sorted_backward_parity():
    """Sorted (LDS block segment-reduce) FFM backward == dense reference."""
    from lightctr_amd.ops import hip_ops

    row_ptr, fids, vals, labels = make_random_csr(B=96, F_total=3000,
                                                  min_f=2, max_f=25, seed=17,
                                                  device="cuda:0",
                                                  binary_vals=False)
    nf, K = 6, 8
    fields = (fids.long() % nf).int()
    g = torch.Generator().manual_seed(6)
    W = torch.randn(3000, generator=g).cuda()
    V = (torch.randn(3000, nf, K, generator=g) * 0.1).cuda()
    pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, V)
    _, dpred = hip_ops.logloss_grad(pred, labels, 1.0 / 96)
    gradW = torch.zeros(3000).cuda()
    gradV = torch.zeros(3000, nf, K).cuda()
    touched = torch.zeros((3000 + 63) // 64, dtype=torch.int64).cuda()
    sorted_fids, perm = torch.sort(fids)
    row_of_entry = hip_ops.row_index(row_ptr, fids.numel())
    hip_ops.ffm_sorted_backward(sorted_fids, perm, row_of_entry, row_ptr,
                                fields, fids, vals, V, dpred, gradW, gradV,
                                touched)
    gW_ref, gV_ref = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                              V, dpred)
    assert torch.allclose(gradW, gW_ref, atol=1e-5, rtol=1e-4), \
        (gradW - gW_ref).abs().max()
    assert torch.allclose(gradV, gV_ref, atol=1e-5, rtol=1e-4), \
        (gradV - gV_ref).abs().max()


@pytest.mark.gpu
def test_ffm_blocks_backward_parity():
    """blocks-mode (emit + sorted block reduce) == dense reference."""
    from lightctr_amd.ops import hip_ops

    row_ptr, fids, vals, labels = make_random_csr(B=96, F_total=3000,
                                                  min_f=2, max_f=25, seed=19,
                                                  device="cuda:0",
                                                  binary_vals=False)
    nf, K = 6, 8
    fields = (fids.long() % nf).int()
    g = torch.Generator().manual_seed(8)
    W = torch.randn(3000, generator=g).cuda()
    V = (torch.randn(3000, nf, K, generator=g) * 0.1).cuda()
    pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, V)
    _, dpred = hip_ops.logloss_grad(pred, labels, 1.0 / 96)
    row_of_entry = hip_ops.row_index(row_ptr, fids.numel())
    gw, gblocks = hip_ops.ffm_block_emit(row_of_entry, row_ptr, fields,
                                         fids, vals, V, dpred)
    sorted_fids, perm = torch.sort(fids)
    gradW = torch.zeros(3000).cuda()
    gradV = torch.zeros(3000, nf, K).cuda()
    touched = torch.zeros((3000 + 63) // 64, dtype=torch.int64).cuda()
    hip_ops.ffm_blocks_apply(sorted_fids, perm, gblocks, gw, gradW,
                             gradV.view(3000, -1), touched)
    gW_ref, gV_ref = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                              V, dpred)
    assert torch.allclose(gradW, gW_ref, atol=1e-5, rtol=1e-4), \
        (gradW - gW_ref).abs().max()
    assert torch.allclose(gradV, gV_ref, atol=1e-5, rtol=1e-4), \
        (gradV - gV_ref).abs().max()


@pytest.mark.gpu
def test_ffm_rowemit_backward_parity():
    """rowemit mode (per-row staged fp16 block emit + interior-store
    reduce) == dense reference within fp16 block tolerance. Includes rows
    longer than the staging cap (maxn=40) to cover the in-kernel HBM
    fallback, and duplicate fields per row (LDS-atomic path)."""
    from lightctr_amd.ops import hip_ops

    row_ptr, fids, vals, labels = make_random_csr(B=96, F_total=3000,
                                                  min_f=2, max_f=60, seed=23,
                                                  device="cuda:0",
                                                  binary_vals=False)
    nf, K = 6, 8
    fields = (fids.long() % nf).int()
    g = torch.Generator().manual_seed(8)
    W = torch.randn(3000, generator=g).cuda()
    V = (torch.randn(3000, nf, K, generator=g) * 0.1).cuda()
    pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, V)
    _, dpred = hip_ops.logloss_grad(pred, labels, 1.0 / 96)
    gw, gblocks = hip_ops.ffm_row_emit(row_ptr, fields, fids, vals, V, dpred)
    assert gblocks.dtype == torch.float16
    sorted_fids, perm = torch.sort(fids)
    gradW = torch.zeros(3000).cuda()
    gradV = torch.zeros(3000, nf, K).cuda()
    touched = torch.zeros((3000 + 63) // 64, dtype=torch.int64).cuda()
    hip_ops.ffm_blocks_apply_f16(sorted_fids, perm, gblocks, gw, gradW,
                                 gradV.view(3000, -1), touched)
    gW_ref, gV_ref = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                              V, dpred)
    # gw is fp32 (exact); gv blocks round through fp16 once
    assert torch.allclose(gradW, gW_ref, atol=1e-5, rtol=1e-4), \
        (gradW - gW_ref).abs().max()
    ref_scale = gV_ref.abs().max()
    assert torch.allclose(gradV, gV_ref, atol=float(ref_scale) * 2e-2,
                          rtol=2e-2), (gradV - gV_ref).abs().max()
    # touched bitmap covers exactly the batch's features
    expect = torch.zeros((3000 + 63) // 64, dtype=torch.int64).cuda()
    for f in torch.unique(fids).tolist():
        expect[f // 64] |= 1 << (f % 64)
    assert torch.equal(touched, expect)


@pytest.mark.gpu
def test_ffm_rowemit_fastpath_parity():
    """Duplicate-free rows (one feature per field, the Criteo shape) take
    the round-2 field-map direct-emit fast path in ffm_row_emit_kernel —
    no LDS accumulation at all. Parity vs the dense reference."""
    from lightctr_amd.ops import hip_ops

    g = torch.Generator().manual_seed(77)
    B, nf, K, F = 128, 13, 8, 4000
    # one entry per field, fields 0..nf-1 in order, distinct per row
    fields = torch.arange(nf, dtype=torch.int32).repeat(B).cuda()
    fids = torch.randint(0, F, (B * nf,), generator=g,
                         dtype=torch.int32).cuda()
    vals = (torch.rand(B * nf, generator=g) + 0.5).cuda()
    row_ptr = (torch.arange(B + 1, dtype=torch.int32) * nf).cuda()
    labels = (torch.rand(B, generator=g) > 0.5).float().cuda()
    W = torch.randn(F, generator=g).cuda()
    V = (torch.randn(F, nf, K, generator=g) * 0.1).cuda()
    pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, V)
    _, dpred = hip_ops.logloss_grad(pred, labels, 1.0 / B)
    gw, gblocks = hip_ops.ffm_row_emit(row_ptr, fields, fids, vals, V, dpred)
    sorted_fids, perm = torch.sort(fids)
    gradW = torch.zeros(F).cuda()
    gradV = torch.zeros(F, nf, K).cuda()
    touched = torch.zeros((F + 63) // 64, dtype=torch.int64).cuda()
    hip_ops.ffm_blocks_apply_f16(sorted_fids, perm, gblocks, gw, gradW,
                                 gradV.view(F, -1), touched)
    gW_ref, gV_ref = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                              V, dpred)
    assert torch.allclose(gradW, gW_ref, atol=1e-5, rtol=1e-4), \
        (gradW - gW_ref).abs().max()
    ref_scale = gV_ref.abs().max()
    assert torch.allclose(gradV, gV_ref, atol=float(ref_scale) * 2e-2,
                          rtol=2e-2), (gradV - gV_ref).abs().max()


@pytest.mark.gpu
def test_ffm_bf16_forward_and_backward_parity():
    """bf16 compute mirror (BASELINE config #3): forward and rowemit
    backward on a bf16 V match the fp32 reference within bf16 rounding."""
    from lightctr_amd.ops import hip_ops

    g = torch.Generator().manual_seed(5)
    B, nf, K, F = 96, 11, 8, 3000
    fields = torch.arange(nf, dtype=torch.int32).repeat(B).cuda()
    fids = torch.randint(0, F, (B * nf,), generator=g,
                         dtype=torch.int32).cuda()
    vals = (torch.rand(B * nf, generator=g) + 0.5).cuda()
    row_ptr = (torch.arange(B + 1, dtype=torch.int32) * nf).cuda()
    labels = (torch.rand(B, generator=g) > 0.5).float().cuda()
    W = torch.randn(F, generator=g).cuda()
    V = (torch.randn(F, nf, K, generator=g) * 0.1).cuda()
    Vh = V.to(torch.bfloat16)
    pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, Vh)
    ref = ffm_ref.ffm_forward_ref(row_ptr.cpu(), fields.cpu(), fids.cpu(),
                                  vals.cpu(), W.cpu(),
                                  Vh.float().cpu())
    assert torch.allclose(pred.cpu(), ref, atol=5e-3, rtol=1e-2), \
        (pred.cpu() - ref).abs().max()

    _, dpred = hip_ops.logloss_grad(pred, labels, 1.0 / B)
    gw, gblocks = hip_ops.ffm_row_emit(row_ptr, fields, fids, vals, Vh,
                                       dpred, scale=128.0)
    sorted_fids, perm = torch.sort(fids)
    gradW = torch.zeros(F).cuda()
    gradV = torch.zeros(F, nf, K).cuda()
    touched = torch.zeros((F + 63) // 64, dtype=torch.int64).cuda()
    hip_ops.ffm_blocks_apply_f16(sorted_fids, perm, gblocks, gw, gradW,
                                 gradV.view(F, -1), touched,
                                 inv_scale=1.0 / 128.0)
    gW_ref, gV_ref = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                              Vh.float(), dpred)
    assert torch.allclose(gradW, gW_ref, atol=1e-5, rtol=1e-4)
    ref_scale = gV_ref.abs().max()
    assert torch.allclose(gradV, gV_ref, atol=float(ref_scale) * 3e-2,
                          rtol=3e-2), (gradV - gV_ref).abs().max()


@pytest.mark.gpu
def test_ffm_rowemit_tiny_gradient_scale():
    """At production batch sizes the 1/B-scaled logloss gradients (~1e-8)
    sit below fp16's subnormal floor; the power-of-two block scale must
    preserve them. Emits with dpred ~1e-8 and checks the reduced grads
    against the fp32 reference — without the scale these flush to 0."""
    from lightctr_amd.ops import hip_ops

    g = torch.Generator().manual_seed(13)
    B, nf, K, F = 64, 13, 8, 2000
    fields = torch.arange(nf, dtype=torch.int32).repeat(B).cuda()
    fids = torch.randint(0, F, (B * nf,), generator=g,
                         dtype=torch.int32).cuda()
    vals = (torch.rand(B * nf, generator=g) + 0.5).cuda()
    row_ptr = (torch.arange(B + 1, dtype=torch.int32) * nf).cuda()
    W = torch.randn(F, generator=g).cuda()
    V = (torch.randn(F, nf, K, generator=g) * 0.1).cuda()
    # dpred at the magnitude a B=65536 logloss step produces
    dpred = ((torch.rand(B, generator=g).cuda() - 0.5) * 2e-8)
    scale = float(1 << 16)
    gw, gblocks = hip_ops.ffm_row_emit(row_ptr, fields, fids, vals, V,
                                       dpred, scale=scale)
    sorted_fids, perm = torch.sort(fids)
    gradW = torch.zeros(F).cuda()
    gradV = torch.zeros(F, nf, K).cuda()
    touched = torch.zeros((F + 63) // 64, dtype=torch.int64).cuda()
    hip_ops.ffm_blocks_apply_f16(sorted_fids, perm, gblocks, gw, gradW,
                                 gradV.view(F, -1), touched,
                                 inv_scale=1.0 / scale)
    gW_ref, gV_ref = ffm_ref.ffm_backward_ref(row_ptr, fields, fids, vals,
                                              V, dpred)
    assert float(gV_ref.abs().max()) > 0
    # the unscaled emit would produce gradV == 0 here
    assert float(gradV.abs().max()) > 0
    ref_scale = gV_ref.abs().max()
    assert torch.allclose(gradV, gV_ref, atol=float(ref_scale) * 2e-2,
                          rtol=2e-2), (gradV - gV_ref).abs().max()


@pytest.mark.gpu
def test_ffm_bf16_model_trains():
    """FFMModel(dtype=bf16) end-to-end: loss decreases and the bf16 mirror
    tracks the fp32 master after optimizer steps."""
    from lightctr_amd.models.ffm import FFMHyper, FFMModel

    gen = SyntheticCriteo(num_features=1 << 14, seed=4, device="cuda:0")
    m = FFMModel(FFMHyper(num_features=1 << 14, num_fields=39, k=8,
                          dtype="bf16"), device="cuda:0")
    losses = []
    for i in range(30):
        row_ptr, fields, fids, vals, labels = gen.batch(512)
        loss = m.train_step(row_ptr, fields, fids, vals, labels)
        losses.append(float(loss.mean()))
    assert losses[-1] < losses[0] - 0.02, losses[::10]
    # mirror coherence on touched rows
    diff = (m.Vh.float() - m.V).abs().max()
    assert float(diff) < 0.01, float(diff)


@pytest.mark.gpu
def test_ffm_forward_staged_long_rows():
    """Forward parity on rows spanning the staged/fallback boundary."""
    from lightctr_amd.ops import hip_ops

    row_ptr, fids, vals, labels = make_random_csr(B=64, F_total=2000,
                                                  min_f=30, max_f=55, seed=31,
                                                  device="cuda:0",
                                                  binary_vals=False)
    nf, K = 8, 8
    fields = (fids.long() % nf).int()
    g = torch.Generator().manual_seed(9)
    W = torch.randn(2000, generator=g).cuda()
    V = (torch.randn(2000, nf, K, generator=g) * 0.1).cuda()
    pred = hip_ops.ffm_forward(row_ptr, fields, fids, vals, W, V)
    ref = ffm_ref.ffm_forward_ref(row_ptr.cpu(), fields.cpu(), fids.cpu(),
                                  vals.cpu(), W.cpu(), V.cpu())
    assert torch.allclose(pred.cpu(), ref, atol=1e-3, rtol=1e-4), \
        (pred.cpu() - ref).abs().max()


@pytest.mark.gpu
def test_ffm_fused_apply_matches_two_phase():
    """Optimizer fused into the apply's interior-run flush == the
    two-phase slab+bitmap+sparse-apply path, for both production
    pairings (adagrad and ftrlW+adagradV), fp32 and bf16."""
    from lightctr_amd.models.ffm import FFMHyper, FFMModel

    for opt, dtype in (("adagrad", "fp32"), ("ftrl", "bf16")):
        # num_fields must match the generator's 39 fields
        h = FFMHyper(num_features=1 << 14, num_fields=39, k=8,
                     optimizer=opt, dtype=dtype, seed=21)
        gen = SyntheticCriteo(num_features=1 << 14, seed=9,
                              device="cuda:0")
        a = FFMModel(h, device="cuda:0")
        a.fused_apply = True
        b = FFMModel(h, device="cuda:0")
        b.fused_apply = False
        for _ in range(3):
            row_ptr, fields, fids, vals, labels = gen.batch(2048)
            a.train_step(row_ptr, fields, fids, vals, labels)
            b.train_step(row_ptr, fields, fids, vals, labels)
        # tolerance: spanning runs accumulate via atomics in both paths;
        # the ordering difference (~1e-8/step) compounds through Adagrad
        # to ~1e-6 on hot features over 3 steps (tools/debug_ffm_fused.py
        # classified the only differing fid as a 3-chunk spanning run)
        assert torch.allclose(a.W, b.W, atol=1e-4), \
            (opt, dtype, (a.W - b.W).abs().max())
        assert torch.allclose(a.V, b.V, atol=1e-4), \
            (opt, dtype, (a.V - b.V).abs().max())
        assert torch.allclose(a.nV, b.nV, atol=1e-4)
        if dtype == "bf16":
            assert torch.allclose(a.Vh.float(), a.V, atol=1e-2)


@pytest.mark.gpu
def test_ffm_large_field_product_falls_back():
    """nfields*K beyond the staged-emit/register caps must select the
    sorted backward automatically (and still train)."""
    from lightctr_amd.models.ffm import FFMHyper, FFMModel

    m = FFMModel(FFMHyper(num_features=1 << 12, num_fields=80, k=16),
                 device="cuda:0")
    assert m.backward_mode == "sorted"
    g = torch.Generator().manual_seed(3)
    B, nf = 64, 80
    fields = torch.arange(nf, dtype=torch.int32).repeat(B).cuda()
    fids = torch.randint(0, 1 << 12, (B * nf,), generator=g,
                         dtype=torch.int32).cuda()
    vals = torch.ones(B * nf).cuda()
    row_ptr = (torch.arange(B + 1, dtype=torch.int32) * nf).cuda()
    labels = (torch.rand(B, generator=g) > 0.5).float().cuda()
    W0, V0 = m.W.clone(), m.V.clone()
    for _ in range(3):
        loss = m.train_step(row_ptr, fields, fids, vals, labels)
        assert torch.isfinite(loss).all()
    # a rejected launch would leave the gradients zero and the step a no-op
    live = torch.unique(fids).long()
    assert (m.W[live] != W0[live]).all()
    assert (m.V[live] != V0[live]).any(dim=(1, 2)).all()
    assert torch.isfinite(m.V).all()
