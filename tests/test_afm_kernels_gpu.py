"""afm_forward / afm_backward (ops/csrc/afm_kernels.hip) against the
definition in float64 under autograd (test_afm.afm_autograd). A shape is
(nf, K, A).

Float set: randn inputs scaled as at init, x0 and Wa holding bf16 values; the
batches of a case are the first B rows of one draw. Per output the tolerance
is 8 times the largest error, over the batches, of ops/afm_ref.py with
rounding="bf16" in fp32 on the CPU against the float64 definition: the
reference's own rounding model sets the scale, 8 covers the MFMA summation
order and the exp of the softmax. It is never taken from the kernels' output.
"""

import pytest
import torch

import kernel_oracles as ko
from test_afm import NAMES, PARAMS, afm_autograd, float_case, ref_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOAT = [(2, 4, 16), (3, 16, 16), (7, 5, 16), (18, 8, 32), (6, 64, 16),
         (39, 16, 32), (64, 16, 64)]


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def batch_sizes():
    t = ops().afm_tile_rows()  # one example past one tile and past two
    return (0, 1, 3, t + 1, 2 * t + 1)


def run(c, save=True):
    """the kernels' outputs, every one written over poisoned memory"""
    nf = c["nf"]
    x0 = c["x0"].to(DEV).bfloat16()
    Wbf = c["Wa"].to(DEV).bfloat16()
    Wtbf = c["Wa"].t().contiguous().to(DEV).bfloat16()
    ba, qa, ua, dpred, dDeep = (c[n].to(DEV).clone() for n in
                                ("ba", "qa", "ua", "dpred", "dDeep"))
    B, n = x0.shape[0], Wbf.numel() + 2 * ba.numel() + ua.numel()
    ko.poison((B,), torch.float32, DEV)
    ko.poison((B,), torch.float32, DEV)
    afm, lse = ops().afm_forward(x0, Wbf, ba, qa, ua, nf, save)
    if not save:
        assert lse.numel() == 0
        return afm
    ko.poison((n,), torch.float32, DEV)
    ko.poison((max(ops().afm_backward_chunks(B) * n, 1),), torch.float32, DEV)
    gr = ops().afm_backward(x0, lse, afm, Wbf, Wtbf, ba, qa, ua, dpred, dDeep,
                            nf)
    return dict(zip(NAMES, (afm, dDeep, *gr)))


@pytest.mark.parametrize("nf,K,A", FLOAT)
def test_float_bound(nf, K, A):
    sizes = batch_sizes()
    full = float_case(max(sizes), nf, K, A, seed=77 * nf + K + A)
    runs = []
    for B in sizes:  # the first B rows under the same parameters
        c = {k: v[:B] if k in ("x0", "dpred", "dDeep") else v
             for k, v in full.items()}
        ref, f32 = afm_autograd(c), ref_outputs(c, rounding="bf16")
        err = {n: float((f32[n].double() - ref[n]).abs().max())
               for n in NAMES if ref[n].numel()}
        runs.append((B, ref, err, run(c)))
    for name in NAMES:
        tol = 8 * max(err.get(name, 0.0) for _, _, err, _ in runs)
        print(f"TOL {name} nf={nf} K={K} A={A} {tol:.3e}")
        for B, ref, _, out in runs:
            if B == 0 and name not in ("afm", "dDeep"):
                assert not out[name].any(), name  # empty batch: zeros
            elif ref[name].numel():
                ko.check_bound(f"{name}[B={B}]", out[name], ref[name],
                               torch.full_like(ref[name], tol))


def test_deterministic_and_save_off():
    c = float_case(37, 39, 16, 32, seed=5)  # three tiles, the last short
    a, b = run(c), run(c)
    for name in NAMES:
        ko.check_bits(name, a[name], b[name].cpu())
        assert a[name].any(), name
    assert not torch.equal(a["dDeep"].cpu(), c["dDeep"])
    ko.check_bits("afm, save off", run(c, save=False), a["afm"].cpu())


BAD = {"nf = 1": (dict(nf=1), r"in \[2, 64\], got 1"),
       "nf = 65": (dict(nf=65), r"in \[2, 64\], got 65"),
       "nf*K = 1088": (dict(nf=64, K=17), "at most 1024, got 1088"),
       "K = 65": (dict(K=65), "at most 64, got 65"),
       "A = 24": (dict(A=24), r"in \[16, 64\], got 24"),
       "A = 80": (dict(A=80), r"in \[16, 64\], got 80"),
       "B*nf = 2^24": (dict(nf=64, K=1, B=1 << 18), "2\\^24, got 16777216")}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(what):
    kw, msg = BAD[what]
    s = {**dict(nf=2, K=4, A=16, B=4), **kw}
    z = lambda *sh, dt=torch.float32: torch.zeros(*sh, dtype=dt, device=DEV)
    x0 = z(s["B"], s["nf"] * s["K"], dt=torch.bfloat16)
    W = z(s["K"], s["A"], dt=torch.bfloat16)
    w = (z(s["A"]), z(s["A"]), z(s["K"]))
    with pytest.raises(RuntimeError, match=msg):
        ops().afm_forward(x0, W, *w, s["nf"], False)
    with pytest.raises(RuntimeError, match=msg):
        ops().afm_backward(x0, z(1), z(1), W, W, *w, z(1), z(1), s["nf"])


@pytest.mark.parametrize("layout", ("position", "field"))
def test_model_hip_against_torch(layout):
    """Three steps of the two arms from one seed, the bounds derived as
    test_autoint_kernels_gpu's twin derives them: both arms read the same
    bf16 mirror and round at the same points, and each is within 8 eps of the
    float64 definition, eps being the error of the bf16-rounded reference
    (fp32, CPU) on the torch arm's own concat, parameters and dpred of step 0,
    per output. Step 0 starts from equal parameters, so the losses differ by
    the attention terms only: 16 eps(afm). The arms' gradients then differ by
    at most 16 eps of dDeep and of the four dense gradients, and Adagrad turns
    a gradient difference e into at most e lr / sqrt(1e-8) on a parameter:
    500 e for E and the wide W (lr 0.05), 10 e for the dense ones (mlp_lr
    1e-3), once a step, so 3 times after three steps. Each arm also rounds
    the stored fp32 parameter once a step, half an ulp each: 3 * 2^-23 |p| on
    top, which is what is left where the gradients agree far below an ulp of
    the step (ua here). The later losses keep the 1e-5 of the twin. predict
    is the training forward with save off."""
    from lightctr_amd.data.synthetic import SyntheticMultiHot
    from lightctr_amd.models.afm import AFMHyper, AFMModel

    nf, K, F, B = 5, 8, 1 << 10, 64
    h = AFMHyper(num_features=F, num_fields=nf, k=K, hidden=(32, 16),
                 mlp_optimizer="adagrad", attn_factor=16, layout=layout,
                 pooling="mean", seed=11)
    hip = AFMModel(h, device=DEV, afm_impl="hip")
    ref = AFMModel(h, device=DEV, afm_impl="torch")
    gen = SyntheticMultiHot(num_features=F, num_fields=nf, multi=(1, 3),
                            max_multi=3, seed=2, device=DEV)
    for step in range(3):
        row_ptr, fields, fids, vals, labels = gen.batch(B)
        if step == 0:
            fl = hip._fields(fields)
            pred, _ = hip._forward_gpu(row_ptr, fids, vals, fields=fl)
            ko.check_bits("predict", hip.predict_proba(
                row_ptr, fids, vals, fields=fields),
                torch.sigmoid(pred.clamp(-16, 16)).cpu())
            score, _ = ref._forward_gpu(row_ptr, fids, vals, train=False,
                                        fields=fl)
            dpred = (torch.sigmoid(score.clamp(-16, 16)) - labels) / B
            c = {"nf": nf, "x0": ref._saved[0].cpu(),
                 "Wa": ref.Wabf.float().cpu(), "dpred": dpred.cpu(),
                 "dDeep": torch.zeros(B, nf * K),
                 **{n: getattr(ref, n).cpu() for n in PARAMS[1:]}}
            f32, f64 = ref_outputs(c, rounding="bf16"), afm_autograd(c)
            err = lambda n: float((f32[n].double() - f64[n]).abs().max())
            eps = err("afm")
            tols = {"E": 3 * 500 * 16 * err("dDeep"),
                    **{n: 3 * 10 * 16 * err("d" + n) for n in PARAMS}}
            tols["W"] = tols["E"]
        lh = hip.train_step(row_ptr, fids, vals, labels, fields=fields)
        lr = ref.train_step(row_ptr, fids, vals, labels, fields=fields)
        tol = 16 * eps + 2 * ko.U23 if step == 0 else 1e-5
        print(f"STEP {step} eps {eps:.3e} "
              f"dloss {float((lh - lr).abs().max()):.3e}")
        torch.testing.assert_close(lh, lr, rtol=0, atol=tol)
    for name, tol in tols.items():
        tol += 3 * ko.U23 * float(getattr(ref, name).abs().max())
        diff = (getattr(hip, name) - getattr(ref, name)).abs().max()
        print(f"PARAM {name} {float(diff):.3e} tol {tol:.3e}")
        torch.testing.assert_close(getattr(hip, name), getattr(ref, name),
                                   rtol=0, atol=tol,
                                   msg=lambda m: f"{name}: {m}")
    assert not torch.equal(ref.ua.cpu(), AFMModel(h).ua)
    assert torch.equal(hip.Watbf, hip.Wa.t().bfloat16())
    assert torch.equal(hip.Wabf, hip.Wa.bfloat16())
