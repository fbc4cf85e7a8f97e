"""autoint_forward / autoint_backward (ops/csrc/autoint_kernels.hip) against
the definition in float64 under autograd (test_autoint.attn_autograd). A shape
is (nf, K, heads, head_dim, L).

Exact set: W_Q = 0 in the even layers and W_K = 0 in the odd ones, so every
score is 0 and every softmax uniform over nf keys, nf a power of two; dS and
the gradient of the zeroed block are still nonzero. x0 in {-1, 0, 1}, mostly
0; every column of the other blocks of W has one entry of +-1 and the four
corners of a block one more; u has 3 entries of +-1, dpred and the incoming
dDeep are in {-2..2}. Exactness is asserted on the reference, not assumed:
ops/autoint_ref.py runs in float64 with its rounder replaced by a check that
the tensor is a bf16 value already (every tensor the kernels hold in bf16
passes through it), and every fp32 output has to survive .float(). The
comparison is then bit equality, up to the sign of a zero. All seven candidate
shapes pass that check on the CPU; none left the list.

Float set: randn inputs scaled as at init, x0 and W holding bf16 values; the
batches of a case are the first B rows of one draw. Per output the tolerance
is 8 times the largest error, over the batches, of ops/autoint_ref.py with
rounding="bf16" in fp32 on the CPU against the float64 definition: the
reference's own rounding model sets the scale, 8 covers the MFMA summation
order and the exp of the softmax. It is never taken from the kernels' output.
"""

import pytest
import torch

import kernel_oracles as ko
from lightctr_amd.ops import autoint_ref
from test_autoint import attn_autograd, float_case, ref_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EXACT = [(1, 5, 1, 16, 4), (2, 16, 2, 32, 4), (2, 1, 4, 16, 3),
         (4, 5, 2, 16, 2), (4, 16, 1, 32, 2), (8, 16, 2, 32, 1),
         (16, 8, 4, 16, 1)]
FLOAT = [(39, 16, 2, 32, 3), (39, 16, 4, 16, 2), (7, 5, 1, 16, 1),
         (17, 8, 1, 32, 4), (64, 16, 2, 32, 2)]


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def batch_sizes():
    t = ops().autoint_tile_rows()  # one example past one tile and past two
    return (0, 1, 3, t + 1, 2 * t + 1)


def exact_case(B, nf, K, heads, hd, L, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    D, W = heads * hd, []
    for l in range(L):
        din = D if l else K
        w = torch.zeros(din, 4, D)
        for blk in range(4):
            if blk == l % 2:  # W_Q or W_K of this layer stays zero
                continue
            w[ri(0, din - 1, D), blk, torch.arange(D)] = ri(0, 1, D) * 2.0 - 1
            for r, c in ((0, 0), (0, D - 1), (din - 1, 0), (din - 1, D - 1)):
                w[r, blk, c] = float(ri(0, 1)) * 2 - 1
        W.append(w.view(din, 4 * D))
    u = torch.zeros(nf * D).scatter_(0, ri(0, nf * D - 1, 3),
                                     ri(0, 1, 3) * 2.0 - 1).view(nf, D)
    x0 = ri(-1, 1, B, nf * K).float() * (ri(0, 3, B, nf * K) == 0)
    return {"nf": nf, "heads": heads, "x0": x0, "W": W, "u": u,
            "dpred": ri(-2, 2, B).float(),
            "dDeep": ri(-2, 2, B, nf * K).float()}


def run(c, save=True):
    """the kernels' outputs, every one written over poisoned memory"""
    nf, heads, L = c["nf"], c["heads"], len(c["W"])
    x0 = c["x0"].to(DEV).bfloat16()
    Wbf = torch.cat([w.flatten() for w in c["W"]]).to(DEV).bfloat16()
    Wtbf = torch.cat([w.t().flatten() for w in c["W"]]).to(DEV).bfloat16()
    u, dpred, dDeep = (c[n].to(DEV).clone() for n in ("u", "dpred", "dDeep"))
    B, D = x0.shape[0], u.shape[1]
    ko.poison((B,), torch.float32, DEV)
    ko.poison((L, B, nf, D), torch.bfloat16, DEV)
    fwd = ops().autoint_forward(x0, Wbf, u, nf, heads, D // heads, save)
    if not save:
        return fwd
    ko.poison((Wbf.numel(),), torch.float32, DEV)
    ko.poison((nf, D), torch.float32, DEV)
    dW, du = ops().autoint_backward(x0, fwd[1], Wbf, Wtbf, u, dpred, dDeep,
                                    nf, heads, D // heads)
    return {"ai": fwd[0], "X": fwd[1], "dDeep": dDeep, "du": du, "dW": dW}


def with_flat_dw(ref, L):
    ref["dW"] = torch.cat([ref[f"dW{l}"].flatten() for l in range(L)])
    return ref


NAMES = ("ai", "X", "dDeep", "du", "dW")


@pytest.mark.parametrize("nf,K,heads,hd,L", EXACT)
def test_exact(nf, K, heads, hd, L, monkeypatch):
    for B in batch_sizes():
        c = exact_case(B, nf, K, heads, hd, L, seed=1000 * L + 10 * nf + B)
        ref = with_flat_dw(attn_autograd(c), L)
        held = []  # is every tensor the kernels round a bf16 value already?
        monkeypatch.setattr(autoint_ref, "_rounder", lambda r: lambda t: (
            held.append(bool((t.bfloat16().to(t.dtype) == t).all())), t)[1])
        f64 = ref_outputs({k: [w.double() for w in v] if k == "W" else v if
                           k in ("nf", "heads") else v.double()
                           for k, v in c.items()}, rounding="bf16")
        monkeypatch.undo()
        assert held and all(held), (B, held)
        assert torch.equal(f64["X"], ref["X"])
        out = run(c)
        for name in NAMES:
            dt = torch.bfloat16 if name == "X" else torch.float32
            assert torch.equal(ref[name].to(dt).double(), ref[name]), (name, B)
            ko.check_bits(f"{name}[B={B}]", out[name] + 0.0,
                          (ref[name] + 0.0).to(dt))


@pytest.mark.parametrize("nf,K,heads,hd,L", FLOAT)
def test_float_bound(nf, K, heads, hd, L):
    sizes = batch_sizes()
    full = float_case(max(sizes), nf, K, heads, hd, L, seed=77 * L + nf + hd)
    runs = []
    for B in sizes:  # the first B rows under the same parameters
        c = {k: v[:B] if k in ("x0", "dpred", "dDeep") else v
             for k, v in full.items()}
        ref = with_flat_dw(attn_autograd(c), L)
        f32 = with_flat_dw(ref_outputs(c, rounding="bf16"), L)
        err = {n: float((f32[n].double() - ref[n]).abs().max())
               for n in NAMES if ref[n].numel()}
        runs.append((B, ref, err, run(c)))
    for name in NAMES:
        tol = 8 * max(err.get(name, 0.0) for _, _, err, _ in runs)
        print(f"TOL {name} nf={nf} K={K} heads={heads} hd={hd} L={L} "
              f"{tol:.3e}")
        for B, ref, _, out in runs:
            if B == 0 and name in ("du", "dW"):
                assert not out[name].any(), name  # empty batch: zeros
            elif ref[name].numel():
                ko.check_bound(f"{name}[B={B}]", out[name], ref[name],
                               torch.full_like(ref[name], tol))


def test_deterministic_and_save_off():
    c = float_case(37, 39, 16, 2, 32, 3, seed=5)  # three tiles, the last short
    a, b = run(c), run(c)
    for name in NAMES:
        ko.check_bits(name, a[name], b[name].cpu())
    assert a["du"].any() and a["dW"].any()
    assert not torch.equal(a["dDeep"].cpu(), c["dDeep"])
    (ai,) = run(c, save=False)
    ko.check_bits("ai, save off", ai, a["ai"].cpu())


BAD = {"nf = 65": (dict(nf=65), r"in \[1, 64\], got 65"),
       "nf*K = 1088": (dict(nf=64, K=17), "at most 1024, got 1088"),
       "K = 65": (dict(K=65), "at most 64, got 65"),
       "heads = 3": (dict(heads=3), "1, 2 or 4, got 3"),
       "head_dim = 24": (dict(hd=24), "16 or 32, got 24"),
       "D = 128": (dict(heads=4, hd=32), "at most 64, got 128"),
       "L = 5": (dict(L=5), "<= 4, got 5"),
       "B*nf = 2^24": (dict(nf=64, K=1, B=1 << 18), "2\\^24, got 16777216")}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(what):
    kw, msg = BAD[what]
    s = {**dict(nf=2, K=4, heads=1, hd=16, L=2, B=4), **kw}
    D = s["heads"] * s["hd"]
    z = lambda *sh, dt=torch.bfloat16: torch.zeros(*sh, dtype=dt, device=DEV)
    x0, u = z(s["B"], s["nf"] * s["K"]), z(s["nf"], D, dt=torch.float32)
    W = z((s["K"] + (s["L"] - 1) * D) * 4 * D)
    a = (s["nf"], s["heads"], s["hd"])
    with pytest.raises(RuntimeError, match=msg):
        ops().autoint_forward(x0, W, u, *a, False)
    with pytest.raises(RuntimeError, match=msg):
        ops().autoint_backward(x0, z(1), W, W, u, z(1), z(1), *a)


@pytest.mark.parametrize("layout", ("position", "field"))
def test_model_hip_against_torch(layout):
    """Three steps of the two arms from one seed, the bounds derived as
    test_cin_kernels_gpu's twin derives them: both arms read the same bf16
    mirror and round at the same points, and each is within 8 eps of the
    float64 definition, eps being the error of the bf16-rounded reference
    (fp32, CPU) on the torch arm's own concat, parameters and dpred of step 0,
    per output. Step 0 starts from equal parameters, so the losses differ by
    the attention terms only: 16 eps(ai). The arms' gradients then differ by
    at most 16 eps of dDeep, dW and du, and Adagrad turns a gradient
    difference e into at most e lr / sqrt(1e-8) on a parameter: 500 e for E
    and the wide W (lr 0.05), 10 e for the dense ones (mlp_lr 1e-3), once a
    step, so 3 times after three steps. The later losses keep the 1e-5 of the
    twin. predict is the training forward with save off."""
    from lightctr_amd.data.synthetic import SyntheticMultiHot
    from lightctr_amd.models.autoint import AutoIntHyper, AutoIntModel

    nf, K, F, B = 5, 8, 1 << 10, 64
    h = AutoIntHyper(num_features=F, num_fields=nf, k=K, hidden=(32, 16),
                     mlp_optimizer="adagrad", attn_layers=3, attn_heads=2,
                     attn_dim=16, layout=layout, pooling="mean", seed=11)
    hip = AutoIntModel(h, device=DEV, attn_impl="hip")
    ref = AutoIntModel(h, device=DEV, attn_impl="torch")
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
            c = {"nf": nf, "heads": 2, "x0": ref._saved[0].cpu(),
                 "W": [w.cpu() for w in ref.layers(ref.Wabf.float())],
                 "u": ref.ua.cpu(), "dpred": dpred.cpu(),
                 "dDeep": torch.zeros(B, nf * K)}
            f32, f64 = ref_outputs(c, rounding="bf16"), attn_autograd(c)
            err = lambda *ns: max(float((f32[n].double() - f64[n]).abs().max())
                                  for n in ns)
            eps = err("ai")
            tols = {"E": 3 * 500 * 16 * err("dDeep"),
                    "Wa": 3 * 10 * 16 * err("dW0", "dW1", "dW2"),
                    "ua": 3 * 10 * 16 * err("du")}
            tols["W"] = tols["E"]
        lh = hip.train_step(row_ptr, fids, vals, labels, fields=fields)
        lr = ref.train_step(row_ptr, fids, vals, labels, fields=fields)
        tol = 16 * eps + 2 * ko.U23 if step == 0 else 1e-5
        print(f"STEP {step} eps {eps:.3e} "
              f"dloss {float((lh - lr).abs().max()):.3e}")
        torch.testing.assert_close(lh, lr, rtol=0, atol=tol)
    for name, tol in tols.items():
        diff = (getattr(hip, name) - getattr(ref, name)).abs().max()
        print(f"PARAM {name} {float(diff):.3e} tol {tol:.3e}")
        torch.testing.assert_close(getattr(hip, name), getattr(ref, name),
                                   rtol=0, atol=tol,
                                   msg=lambda m: f"{name}: {m}")
    assert not torch.equal(ref.ua.cpu(), AutoIntModel(h).ua)
    assert torch.equal(hip._layer(hip.Watbf, 1, True),
                       hip._layer(hip.Wa, 1).t().bfloat16())
    assert torch.equal(hip.Wabf, hip.Wa.bfloat16())
