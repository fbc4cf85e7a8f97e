"""cin_forward / cin_backward / cin_wgrad (ops/csrc/cin_kernels.hip) against
the layer-by-layer definition in float64 under autograd
(test_xdeepfm.cin_autograd).

Exact set: x0 in {-1, 0, 1}; every map of W^l has at most two entries of +-1,
one at a corner of the (i, j) range (i = 0 or H_{l-1}-1, j = 0 or m-1, in
turn over the maps) and one anywhere, so |X^l| <= 2^l; u with 3 entries of
+-1 a layer, dpred and the incoming dDeep in {-2..2}. The definition run on
the absolute values of the inputs bounds every term: what passes through bf16
(X, dX, and the generated product, which is below |X|) is asserted to stay
below 2^8 and every fp32 sum below 2^24, so all of it is integers that both
formats hold in any summation order and the comparison is bit equality, up to
the sign of a zero (+ 0.0 on both sides).

Float set: randn inputs, W and u scaled as at init, x0 and W holding bf16
values; the batches of a case are the first B rows of one draw. Per output
the tolerance is 8 times the largest error, over the batches of the case, of
ops/cin_ref.py with rounding="bf16" run in fp32 torch on the CPU against the
float64 definition on the same inputs: the reference's own rounding model
sets the scale, 8 covers the MFMA summation order. It is never taken from the
kernels' output.
"""

import pytest
import torch

import kernel_oracles as ko
from lightctr_amd.ops import cin_ref
from test_xdeepfm import cin_autograd, float_case, ref_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NFS, KS, HS, LS = (1, 7, 8, 9, 39, 64), (1, 5, 16), (16, 48, 128), (1, 2, 4)
# every nf with every L; K and H in turn, so that each value appears
EXACT = [(nf, KS[(a + b) % 3], HS[(a + 2 * b) % 3], L)
         for a, nf in enumerate(NFS) for b, L in enumerate(LS)]
FLOAT = [(39, 16, 64, 2), (39, 16, 64, 4), (7, 5, 16, 1), (9, 1, 48, 2),
         (64, 16, 128, 2)]


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def batch_sizes(K):
    t = ops().cin_tile_rows()  # B*K one row past one tile and past two
    return (0, 1, 3, -(-(t + 1) // K), -(-(2 * t + 1) // K))


def exact_case(B, nf, K, H, L, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)
    W = []
    for l in range(L):
        hp = nf if l == 0 else H
        w, h = torch.zeros(H, hp, nf), torch.arange(H)
        w[h, ri(0, hp - 1, H), ri(0, nf - 1, H)] = ri(0, 1, H) * 2.0 - 1
        w[h, (h % 2) * (hp - 1), (h // 2 % 2) * (nf - 1)] = \
            ri(0, 1, H) * 2.0 - 1
        W.append(w)
    u = torch.zeros(L, H).scatter_(1, ri(0, H - 1, L, 3),
                                   ri(0, 1, L, 3) * 2.0 - 1)
    return {"nf": nf, "x0": ri(-1, 1, B, nf * K).float(), "W": W, "u": u,
            "dpred": ri(-2, 2, B).float(),
            "dDeep": ri(-2, 2, B, nf * K).float()}


def kernel_order(W, nf, transposed=False):
    """the flat buffer of the layers' [H, Kl] (or [Kl, H]) matrices"""
    flat = []
    for w in W:
        idx, cols = cin_ref.cin_order(nf, w.shape[1])
        m = torch.zeros(w.shape[0], cols, dtype=w.dtype)
        m[:, idx.flatten()] = w.flatten(1)
        flat.append((m.t() if transposed else m).flatten())
    return torch.cat(flat)


def run(c, save=True):
    """the kernels' outputs, every one written over poisoned memory; dW comes
    back in kernel order and is compared in that order, pads included"""
    nf, W, L = c["nf"], c["W"], len(c["W"])
    x0 = c["x0"].to(DEV).bfloat16()
    Wbf = kernel_order(W, nf).to(DEV).bfloat16()
    Wtbf = kernel_order(W, nf, True).to(DEV).bfloat16()
    u, dpred, dDeep = (c[n].to(DEV).clone() for n in ("u", "dpred", "dDeep"))
    B, K, H = x0.shape[0], x0.shape[1] // nf, u.shape[1]
    saved, bf = (L, B, K, H), torch.bfloat16
    ko.poison((B,), torch.float32, DEV)
    ko.poison(saved, bf, DEV)
    fwd = ops().cin_forward(x0, Wbf, u, nf, save)
    if not save:
        return fwd
    cin, X = fwd
    ko.poison(saved, bf, DEV)
    ko.poison((L, H), torch.float32, DEV)
    dX, du = ops().cin_backward(x0, X, Wtbf, u, dpred, dDeep, nf)
    ko.poison((Wbf.numel(),), torch.float32, DEV)
    dW = ops().cin_wgrad(x0, X, dX, u, nf)
    return {"cin": cin, "X": X, "dX": dX, "dDeep": dDeep, "du": du, "dW": dW}


def with_flat_dw(ref, nf, L):
    ref["dW"] = kernel_order([ref[f"dW{l}"] for l in range(L)], nf)
    return ref


NAMES = ("cin", "X", "dX", "dDeep", "du", "dW")


@pytest.mark.parametrize("nf,K,H,L", EXACT)
def test_exact(nf, K, H, L):
    for B in batch_sizes(K):
        c = exact_case(B, nf, K, H, L, seed=1000 * L + 10 * nf + H + B)
        ref = with_flat_dw(cin_autograd(c), nf, L)
        mag = with_flat_dw(cin_autograd(
            {k: [w.abs() for w in v] if k == "W" else
             v if k == "nf" else v.abs() for k, v in c.items()}), nf, L)
        out = run(c)
        for name in NAMES:
            held = name in ("X", "dX")
            assert not (mag[name] >= (2 ** 8 if held else 2 ** 24)).any(), (
                name, B)
            dt = torch.bfloat16 if held else torch.float32
            ko.check_bits(f"{name}[B={B}]", out[name] + 0.0,
                          (ref[name] + 0.0).to(dt))


@pytest.mark.parametrize("nf,K,H,L", FLOAT)
def test_float_bound(nf, K, H, L):
    sizes = batch_sizes(K)
    full = float_case(max(sizes), nf, K, H, L, seed=77 * L + 10 * nf + H)
    runs = []
    for B in sizes:  # the first B rows under the same parameters
        c = {k: v[:B] if k in ("x0", "dpred", "dDeep") else v
             for k, v in full.items()}
        ref = with_flat_dw(cin_autograd(c), nf, L)
        f32 = with_flat_dw(ref_outputs(c, rounding="bf16"), nf, L)
        err = {n: float((f32[n].double() - ref[n]).abs().max())
               for n in NAMES if ref[n].numel()}
        runs.append((B, ref, err, run(c)))
    for name in NAMES:
        tol = 8 * max(err.get(name, 0.0) for _, _, err, _ in runs)
        print(f"TOL {name} nf={nf} K={K} H={H} L={L} {tol:.3e}")
        for B, ref, _, out in runs:
            if B == 0 and name in ("du", "dW"):
                assert not out[name].any(), name  # empty batch: zeros
            elif ref[name].numel():
                ko.check_bound(f"{name}[B={B}]", out[name], ref[name],
                               torch.full_like(ref[name], tol))


def test_deterministic_and_save_off():
    c = float_case(27, 39, 16, 64, 2, seed=5)  # 432 rows: three full tiles on
    a, b = run(c), run(c)
    for name in NAMES:
        ko.check_bits(name, a[name], b[name].cpu())
    assert a["du"].any() and a["dW"].any() and a["dX"].any()
    (cin,) = run(c, save=False)
    ko.check_bits("cin, save off", cin, a["cin"].cpu())


BAD = {"nf = 65": (dict(nf=65), r"in \[1, 64\], got 65"),
       "nf*K = 1088": (dict(nf=64, K=17), "at most 1024, got 1088"),
       "H = 24": (dict(H=24), r"in \[16, 128\], got 24"),
       "H = 144": (dict(H=144), r"in \[16, 128\], got 144"),
       "L = 5": (dict(L=5), "<= 4, got 5"),
       "B*K = 2^24": (dict(nf=1, K=1024, B=1 << 14), "2\\^24, got 16777216")}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(what):
    kw, msg = BAD[what]
    s = {**dict(nf=2, K=4, H=16, L=2, B=4), **kw}
    z = lambda *sh, dt=torch.bfloat16: torch.zeros(*sh, dtype=dt, device=DEV)
    x0, u = z(s["B"], s["nf"] * s["K"]), z(s["L"], s["H"], dt=torch.float32)
    with pytest.raises(RuntimeError, match=msg):
        ops().cin_forward(x0, z(16), u, s["nf"], False)
    with pytest.raises(RuntimeError, match=msg):
        ops().cin_backward(x0, z(1), z(16), u, z(1), z(1), s["nf"])
    with pytest.raises(RuntimeError, match=msg):
        ops().cin_wgrad(x0, z(1), z(1), u, s["nf"])


@pytest.mark.parametrize("layout", ("position", "field"))
def test_model_hip_against_torch(layout):
    """Three steps of the two arms from one seed, with the float-set bound
    scaled as test_dcn2_kernels_gpu's twin test scales it: both arms read the
    same bf16 mirror and round at the same points, and each is within 8 eps
    of the float64 definition, eps being the error of the bf16-rounded
    reference (fp32, CPU) on the torch arm's own concat, parameters and dpred
    of step 0, per output. Step 0 starts from equal parameters, so the losses
    differ by the CIN terms only: 16 eps(cin). The arms' gradients then differ
    by at most 16 eps of dDeep, dW and du, and Adagrad turns a gradient
    difference e into at most e lr / sqrt(1e-8) on a parameter: 500 e for E
    and the wide W (lr 0.05), 10 e for the dense ones (mlp_lr 1e-3), once a
    step, so 3 times after three steps. The later losses keep the 1e-5 of the
    DCN-v2 twin. predict is the training forward with save off."""
    from lightctr_amd.data.synthetic import SyntheticMultiHot
    from lightctr_amd.models.xdeepfm import XDeepFMHyper, XDeepFMModel

    nf, K, F, B = 5, 8, 1 << 10, 64
    h = XDeepFMHyper(num_features=F, num_fields=nf, k=K, hidden=(32, 16),
                     mlp_optimizer="adagrad", cin_layers=3, cin_maps=16,
                     layout=layout, pooling="mean", seed=11)
    hip = XDeepFMModel(h, device=DEV, cin_impl="hip")
    ref = XDeepFMModel(h, device=DEV, cin_impl="torch")
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
                 "W": [w.cpu() for w in ref.canonical(ref.Wkbf.float())],
                 "u": ref.u.cpu(), "dpred": dpred.cpu(),
                 "dDeep": torch.zeros(B, nf * K)}
            f32, f64 = ref_outputs(c, rounding="bf16"), cin_autograd(c)
            err = lambda *ns: max(float((f32[n].double() - f64[n]).abs().max())
                                  for n in ns)
            eps = err("cin")
            tols = {"E": 3 * 500 * 16 * err("dDeep"),
                    "Wk": 3 * 10 * 16 * err("dW0", "dW1", "dW2"),
                    "u": 3 * 10 * 16 * err("du")}
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
    assert not torch.equal(ref.u.cpu(), XDeepFMModel(h).u)
    assert torch.equal(hip._layer(hip.Wktbf, 1, True),
                       hip._layer(hip.Wk, 1).t().bfloat16())
