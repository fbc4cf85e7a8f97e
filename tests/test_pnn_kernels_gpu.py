"""pnn_forward / pnn_backward (ops/csrc/pnn_kernels.hip) against the float64
definition (test_pnn.pnn_autograd). A shape is (nf, K); the batches of a case
are the first B rows of one draw. Exact set: e and dz from {-1, 0, 1}, so
|g| <= 64 is exact in bf16 and |dDeep| <= 129 in fp32 in any order of the
sums: bit equality. Float set: per output the tolerance is 8 times the error
of ops/pnn_ref.py with rounding="bf16" in fp32 on the CPU against float64 (8
covers the MFMA summation order and a rounding of g or of a pair gradient
that falls the other way); it is never taken from the kernels' output.
"""

import pytest
import torch

import kernel_oracles as ko
from test_pnn import SHAPES, exact_case, float_case, pnn_autograd, ref_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def batch_sizes():
    t = ops().pnn_tile_rows()  # one example past one sweep and past two
    return (0, 1, 3, t + 1, 2 * t + 1)


def run(x0, dz, nf):
    """(z, dDeep) of the kernels, both written over poisoned memory"""
    xg, dg = x0.to(DEV).bfloat16(), dz.to(DEV)
    ko.poison((x0.shape[0], dz.shape[1]), torch.bfloat16, DEV)
    z = ops().pnn_forward(xg, nf)
    ko.poison(tuple(x0.shape), torch.float32, DEV)
    return z, ops().pnn_backward(z, dg, nf, x0.shape[1] // nf)


@pytest.mark.parametrize("nf,K", SHAPES)
def test_exact_bits(nf, K):
    x0, dz = exact_case(max(batch_sizes()), nf, K, seed=31 * nf + K)
    z64, dD64 = pnn_autograd(x0, dz, nf)  # its pad is +0 (test_pnn)
    assert ops().pnn_out_dim(nf, K) == z64.shape[1]
    for B in batch_sizes():
        z, dDeep = run(x0[:B], dz[:B], nf)
        ko.check_bits(f"z[B={B}]", z, z64[:B].bfloat16())
        ko.check_bits(f"dDeep[B={B}]", dDeep, dD64[:B].float())


@pytest.mark.parametrize("nf,K", SHAPES)
def test_float_bound(nf, K):
    x0, dz = float_case(max(batch_sizes()), nf, K, seed=77 * nf + K)
    z64, dD64 = pnn_autograd(x0, dz, nf)
    zr, dr = ref_outputs(x0, dz, nf, rounding="bf16")
    tz = 8 * float((zr.double() - z64).abs().max())
    td = 8 * float((dr.double() - dD64).abs().max())
    print(f"TOL nf={nf} K={K} z {tz:.3e} dDeep {td:.3e}")
    for B in batch_sizes():
        z, dDeep = run(x0[:B], dz[:B], nf)
        ko.check_bound(f"z[B={B}]", z, z64[:B], torch.full_like(z64[:B], tz))
        ko.check_bound(f"dDeep[B={B}]", dDeep, dD64[:B],
                       torch.full_like(dD64[:B], td))
        ko.check_bits(f"x0 in z[B={B}]", z[:, :nf * K], x0[:B].bfloat16())


def test_deterministic():
    x0, dz = float_case(37, 39, 16, seed=5)
    a, b = run(x0, dz, 39), run(x0, dz, 39)
    for name, u, v in zip(("z", "dDeep"), a, b):
        ko.check_bits(name, u, v.cpu())
        assert u.any(), name


def _args(nf=2, K=4, x0w=None, zw=None, dzw=None, x0dt=torch.bfloat16,
          dzdt=torch.float32, dev=DEV, strided=False):
    Dz = (nf * K + nf * (nf - 1) // 2 + 7) // 8 * 8
    mk = lambda w, dt: torch.zeros(4, 2 * w if strided else w, dtype=dt,
                                   device=dev)[:, :w]
    return (mk(x0w or nf * K, x0dt), mk(zw or Dz, torch.bfloat16),
            mk(dzw or Dz, dzdt))


BAD = {  # what: (f = forward and / or b = backward, arguments, message)
       "nf = 1": ("fb", dict(nf=1), r"in \[2, 64\], got 1"),
       "nf = 65": ("fb", dict(nf=65), r"in \[2, 64\], got 65"),
       "K = 5": ("fb", dict(K=5), "4, 8, 16, 32 or 64, got 5"),
       "nf*K = 2048": ("fb", dict(nf=32, K=64), "at most 1024, got 2048"),
       "x0 width": ("f", dict(x0w=9), "got width 9"),
       "z width": ("b", dict(zw=24), r"z must be \[B, Dz.*got width 24"),
       "dz width": ("b", dict(dzw=24), r"dz must be \[B, Dz.*got width 24"),
       "x0 dtype": ("f", dict(x0dt=torch.float32), "x0 must be bf16"),
       "dz dtype": ("b", dict(dzdt=torch.bfloat16), "dz must be fp32"),
       "device": ("fb", dict(dev="cpu"), "must be on GPU"),
       "strided": ("fb", dict(strided=True), "must be contiguous")}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(what):
    which, kw, msg = BAD[what]
    nf, K = kw.get("nf", 2), kw.get("K", 4)
    x0, z, dz = _args(**kw)
    if "f" in which:
        with pytest.raises(RuntimeError, match=msg):
            ops().pnn_forward(x0, nf)
    if "b" in which:
        with pytest.raises(RuntimeError, match=msg):
            ops().pnn_backward(z, dz, nf, K)


def test_batch_limit():
    """B*Dz = 706421 * 3040 >= 2^31, on one row of storage, expanded"""
    x0 = torch.zeros(1, 1024, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match=r"2\^31, got 2147519840"):
        ops().pnn_forward(x0.expand(706421, 1024), 64)


@pytest.mark.parametrize("layout", ("position", "field"))
def test_model_hip_against_torch(layout):
    """Three steps of both arms from one seed, bounds as in
    test_afm_kernels_gpu's twin: each arm is within 8 eps of float64, eps the
    error of the bf16-rounded reference (fp32, CPU) on the torch arm's concat
    and dz of step 0. Step 0: the scores differ by at most 16 eps(z) times the
    largest row sum of |d score / d z| over the pair columns (the log loss is
    1-Lipschitz). dDeep differs by at most 16 eps(dDeep), which Adagrad turns
    into 500 times as much on E and W (lr 0.05 / sqrt(1e-8)) a step, plus
    3 * 2^-23 |p| of parameter rounding. Later losses: the twin's 1e-5."""
    from lightctr_amd.data.synthetic import SyntheticMultiHot
    from lightctr_amd.models.pnn import PNNHyper, PNNModel

    nf, K, F, B = 5, 8, 1 << 10, 64
    h = PNNHyper(num_features=F, num_fields=nf, k=K, hidden=(32, 16),
                 mlp_optimizer="adagrad", layout=layout, pooling="mean",
                 seed=11)
    hip = PNNModel(h, device=DEV, pnn_impl="hip")
    ref = PNNModel(h, device=DEV, pnn_impl="torch")
    gen = SyntheticMultiHot(num_features=F, num_fields=nf, multi=(1, 3),
                            max_multi=3, seed=2, device=DEV)
    d = nf * K
    for step in range(3):
        row_ptr, fields, fids, vals, labels = gen.batch(B)
        if step == 0:
            fl = hip._fields(fields)
            pred, _ = hip._forward_gpu(row_ptr, fids, vals, fields=fl)
            ko.check_bits("predict", hip.predict_proba(
                row_ptr, fids, vals, fields=fields),
                torch.sigmoid(pred.clamp(-16, 16)).cpu())
            score, _ = ref._forward_gpu(row_ptr, fids, vals, fields=fl)
            ones = torch.ones(B, 1, device=DEV)
            jac = ref.mlp.backward(ones).cpu()  # d score / d z, a row each
            x0 = ref._z[:, :d].float().cpu()
            dpred = (torch.sigmoid(score.clamp(-16, 16)) - labels).cpu() / B
            dz = jac * dpred[:, None]
            (zr, dr), (z64, d64) = (ref_outputs(x0, dz, nf, rounding="bf16"),
                                    pnn_autograd(x0, dz, nf))
            eps_z = float((zr.double() - z64).abs().max())
            eps_d = float((dr.double() - d64).abs().max())
            tol0 = 16 * eps_z * float(jac[:, d:].abs().sum(1).max())
            tolp = 3 * 500 * 16 * eps_d
        lh = hip.train_step(row_ptr, fids, vals, labels, fields=fields)
        lr = ref.train_step(row_ptr, fids, vals, labels, fields=fields)
        tol = tol0 + 2 * ko.U23 if step == 0 else 1e-5
        print(f"STEP {step} eps_z {eps_z:.3e} eps_d {eps_d:.3e} tol {tol:.3e} "
              f"dloss {float((lh - lr).abs().max()):.3e}")
        torch.testing.assert_close(lh, lr, rtol=0, atol=tol)
    for name in ("E", "W"):
        tol = tolp + 3 * ko.U23 * float(getattr(ref, name).abs().max())
        diff = (getattr(hip, name) - getattr(ref, name)).abs().max()
        print(f"PARAM {name} {float(diff):.3e} tol {tol:.3e}")
        torch.testing.assert_close(getattr(hip, name), getattr(ref, name),
                                   rtol=0, atol=tol,
                                   msg=lambda m: f"{name}: {m}")
    assert not torch.equal(ref.E.cpu(), PNNModel(h).E)
