"""dcn_cross_prep / dcn_cross_forward / dcn_cross_backward
(ops/csrc/dcn_kernels.hip) against the layer-by-layer definition in float64
under autograd (test_dcn.layers_autograd), never the closed form.

Exact set: x0 in {-1, 0, 1}, w_l and u with at most 4 entries of +-1 (columns
0 and d-1 always among them), b_l with at most 2, dpred and the incoming
dDeep in {-2..2}. The same definition run on the absolute values of the
inputs gives, per output, the sum of the absolute values of its terms; it is
asserted to stay below 2^24, so every quantity is an integer that fp32 holds
in any summation order and the comparison is bit equality.

Float set: randn inputs, w and u scaled by 1/sqrt(d); the batches of a case
are the first B rows of one draw under the same parameters. Per output (cross,
P, dDeep, dWc, dbc, du) the tolerance is 8 times the largest error of the same
definition run in fp32 torch on the CPU against float64, on the same inputs,
over the batches of the case (8 covers the closed form's other operation
order and the dots' summation order). The largest error and not each
element's or each batch's own: one fp32 result is now and then right to a
hundredth of an ulp (seen at B = 1: 7.7e-8 on a cross term near 100), which
no fp32 code can be held to.
"""

import pytest
import torch

import kernel_oracles as ko
from test_dcn import OUTS, float_case, layers_autograd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DS = (4, 8, 60, 256, 260, 624, 2496)


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def batch_sizes():
    return (0, 1, 3, 257, ops().dcn_cross_backward_rows() + 1)


def exact_case(B, d, L, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()

    def sparse(rows, n):  # n entries of +-1 a row; the first two at the ends
        w = torch.zeros(rows, d)
        cols = torch.randint(0, d, (rows, n), generator=g)
        cols[:, 0], cols[:, 1] = 0, d - 1
        return w.scatter_(1, cols, ri(0, 1, rows, n) * 2 - 1)

    return {"x0": ri(-1, 1, B, d), "Wc": sparse(L, 4), "bc": sparse(L, 2),
            "u": sparse(1, 4)[0], "dpred": ri(-2, 2, B),
            "dDeep": ri(-2, 2, B, d)}


def run(c):
    """the kernels' six outputs, every one written over poisoned memory"""
    g = {k: v.to(DEV) for k, v in c.items()}
    x0 = g["x0"].bfloat16()
    B, d = c["x0"].shape
    L = c["Wc"].shape[0]
    C, q = ops().dcn_cross_prep(g["Wc"], g["bc"], g["u"])
    for shape in ((B,), (B, L + 1)):
        ko.poison(shape, torch.float32, DEV)
    cross, P = ops().dcn_cross_forward(x0, g["Wc"], g["u"], q)
    for shape in ((L, d), (L, d), (d,)):
        ko.poison(shape, torch.float32, DEV)
    dDeep = g["dDeep"].clone()
    dWc, dbc, du = ops().dcn_cross_backward(x0, P, g["Wc"], g["u"], q, C,
                                            g["dpred"], dDeep)
    return dict(zip(OUTS, (cross, P, dDeep, dWc, dbc, du)))


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("L", (1, 2, 3, 4))
def test_exact(L, d):
    for B in batch_sizes():
        c = exact_case(B, d, L, seed=1000 * L + d + B)
        ref = layers_autograd(c)
        mag = layers_autograd({k: v.abs() for k, v in c.items()})
        out = run(c)
        for name in OUTS:
            assert not (mag[name] >= 2 ** 24).any(), (name, B)
            # + 0.0: the kernels' sums start from +0 and never end in -0
            ko.check_bits(f"{name}[B={B}]", out[name],
                          (ref[name] + 0.0).float())


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("L", (3, 6, 8))
def test_float_bound(L, d):
    sizes = batch_sizes()
    full = float_case(max(sizes), d, L, seed=77 * L + d)
    runs = []
    for B in sizes:  # the first B rows under the same parameters
        c = {k: v[:B] if k in ("x0", "dpred", "dDeep") else v
             for k, v in full.items()}
        ref, f32 = layers_autograd(c), layers_autograd(c, torch.float32)
        err = {n: float((f32[n].double() - ref[n]).abs().max())
               for n in OUTS if ref[n].numel()}
        runs.append((B, ref, err, run(c)))
    for name in OUTS:
        tol = 8 * max(err.get(name, 0.0) for _, _, err, _ in runs)
        for B, ref, _, out in runs:
            if B == 0 and name in ("dWc", "dbc", "du"):
                assert not out[name].any(), name  # empty batch: zeros
            elif ref[name].numel():
                ko.check_bound(f"{name}[B={B}]", out[name], ref[name],
                               torch.full_like(ref[name], tol))


def test_backward_is_deterministic():
    c = float_case(3 * ops().dcn_cross_backward_rows() + 5, 624, 3, seed=5)
    a, b = run(c), run(c)
    for name in OUTS:
        ko.check_bits(name, a[name], b[name].cpu())
    assert a["dWc"].any() and a["dbc"].any()


BAD = {"L = 0": dict(Wc=torch.zeros(0, 8), bc=torch.zeros(0, 8)),
       "L = 9": dict(Wc=torch.zeros(9, 8), bc=torch.zeros(9, 8)),
       "Wc dtype": dict(Wc=torch.zeros(3, 8, dtype=torch.float64)),
       "u length": dict(u=torch.zeros(12)),
       "x0 dtype": dict(x0=torch.zeros(4, 8)),
       "x0 width": dict(x0=torch.zeros(4, 12).bfloat16()),
       "d % 4": dict(Wc=torch.zeros(3, 6), u=torch.zeros(6),
                     x0=torch.zeros(4, 6).bfloat16())}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(what):
    c = float_case(4, 8, 3, seed=1)
    c["x0"] = c["x0"].bfloat16()
    c.update(BAD[what])
    g = {k: v.to(DEV) for k, v in c.items()}
    L = c["Wc"].shape[0]
    q, C = torch.zeros(L + 1, device=DEV), torch.zeros(L + 1, 8, device=DEV)
    if "x0" not in BAD[what]:
        with pytest.raises(RuntimeError):
            ops().dcn_cross_prep(g["Wc"], g["bc"], g["u"])
    with pytest.raises(RuntimeError):
        ops().dcn_cross_forward(g["x0"], g["Wc"], g["u"], q)
    with pytest.raises(RuntimeError):
        ops().dcn_cross_backward(g["x0"], torch.zeros(4, L + 1, device=DEV),
                                 g["Wc"], g["u"], q, C, g["dpred"],
                                 g["dDeep"])


def test_lds_limit_names_the_bytes():
    from lightctr_amd.models.dcn import DCNHyper, DCNModel

    o = ops()
    have = o.ffm_max_lds_per_block()
    assert o.dcn_cross_lds_bytes(8, 2496) <= have
    d = have // (9 * 4) // 4 * 4 + 4        # first d past the limit at L = 8
    z = lambda *s: torch.zeros(*s, device=DEV)
    msg = f"needs {o.dcn_cross_lds_bytes(8, d)} bytes of LDS per block, " \
          f"the device gives {have}"
    with pytest.raises(RuntimeError, match=msg):
        o.dcn_cross_forward(z(2, d).bfloat16(), z(8, d), z(d), z(9))
    with pytest.raises(ValueError, match="bytes of LDS"):
        DCNModel(DCNHyper(num_features=64, num_fields=d // 4, k=4,
                          cross_layers=8), device=DEV)


@pytest.mark.parametrize("layout", ("position", "field"))
def test_model_hip_against_torch(layout):
    """Three steps of the two arms from one seed. Step 0 starts from equal
    parameters, so the losses differ by the cross terms only: each arm is
    within 8 eps of the float64 definition (eps: the fp32 error above, on the
    model's own concat and parameters), and the loss moves by at most the
    score's change. Later the arms' parameters differ: Adagrad turns a
    gradient difference e into at most e lr / sqrt(eps) = 500 e for E (10 e
    for the dense ones), and gradients are dpred (= 1/B a row) times
    activations of order 1, so 16 eps of score gives parameters equal to
    about 500 * 16 eps / 4; eps is near 1e-9 here, and 1e-5 is the atol of
    the FM and FwFM twins for the same chain."""
    from lightctr_amd.data.synthetic import SyntheticMultiHot
    from lightctr_amd.models.dcn import DCNHyper, DCNModel

    nf, K, F, B = 5, 8, 1 << 10, 64
    h = DCNHyper(num_features=F, num_fields=nf, k=K, hidden=(32, 16),
                 mlp_optimizer="adagrad", cross_layers=3, layout=layout,
                 pooling="mean", seed=11)
    hip = DCNModel(h, device=DEV, cross_impl="hip")
    ref = DCNModel(h, device=DEV, cross_impl="torch")
    gen = SyntheticMultiHot(num_features=F, num_fields=nf, multi=(1, 3),
                            max_multi=3, seed=2, device=DEV)
    for step in range(3):
        row_ptr, fields, fids, vals, labels = gen.batch(B)
        if step == 0:
            ref._forward_gpu(row_ptr, fids, vals, train=False,
                             fields=ref._fields(fields))
            c = {"x0": ref._saved[0].cpu(), "Wc": ref.Wc.cpu(),
                 "bc": ref.bc.cpu(), "u": ref.u.cpu(),
                 "dpred": torch.zeros(B), "dDeep": torch.zeros(B, nf * K)}
            eps = float((layers_autograd(c, torch.float32)["cross"].double()
                         - layers_autograd(c)["cross"]).abs().max())
        lh = hip.train_step(row_ptr, fids, vals, labels, fields=fields)
        lr = ref.train_step(row_ptr, fids, vals, labels, fields=fields)
        tol = 16 * eps + 2 * ko.U23 if step == 0 else 1e-5
        torch.testing.assert_close(lh, lr, rtol=0, atol=tol)
    for name in ("Wc", "bc", "u", "E", "W"):
        torch.testing.assert_close(getattr(hip, name), getattr(ref, name),
                                   rtol=0, atol=1e-5,
                                   msg=lambda m: f"{name}: {m}")
    assert ref.bc.any() and not torch.equal(ref.u.cpu(), DCNModel(h).u)
