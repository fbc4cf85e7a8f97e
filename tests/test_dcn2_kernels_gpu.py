"""dcn2_cross_forward / dcn2_cross_backward (ops/csrc/dcn2_kernels.hip)
against the layer-by-layer definition in float64 under autograd
(test_dcn2.dcn2_layers_autograd).

Exact set: x0 in {-1, 0, 1}; every V_l and U_l a signed partial permutation
(min(r, d) entries of +-1 in distinct rows and distinct columns, rows 0 and
d-1 and columns 0 and r-1 among them), so |T_l| <= |x_l|, |z_l| <= |x_l| + 1,
|x_l| <= 2^(l+1) - 1 and |g_l| <= 2^(L-l+1); b_l with at most 2 entries of
+-1, u with 4, dpred and the incoming dDeep in {-2..2}. The definition run on
the absolute values of the inputs bounds every term: what passes through bf16
(X, T, G, S) is asserted to stay below 2^8 and every fp32 sum below 2^24, so
all of it is integers that both formats hold in any summation order and the
comparison is bit equality, up to the sign of a zero (+ 0.0 on both sides).

Float set: randn inputs, U, V and u scaled as at init, x0, U and V holding
bf16 values; the batches of a case are the first B rows of one draw. Per
output the tolerance is 8 times the largest error, over the batches of the
case, of ops/dcn2_ref.py with rounding="bf16" run in fp32 torch on the CPU
against the float64 definition on the same inputs: the reference's own
rounding model sets the scale, 8 covers the MFMA summation order. It is
never taken from the kernels' output.
"""

import pytest
import torch

import kernel_oracles as ko
from test_dcn2 import OUTS, dcn2_layers_autograd, float_case, ref_outputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DS = (4, 8, 60, 260, 624, 1024)
RS = (16, 48, 128)
BF16_OUTS = ("X", "T", "G", "S")


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


def batch_sizes():
    t = ops().dcn2_cross_tile_rows()
    return (0, 1, 3, t + 1, 2 * t + 1)


def exact_case(B, d, r, L, seed):
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    n = min(r, d)

    def pick(total):  # n distinct of range(total), its two ends among them
        mid = torch.randperm(total - 2, generator=g)[:n - 2] + 1
        return torch.cat([torch.tensor([0, total - 1]), mid])

    def perms():
        w = torch.zeros(L, d, r)
        for l in range(L):
            cols = pick(r)[torch.randperm(n, generator=g)]
            w[l, pick(d), cols] = ri(0, 1, n) * 2 - 1
        return w

    def sparse(rows, k):  # k entries of +-1 a row; the first two at the ends
        w = torch.zeros(rows, d)
        cols = torch.randint(0, d, (rows, k), generator=g)
        cols[:, 0], cols[:, 1] = 0, d - 1
        return w.scatter_(1, cols, ri(0, 1, rows, k) * 2 - 1)

    return {"x0": ri(-1, 1, B, d), "U": perms(), "V": perms(),
            "bc": sparse(L, 2), "u": sparse(1, 4)[0], "dpred": ri(-2, 2, B),
            "dDeep": ri(-2, 2, B, d)}


def run(c, save=True):
    """the kernels' eight outputs, every one written over poisoned memory"""
    g = {k: v.to(DEV) for k, v in c.items()}
    bf = lambda t: t.contiguous().bfloat16()
    x0, Ubf, Vbf = bf(g["x0"]), bf(g["U"]), bf(g["V"])
    Utbf, Vtbf = bf(g["U"].transpose(1, 2)), bf(g["V"].transpose(1, 2))
    (B, d), (L, _, r) = c["x0"].shape, c["U"].shape
    saved = (((L, B, d), torch.bfloat16), ((L, B, r), torch.bfloat16))
    for shape, dt in (((B,), torch.float32),) + saved:
        ko.poison(shape, dt, DEV)
    fwd = ops().dcn2_cross_forward(x0, Ubf, Vtbf, g["bc"], g["u"], save)
    if not save:
        return fwd
    cross, X, T = fwd
    for shape, dt in saved + (((L, d), torch.float32), ((d,), torch.float32)):
        ko.poison(shape, dt, DEV)
    dDeep = g["dDeep"].clone()
    G, S, dbc, du = ops().dcn2_cross_backward(
        x0, X, T, Ubf, Utbf, Vbf, g["bc"], g["u"], g["dpred"], dDeep)
    return dict(zip(OUTS, (cross, X, T, dDeep, G, S, dbc, du)))


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("L", (1, 3, 4))
def test_exact(L, r, d):
    for B in batch_sizes():
        c = exact_case(B, d, r, L, seed=1000 * L + 10 * d + r + B)
        ref = dcn2_layers_autograd(c)
        mag = dcn2_layers_autograd({k: v.abs() for k, v in c.items()})
        out = run(c)
        for name in OUTS:
            lim = 2 ** 8 if name in BF16_OUTS else 2 ** 24
            assert not (mag[name] >= lim).any(), (name, B)
            dt = torch.bfloat16 if name in BF16_OUTS else torch.float32
            ko.check_bits(f"{name}[B={B}]", out[name] + 0.0,
                          (ref[name] + 0.0).to(dt))


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("r", RS)
@pytest.mark.parametrize("L", (3, 8))
def test_float_bound(L, r, d):
    sizes = batch_sizes()
    full = float_case(max(sizes), d, r, L, seed=77 * L + 10 * d + r)
    runs = []
    for B in sizes:  # the first B rows under the same parameters
        c = {k: v[:B] if k in ("x0", "dpred", "dDeep") else v
             for k, v in full.items()}
        ref, f32 = dcn2_layers_autograd(c), ref_outputs(c, rounding="bf16")
        err = {n: float((f32[n].double() - ref[n]).abs().max())
               for n in OUTS if ref[n].numel()}
        runs.append((B, ref, err, run(c)))
    for name in OUTS:
        tol = 8 * max(err.get(name, 0.0) for _, _, err, _ in runs)
        print(f"TOL {name} d={d} r={r} L={L} {tol:.3e}")
        for B, ref, _, out in runs:
            if B == 0 and name in ("dbc", "du"):
                assert not out[name].any(), name  # empty batch: zeros
            elif ref[name].numel():
                ko.check_bound(f"{name}[B={B}]", out[name], ref[name],
                               torch.full_like(ref[name], tol))


def test_deterministic_and_save_off():
    c = float_case(3 * ops().dcn2_cross_tile_rows() + 5, 624, 64, 3, seed=5)
    a, b = run(c), run(c)
    for name in OUTS:
        ko.check_bits(name, a[name], b[name].cpu())
    assert a["dbc"].any() and a["du"].any() and a["S"].any()
    (cross,) = run(c, save=False)
    ko.check_bits("cross, save off", cross, a["cross"].cpu())


def _zeros(L=3, d=8, r=16, B=4):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    bf = torch.bfloat16
    return dict(x0=z(B, d, dt=bf), X=z(L, B, d, dt=bf), T=z(L, B, r, dt=bf),
                Ubf=z(L, d, r, dt=bf), Utbf=z(L, r, d, dt=bf),
                Vbf=z(L, d, r, dt=bf), bc=z(L, d), u=z(d), dpred=z(B),
                dDeep=z(B, d))


BAD = {"r % 16": dict(r=24), "r > 128": dict(r=144),
       "d % 4": dict(d=6), "d > 1024": dict(d=1028), "L = 0": dict(L=0),
       "L = 9": dict(L=9),
       "Ubf dtype": dict(Ubf=lambda a: a["Ubf"].float()),
       "x0 dtype": dict(x0=lambda a: a["x0"].float()),
       "bc dtype": dict(bc=lambda a: a["bc"].double()),
       "x0 width": dict(x0=lambda a: a["x0"][:, :4].contiguous()),
       "u length": dict(u=lambda a: a["u"][:4].contiguous()),
       "mirror shape": dict(Utbf=lambda a: a["Ubf"], Vtbf=lambda a: a["Ubf"])}


@pytest.mark.parametrize("what", list(BAD))
def test_argument_errors(what):
    a = _zeros(**{k: v for k, v in BAD[what].items() if isinstance(v, int)})
    a["Vtbf"] = a["Utbf"]
    a.update({k: v(a) for k, v in BAD[what].items() if callable(v)})
    with pytest.raises(RuntimeError):
        ops().dcn2_cross_forward(a["x0"], a["Ubf"], a["Vtbf"], a["bc"],
                                 a["u"], True)
    with pytest.raises(RuntimeError):
        ops().dcn2_cross_backward(*(a[n] for n in (
            "x0", "X", "T", "Ubf", "Utbf", "Vbf", "bc", "u", "dpred",
            "dDeep")))


def test_limits_name_the_figures():
    """Every shape in the served range fits the device's LDS, so the LDS
    message (which names the bytes) cannot be raised here; the range messages
    name the figure they refuse."""
    from lightctr_amd.models.dcn2 import DCNv2Hyper, DCNv2Model

    o = ops()
    assert o.dcn2_cross_lds_bytes(8, 1024, 128) <= o.ffm_max_lds_per_block()
    assert o.dcn2_cross_lds_bytes(8, 1024, 128) > \
        o.dcn2_cross_lds_bytes(1, 4, 16) > 0
    a = _zeros(d=1028)
    with pytest.raises(RuntimeError, match=r"in \[4, 1024\], got 1028"):
        o.dcn2_cross_forward(a["x0"], a["Ubf"], a["Utbf"], a["bc"], a["u"],
                             False)
    a = _zeros(r=144)
    with pytest.raises(RuntimeError, match=r"in \[16, 128\], got 144"):
        o.dcn2_cross_forward(a["x0"], a["Ubf"], a["Utbf"], a["bc"], a["u"],
                             False)
    with pytest.raises(ValueError, match="4..1024, got 1028"):
        DCNv2Model(DCNv2Hyper(num_features=64, num_fields=257, k=4),
                   device=DEV)


@pytest.mark.parametrize("layout", ("position", "field"))
def test_model_hip_against_torch(layout):
    """Three steps of the two arms from one seed; both read the same bf16
    mirrors of U and V and round at the same points. Step 0 starts from equal
    parameters, so the losses differ by the cross terms only: each arm is
    within 8 eps of the float64 definition, eps being the error of the
    bf16-rounded reference (fp32, CPU) on the model's own concat and
    parameters, and the loss moves by at most the score's change. Later the
    arms' parameters differ, as in DCN's twin test: Adagrad turns a gradient
    difference e into at most e lr / sqrt(eps) = 500 e for E (10 e for the
    dense ones). Beside fp32 summation order (1e-9 here, as in DCN) the arms
    can differ where their two fp32 values straddle a bf16 boundary at a
    rounding point: one bf16 ulp, 2^-8, of that element. The concat entries
    are of the order of init_sigma = 0.01 and dpred is at most 1/B = 0.016
    a row, so g is at most 0.016 |u_c| = 2.5e-3, T and z are near 0.01, and
    G and S are near 4e-5: a flipped T moves one dx0 entry by 2^-8 0.01 |U|
    g = 2.5e-8 and a flipped G or S by 2^-8 4e-5 |V| = 2.5e-8 as well, which
    Adagrad carries to 1.2e-5 on one entry of E at the very most, were that
    entry's gradient zero otherwise; with its own gradient of the same size
    beside it the factor is below 500 / 2, inside the 1e-5 that the FM, FwFM
    and DCN twins use for the same chain."""
    from lightctr_amd.data.synthetic import SyntheticMultiHot
    from lightctr_amd.models.dcn2 import DCNv2Hyper, DCNv2Model

    nf, K, F, B = 5, 8, 1 << 10, 64
    h = DCNv2Hyper(num_features=F, num_fields=nf, k=K, hidden=(32, 16),
                   mlp_optimizer="adagrad", cross_layers=3, cross_rank=16,
                   layout=layout, pooling="mean", seed=11)
    hip = DCNv2Model(h, device=DEV, cross_impl="hip")
    ref = DCNv2Model(h, device=DEV, cross_impl="torch")
    gen = SyntheticMultiHot(num_features=F, num_fields=nf, multi=(1, 3),
                            max_multi=3, seed=2, device=DEV)
    for step in range(3):
        row_ptr, fields, fids, vals, labels = gen.batch(B)
        if step == 0:
            ref._forward_gpu(row_ptr, fids, vals, train=False,
                             fields=ref._fields(fields))
            c = {"x0": ref._saved[0].cpu(), "U": ref.Ubf.float().cpu(),
                 "V": ref.Vbf.float().cpu(), "bc": ref.bc.cpu(),
                 "u": ref.u.cpu(), "dpred": torch.zeros(B),
                 "dDeep": torch.zeros(B, nf * K)}
            eps = float((ref_outputs(c, rounding="bf16")["cross"].double()
                         - dcn2_layers_autograd(c)["cross"]).abs().max())
        lh = hip.train_step(row_ptr, fids, vals, labels, fields=fields)
        lr = ref.train_step(row_ptr, fids, vals, labels, fields=fields)
        tol = 16 * eps + 2 * ko.U23 if step == 0 else 1e-5
        print(f"STEP {step} eps {eps:.3e} "
              f"dloss {float((lh - lr).abs().max()):.3e}")
        torch.testing.assert_close(lh, lr, rtol=0, atol=tol)
    for name in ("U", "V", "bc", "u", "E", "W"):
        diff = (getattr(hip, name) - getattr(ref, name)).abs().max()
        print(f"PARAM {name} {float(diff):.3e}")
        torch.testing.assert_close(getattr(hip, name), getattr(ref, name),
                                   rtol=0, atol=1e-5,
                                   msg=lambda m: f"{name}: {m}")
    assert ref.bc.any() and not torch.equal(ref.u.cpu(), DCNv2Model(h).u)
    assert torch.equal(hip.Utbf, hip.U.transpose(1, 2).bfloat16())
