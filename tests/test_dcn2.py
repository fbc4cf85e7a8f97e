"""DCN-v2 on the CPU: ops/dcn2_ref.py against the definition in float64 under
autograd, and DCNv2Model's train step, bundled-data run, checkpoint and CLI
predict. ``dcn2_layers_autograd`` is also the reference of
test_dcn2_kernels_gpu.py."""

import os

import pytest
import torch

from lightctr_amd.models.dcn2 import DCNv2Hyper, DCNv2Model, DCNv2Trainer
from lightctr_amd.ops import dcn2_ref

DATA = os.path.join(os.path.dirname(__file__), "..", "data")
OUTS = ("cross", "X", "T", "dDeep", "G", "S", "dbc", "du")


def dcn2_layers_autograd(c, dtype=torch.float64):
    """The definition T_l = x_l V_l, z_l = T_l U_l^T + b_l, x_{l+1} = x0 z_l
    + x_l, cross = x_L . u, layer by layer in `dtype`; its gradients by
    autograd with dpred as the upstream gradient. G_l and S_l are the
    gradients at z_l and T_l, X holds x_1 .. x_L, dDeep is the incoming one
    plus dx0. dU and dV come with them for the CPU test."""
    x0, U, V, bc, u = (c[n].to(dtype).clone().requires_grad_()
                       for n in ("x0", "U", "V", "bc", "u"))
    L = U.shape[0]
    x, X, T, Z = x0, [], [], []
    for l in range(L):
        T.append(x @ V[l])
        Z.append(T[l] @ U[l].t() + bc[l])
        x = x0 * Z[l] + x
        X.append(x)
    cross = x @ u
    gr = torch.autograd.grad(cross, (x0, U, V, bc, u, *Z, *T),
                             c["dpred"].to(dtype))
    dx0, dU, dV, dbc, du = gr[:5]
    st = lambda ts: torch.stack([t.detach() for t in ts])
    out = dict(zip(OUTS, (cross.detach(), st(X), st(T),
                          c["dDeep"].to(dtype) + dx0, st(gr[5:5 + L]),
                          st(gr[5 + L:]), dbc, du)))
    out.update(dU=dU, dV=dV)
    return out


def float_case(B, d, r, L, seed):
    """randn inputs, U, V and u scaled as at init; x0, U and V hold bf16
    values, which is what the kernels are given"""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    bf = lambda t: t.bfloat16().float()
    return {"x0": bf(rn(B, d)), "U": bf(rn(L, d, r) / r ** 0.5),
            "V": bf(rn(L, d, r) / d ** 0.5), "bc": rn(L, d),
            "u": rn(d) / d ** 0.5, "dpred": rn(B), "dDeep": rn(B, d)}


def ref_outputs(c, rounding=None):
    """ops/dcn2_ref.py on a case, in the dtype of the case"""
    cross, X, T = dcn2_ref.dcn2_cross_forward_ref(
        c["x0"], c["U"], c["V"], c["bc"], c["u"], rounding)
    dx0, G, S, dU, dV, dbc, du = dcn2_ref.dcn2_cross_backward_ref(
        c["x0"], X, T, c["U"], c["V"], c["bc"], c["u"], c["dpred"], rounding)
    out = dict(zip(OUTS, (cross, X, T, c["dDeep"] + dx0, G, S, dbc, du)))
    out.update(dU=dU, dV=dV)
    return out


@pytest.mark.parametrize("d", (4, 60))
@pytest.mark.parametrize("r", (16, 48))
@pytest.mark.parametrize("L", (1, 3, 8))
def test_ref_matches_definition(L, r, d):
    c = {k: v.double()
         for k, v in float_case(9, d, r, L, seed=100 * L + r + d).items()}
    ref, got = dcn2_layers_autograd(c), ref_outputs(c)
    for name, want in ref.items():
        torch.testing.assert_close(got[name], want, rtol=1e-10, atol=1e-10,
                                   msg=lambda m: f"{name}: {m}")
    with pytest.raises(ValueError, match="rounding"):
        ref_outputs(c, rounding="fp16")


def test_model_step_data_checkpoint_and_cli(tmp_path, capsys):
    from lightctr_amd import cli
    from lightctr_amd.data.libffm import load_libffm

    path = os.path.join(DATA, "train_sparse.csv")
    ds = load_libffm(path)
    h = DCNv2Hyper(num_features=ds.num_features, num_fields=ds.num_fields,
                   k=4, cross_layers=2, cross_rank=16, layout="field",
                   pooling="mean")
    tr = DCNv2Trainer(ds, h, batch_size=128, epochs=3)
    m = tr.model
    names = ("U", "V", "bc", "u", "E")
    before = [getattr(m, n).clone() for n in names] + \
        [m.mlp.layers[0].W.clone()]
    b = ds.slice_rows(0, 128)
    m.train_step(b.row_ptr, b.fids, b.vals, b.labels, fields=b.fields)
    after = [getattr(m, n) for n in names] + [m.mlp.layers[0].W]
    for n, x, y in zip(names + ("mlp",), before, after):
        assert not torch.equal(x, y), n
    losses = []
    tr.train(log=lambda s: losses.append(float(s.split("=")[1])))
    assert losses[-1] < losses[0] - 0.05, losses
    m.save(tmp_path / "m.pt")
    m2 = DCNv2Model(h)
    m2.load(str(tmp_path / "m.pt"))
    for n in m._cross_state() + ["W", "E", "nE"]:
        assert torch.equal(getattr(m, n), getattr(m2, n)), n
    assert m2.cross_step == m.cross_step > 0
    want = m.predict_proba(b.row_ptr, b.fids, b.vals, fields=b.fields)
    torch.testing.assert_close(
        m2.predict_proba(b.row_ptr, b.fids, b.vals, fields=b.fields), want,
        rtol=0, atol=0)
    # predict takes depth 2 and rank 16 from the checkpoint, not the flags
    dump = tmp_path / "scores.txt"
    assert cli.main(["predict", "--model", "dcn2", "--data", path, "--k", "4",
                     "--features", str(ds.num_features),
                     "--load", str(tmp_path / "m.pt"), "--device", "cpu",
                     "--cross-layers", "5", "--cross-rank", "32",
                     "--dump", str(dump)]) == 0
    capsys.readouterr()
    scores = torch.tensor([float(s) for s in dump.read_text().split()])
    torch.testing.assert_close(scores[:128], want, rtol=0, atol=2e-6)
    for bad in (dict(cross_layers=9), dict(cross_rank=24),
                dict(cross_rank=144), dict(k=64, num_fields=17)):
        kw = dict(num_features=8, num_fields=2, k=4)
        kw.update(bad)
        with pytest.raises(ValueError, match="cross_|num_fields"):
            DCNv2Model(DCNv2Hyper(**kw))
