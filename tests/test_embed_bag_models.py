"""Wide&Deep and DeepFM with the concat addressed by field (layout="field"),
on the CPU path: equality with layout="position" where the two coincide,
invariance under the order of a row's tokens, three training steps against a
float64 replay of the definition under autograd, the fields=None error, the
checkpoint and the CLI."""

import pytest
import torch

from lightctr_amd.data import LibffmDataset, load_libffm
from lightctr_amd.data.synthetic import SyntheticCriteo, SyntheticMultiHot
from lightctr_amd.models.deepfm import DeepFMHyper, DeepFMModel
from lightctr_amd.models.wide_deep import WideDeepHyper, WideDeepModel

MODELS = {"widedeep": (WideDeepHyper, WideDeepModel),
          "deepfm": (DeepFMHyper, DeepFMModel)}
F, NF, K = 512, 5, 8


def make(name, **kw):
    H, M = MODELS[name]
    base = dict(num_features=F, num_fields=NF, k=K, hidden=(16, 8),
                init_sigma=0.1, lr=0.05)
    base.update(kw)
    return M(H(**base), device="cpu")


def multihot(seed, rows=9):
    return SyntheticMultiHot(num_features=F, num_fields=NF, multi=(1, 3),
                             max_multi=4, p_missing=0.3,
                             seed=seed).batch(rows)


def _tensors(m):
    out = {n: getattr(m, n) for n in ("W", "E", "nW", "nE")}
    for i, la in enumerate(m.mlp.layers):
        out[f"mlp{i}.W"], out[f"mlp{i}.b"] = la.W, la.b
    return out


@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("name", list(MODELS))
def test_field_equals_position_on_in_order_rows(name, pooling):
    """one entry per field, in order: both layouts and both poolings are the
    same computation; losses and every parameter are equal after 3 steps"""
    gen = SyntheticCriteo(num_features=F, num_fields=NF, seed=3)
    a = make(name)
    b = make(name, layout="field", pooling=pooling)
    for _ in range(3):
        rp, fl, fi, v, lb = gen.batch(32)
        la = a.train_step(rp, fi, v, lb)
        lb_ = b.train_step(rp, fi, v, lb, fields=fl)
        assert torch.equal(la, lb_)
    ta, tb = _tensors(a), _tensors(b)
    for n in ta:
        assert torch.equal(ta[n], tb[n]), n
    assert float(a.nE.abs().max()) > 0


@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("name", list(MODELS))
def test_prediction_ignores_token_order(name, pooling):
    """shuffling the tokens inside every row moves the prediction by fp32
    summation order only (bound: every sum of the score has at most
    n = NF*K + 16 + 8 + row length terms of magnitude <= 1, n 2^-23 each
    way); the position layout moves by far more on the same rows"""
    rp, fl, fi, v, _ = multihot(7)
    g = torch.Generator().manual_seed(1)
    perm = torch.cat([int(rp[r]) + torch.randperm(int(rp[r + 1] - rp[r]),
                                                  generator=g)
                      for r in range(rp.numel() - 1)])
    m = make(name, layout="field", pooling=pooling)
    m.W.copy_(torch.randn(F, generator=g) * 0.1)
    p = m.predict_proba(rp, fi, v, fields=fl)
    q = m.predict_proba(rp, fi[perm], v[perm], fields=fl[perm])
    n = NF * K + 16 + 8 + int((rp[1:] - rp[:-1]).max())
    assert float((p - q).abs().max()) <= 2 * n * 2.0 ** -23
    pos = make(name)
    pos.W.copy_(m.W)
    p0 = pos.predict_proba(rp, fi, v)
    q0 = pos.predict_proba(rp, fi[perm], v[perm])
    assert float((p0 - q0).abs().max()) > 1e-4


def _replay64(m, name, batches, pooling):
    """Three steps of the model's definition in float64: the forward of the
    field layout under autograd for every gradient, then sparse Adagrad on
    the touched rows of W and E and the MLP's dense Adagrad. Returns the
    losses and the final parameters."""
    dd = torch.float64
    W = m.W.double().clone()
    E = m.E.double().clone()
    nW, nE = torch.zeros_like(W), torch.zeros_like(E)
    layers = [(la.W.double().clone(), la.b.double().clone())
              for la in m.mlp.layers]
    ns = [(torch.zeros_like(w), torch.zeros_like(b)) for w, b in layers]
    h = m.h
    losses = []
    for rp, fl, fi, v, lb in batches:
        B = rp.numel() - 1
        params = [W.requires_grad_(True), E.requires_grad_(True)]
        for w, b in layers:
            params += [w.requires_grad_(True), b.requires_grad_(True)]
        rl = rp.long()
        row = torch.repeat_interleave(torch.arange(B), rl[1:] - rl[:-1])
        f, x, c = fi.long(), v.double(), fl.long()
        vx = E[f] * x.unsqueeze(1)
        keep = (c >= 0) & (c < NF)
        slot = (row * NF + c)[keep]
        S = torch.zeros(B * NF, K, dtype=dd).index_add(0, slot, vx[keep])
        if pooling == "mean":
            cnt = torch.zeros(B * NF, dtype=dd).index_add(
                0, slot, torch.ones(slot.numel(), dtype=dd))
            S = S / cnt.clamp(min=1).unsqueeze(1)
        y = S.view(B, NF * K)
        for i, (w, b) in enumerate(layers):
            y = y @ w.t() + b
            if i < len(layers) - 1:
                y = torch.relu(y)
        score = torch.zeros(B, dtype=dd).index_add(0, row, W[f] * x) \
            + y[:, 0]
        if name == "deepfm":
            s = torch.zeros(B, K, dtype=dd).index_add(0, row, vx)
            q = torch.zeros(B, K, dtype=dd).index_add(0, row, vx * vx)
            score = score + 0.5 * (s * s - q).sum(1)
        y01 = lb.double()
        loss = torch.clamp(score, min=0) - score * y01 \
            + torch.log1p(torch.exp(-score.abs()))
        grads = torch.autograd.grad(loss.sum() / B, params)
        losses.append(loss.detach())
        with torch.no_grad():
            u = torch.unique(f)
            for p, n, g in ((W, nW, grads[0]), (E, nE, grads[1])):
                gu = g[u] + h.l2 * p[u]
                n[u] += gu * gu
                p[u] -= h.lr * gu / torch.sqrt(n[u] + h.eps)
            for i, la in enumerate(m.mlp.layers):
                for j, l2 in ((0, la.l2), (1, 0.0)):
                    p, n = layers[i][j], ns[i][j]
                    g = grads[2 + 2 * i + j] + l2 * p
                    n += g * g
                    p -= la.lr * g / (n + la.eps).sqrt()
        W, E = W.detach(), E.detach()
        layers = [(w.detach(), b.detach()) for w, b in layers]
    out = {"W": W, "E": E}
    for i, (w, b) in enumerate(layers):
        out[f"mlp{i}.W"], out[f"mlp{i}.b"] = w, b
    return losses, out


@pytest.mark.parametrize("pooling", ["sum", "mean"])
@pytest.mark.parametrize("name", list(MODELS))
def test_three_steps_match_float64_replay(name, pooling):
    """Multi-hot rows with missing fields. Bound from the operation count:
    the longest accumulation chains between the inputs and a gradient are the
    slot sum (<= 4 terms), the row sums (<= 11), the three GEMMs (NF*K = 40,
    16, 8 terms) and their transposes on the way back, the batch sums of the
    weight gradients (9): n = 2 (4 + 11 + 40 + 16 + 8) + 9 = 167 roundings of
    2^-24 relative to magnitudes <= 1 (init_sigma = 0.1, |x| = 1, scores of
    order one), so 167 2^-24 = 1e-5 per step on a loss or gradient; Adagrad
    with eps = 1 has |d step / d g| <= lr <= 1, so the parameters inherit at
    most the gradient's error per step, and three steps compound to at most
    3 * 2 * 1e-5 = 6e-5 (each step's error enters the next once through
    the forward and once through the backward). eps = 1 on both sides keeps
    the update well conditioned; at the default 1e-8 the first Adagrad step
    is lr sign(g), whose slope lr / sqrt(eps) would multiply the bound by
    1e4."""
    tol = 3 * 2 * 167 * 2.0 ** -24
    batches = [multihot(40 + i) for i in range(3)]
    assert any(((b[1] < 0) | (b[1] >= NF)).sum() == 0 for b in batches)
    lens = torch.cat([b[0][1:] - b[0][:-1] for b in batches])
    assert int(lens.max()) <= 11 and int(lens.min()) < NF
    m = make(name, layout="field", pooling=pooling, eps=1.0,
             mlp_optimizer="adagrad")
    for la in m.mlp.layers:
        la.eps = 1.0
    g = torch.Generator().manual_seed(9)
    m.W.copy_(torch.randn(F, generator=g) * 0.1)
    want_losses, want = _replay64(m, name, batches, pooling)
    for (rp, fl, fi, v, lb), wl in zip(batches, want_losses):
        loss = m.train_step(rp, fi, v, lb, fields=fl)
        err = float((loss.double() - wl).abs().max())
        print(f"REPLAY {name} {pooling} loss err {err:.3g} tol {tol:.3g}")
        assert err <= tol
    got = _tensors(m)
    moved = 0.0
    for n, w in want.items():
        err = float((got[n].double() - w).abs().max())
        print(f"REPLAY {name} {pooling} {n} err {err:.3g}")
        assert err <= tol, n
    moved = float((m.E.double() - want["E"]).abs().max())
    assert float(m.nE.abs().max()) > 0 and moved <= tol


@pytest.mark.parametrize("name", list(MODELS))
def test_fields_none_raises(name):
    rp, fl, fi, v, lb = multihot(1)
    m = make(name, layout="field")
    with pytest.raises(ValueError, match="fields"):
        m.train_step(rp, fi, v, lb)
    with pytest.raises(ValueError, match="fields"):
        m.predict_proba(rp, fi, v)
    with pytest.raises(ValueError, match="layout"):
        make(name, layout="slot")
    with pytest.raises(ValueError, match="pooling"):
        make(name, layout="field", pooling="max")
    # position layout: fields is accepted and ignored
    p = make(name)
    assert torch.equal(p.predict_proba(rp, fi, v, fields=fl),
                       p.predict_proba(rp, fi, v))


@pytest.mark.parametrize("name", list(MODELS))
def test_checkpoint_keeps_layout_and_pooling(tmp_path, name):
    rp, fl, fi, v, lb = multihot(2)
    a = make(name, layout="field", pooling="mean")
    a.train_step(rp, fi, v, lb, fields=fl)
    path = str(tmp_path / "m.pt")
    a.save(path)
    d = torch.load(path, map_location="cpu", weights_only=True)
    assert d["hyper"]["layout"] == "field"
    assert d["hyper"]["pooling"] == "mean"
    H, M = MODELS[name]
    hyper = dict(d["hyper"])
    hyper["hidden"] = tuple(hyper["hidden"])
    b = M(H(**hyper), device="cpu")
    b.load(path)
    assert torch.equal(a.predict_proba(rp, fi, v, fields=fl),
                       b.predict_proba(rp, fi, v, fields=fl))


def test_generator_rows():
    """missing fields, multi-valued fields, shuffled order, a libffm file
    that reads back"""
    gen = SyntheticMultiHot(num_features=F, num_fields=NF, multi=(1, 3),
                            max_multi=4, p_missing=0.3, seed=5)
    rp, fl, fi, v, lb = gen.batch(200)
    assert rp.dtype == fl.dtype == fi.dtype == torch.int32
    assert int(fl.min()) >= 0 and int(fl.max()) < NF
    assert int(fi.min()) >= 0 and int(fi.max()) < F
    lens = (rp[1:] - rp[:-1]).tolist()
    per = [fl[rp[r]:rp[r + 1]].tolist() for r in range(200)]
    assert any(len(set(p)) < NF for p in per)            # a field missing
    assert any(p.count(1) > 1 for p in per)              # multi-valued
    assert all(p.count(0) <= 1 and p.count(2) <= 1 for p in per)
    assert max(p.count(3) for p in per) <= 4
    assert any(p != sorted(p) for p in per)              # shuffled
    assert set(lb.tolist()) == {0.0, 1.0} and sum(lens) == fi.numel()


def test_cli_field_layout_roundtrip(tmp_path):
    """cli train --model deepfm --layout field --pooling mean, then predict
    (layout and pooling come from the checkpoint), on a 64-row file written
    by the generator"""
    from lightctr_amd.cli import main

    data = str(tmp_path / "multihot.ffm")
    SyntheticMultiHot(num_features=F, num_fields=NF, multi=(1, 3),
                      max_multi=4, p_missing=0.3, seed=8).write_libffm(data,
                                                                       64)
    ds = load_libffm(data)
    assert isinstance(ds, LibffmDataset) and ds.num_rows == 64
    model_path = str(tmp_path / "deepfm.pt")
    dump_path = str(tmp_path / "deepfm.scores")
    rc = main(["train", "--model", "deepfm", "--data", data, "--features",
               str(F), "--k", "8", "--epochs", "1", "--batch", "32",
               "--device", "cpu", "--layout", "field", "--pooling", "mean",
               "--save", model_path])
    assert rc == 0
    hyper = torch.load(model_path, map_location="cpu",
                       weights_only=True)["hyper"]
    assert hyper["layout"] == "field" and hyper["pooling"] == "mean"
    rc = main(["predict", "--model", "deepfm", "--data", data, "--features",
               str(F), "--k", "8", "--device", "cpu", "--load", model_path,
               "--dump", dump_path])
    assert rc == 0
    with open(dump_path) as f:
        scores = [float(s) for s in f.read().split()]
    assert len(scores) == 64 and all(0.0 <= s <= 1.0 for s in scores)
    # a file in which no row carries the last field: num_fields comes from
    # the checkpoint, not from the data
    short = str(tmp_path / "short.ffm")
    with open(data) as f, open(short, "w") as out:
        for line in f:
            toks = line.split()
            out.write(" ".join([toks[0]] + [t for t in toks[1:] if
                                            int(t.split(":")[0]) < NF - 1])
                      + "\n")
    assert load_libffm(short).num_fields < NF
    rc = main(["predict", "--model", "deepfm", "--data", short, "--features",
               str(F), "--k", "8", "--device", "cpu", "--load", model_path,
               "--dump", dump_path])
    assert rc == 0
