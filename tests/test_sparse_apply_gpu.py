"""Parity tests for the runtime-D sparse optimizers FFM uses
(misc_kernels.hip): sparse_adagrad_apply and sparse_ftrl_apply against
fm_ref.adagrad_apply_ref / fm_ref.ftrl_apply_ref evaluated in float64 on
[F, D] state.

D in {4, 8, 256, 312} takes the float4 body (312 = 39*8: two trips per
lane, the second partial), D in {6, 70} the scalar body (70: more than one
lane-stride trip); FTRL with v_adagrad=0 takes the scalar body for every
D. Bounds come from kernel_oracles.adagrad_ref / ftrl_ref, whose values
test_kernel_oracles.py ties to fm_ref.
"""

import pytest
import torch

import kernel_oracles as ko
from lightctr_amd.ops import fm_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
DS = (4, 8, 256, 312, 6, 70)
NLIVE = ko.SPARSE_NLIVE
V_OPT = dict(v_lr=0.05, v_eps=1e-8, v_l2=1e-5)
ADA = dict(lr=0.05, eps=1e-8, l2=1e-5)


def ops():
    from lightctr_amd.ops import hip_ops
    return hip_ops


STATE = ("W", "V", "nW", "nV", "zW", "zV", "gradW", "gradV")


def _upload(st):
    return {k: st[k].to(DEV) for k in STATE if k in st}


def _snapshot(gpu, Vh):
    snap = {k: t.cpu().clone() for k, t in gpu.items()}
    if Vh is not None:
        snap["Vh"] = Vh.cpu().clone()
    return snap


def _full(shape, rows, val):
    t = torch.zeros(shape, dtype=torch.float64)
    t[rows] = val
    return t


def _second_grads(st, gpu, seed, ftrl):
    """fresh gradients for the second application (the first zeroed the
    listed slots): random, with the dead-zone rows nudged by 0.1 l1 so
    some |z| stay inside l1 on non-zero n state"""
    g = torch.Generator().manual_seed(seed)
    gW = torch.randn(st["W"].shape, generator=g)
    gV = torch.randn(st["V"].shape, generator=g)
    if ftrl:
        live = st["uniq"][:6].long()
        gW[live] = 0.1 * ko.f32(ko.FTRL["l1"])
        gV[live] = 0.1 * ko.f32(ko.FTRL["l1"])
    gpu["gradW"].copy_(gW)
    gpu["gradV"].copy_(gV)


def _check_untouched(before, after, live):
    """rows past `count` and rows never listed are bit-identical in every
    tensor; listed rows have exactly +0 gradients"""
    F = before["W"].shape[0]
    rest = torch.ones(F, dtype=torch.bool)
    rest[live] = False
    for k in before:
        ko.check_bits("sparse.untouched." + k, after[k][rest],
                      before[k][rest])
    ko.check_bits("sparse.gradW", after["gradW"][live],
                  torch.zeros(live.numel()))
    ko.check_bits("sparse.gradV", after["gradV"][live],
                  torch.zeros(live.numel(), before["V"].shape[1]))


def _check_mirror(after, live):
    if "Vh" in after:
        ko.check_bits("sparse.Vh", after["Vh"][live],
                      after["V"][live].to(BF))


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("mirror", [False, True])
def test_sparse_adagrad_apply(D, mirror):
    """Two consecutive applications (the second on non-zero n), each
    compared with fm_ref.adagrad_apply_ref in float64 from the state the
    GPU held before the call."""
    st = ko.sparse_inputs(D, seed=D)
    live = st["uniq"][:NLIVE].long()
    gpu = _upload(st)
    uniq = st["uniq"].to(DEV)
    count = torch.tensor([NLIVE], dtype=torch.int32, device=DEV)
    Vh = gpu["V"].to(BF) if mirror else None
    for rnd in range(2):
        if rnd:
            _second_grads(st, gpu, seed=D + 50, ftrl=False)
        before = _snapshot(gpu, Vh)
        ref = {k: before[k].double().clone() for k in gpu}
        fm_ref.adagrad_apply_ref(st["uniq"][:NLIVE], ref["W"], ref["V"],
                                 ref["nW"], ref["nV"], ref["gradW"],
                                 ref["gradV"], ko.f32(ADA["lr"]),
                                 ko.f32(ADA["eps"]), ko.f32(ADA["l2"]))
        bW = ko.adagrad_ref(before["W"][live], before["gradW"][live],
                            before["nW"][live], **ADA)
        bV = ko.adagrad_ref(before["V"][live], before["gradV"][live],
                            before["nV"][live], **ADA)
        ops().sparse_adagrad_apply(uniq, count, gpu["W"], gpu["V"],
                                   gpu["nW"], gpu["nV"], gpu["gradW"],
                                   gpu["gradV"], ADA["lr"], ADA["eps"],
                                   ADA["l2"], Vh)
        after = _snapshot(gpu, Vh)
        for k, b in (("W", bW["W"]), ("nW", bW["n"]), ("V", bV["W"]),
                     ("nV", bV["n"])):
            ko.check_bound("sparse_adagrad." + k, after[k], ref[k],
                           _full(ref[k].shape, live, b[1]))
        _check_untouched(before, after, live)
        _check_mirror(after, live)


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("v_adagrad", [1, 0])
@pytest.mark.parametrize("mirror", [False, True])
def test_sparse_ftrl_apply(D, v_adagrad, mirror):
    """Two consecutive applications against fm_ref.ftrl_apply_ref in
    float64. From zero state z' = g exactly, so the rows fed g = +-l1 and
    +-0.5 l1 must come out as exactly +0.0 (the '<=' of the dead zone; '<'
    would give -0.0 at the edge) and the rows fed +-(1 + 2^-10) l1 must
    move. In the second application every weight whose float64 |z'| is
    inside l1 by more than z's bound must again be exactly +0.0."""
    st = ko.sparse_inputs(D, seed=D + 7, ftrl=True)
    live = st["uniq"][:NLIVE].long()
    gpu = _upload(st)
    uniq = st["uniq"].to(DEV)
    count = torch.tensor([NLIVE], dtype=torch.int32, device=DEV)
    Vh = gpu["V"].to(BF) if mirror else None
    l1 = ko.f32(ko.FTRL["l1"])
    for rnd in range(2):
        if rnd:
            _second_grads(st, gpu, seed=D + 60, ftrl=True)
        before = _snapshot(gpu, Vh)
        ref = {k: before[k].double().clone() for k in gpu}
        fm_ref.ftrl_apply_ref(
            st["uniq"][:NLIVE], ref["W"], ref["V"], ref["zW"], ref["nW"],
            ref["zV"], ref["nV"], ref["gradW"], ref["gradV"],
            *(ko.f32(ko.FTRL[k]) for k in ("alpha", "beta", "l1", "l2")),
            v_adagrad=bool(v_adagrad),
            **{k: ko.f32(v) for k, v in V_OPT.items()})
        bW = ko.ftrl_ref(before["W"][live], before["zW"][live],
                         before["nW"][live], before["gradW"][live],
                         **ko.FTRL)
        bounds = {"W": bW["w"][1], "zW": bW["z"][1], "nW": bW["n"][1]}
        if v_adagrad:
            bV = ko.adagrad_ref(before["V"][live], before["gradV"][live],
                                before["nV"][live], lr=V_OPT["v_lr"],
                                eps=V_OPT["v_eps"], l2=V_OPT["v_l2"])
            bounds.update(V=bV["W"][1], nV=bV["n"][1],
                          zV=torch.zeros(NLIVE, D, dtype=torch.float64))
        else:
            bV = ko.ftrl_ref(before["V"][live], before["zV"][live],
                             before["nV"][live], before["gradV"][live],
                             **ko.FTRL)
            bounds.update(V=bV["w"][1], zV=bV["z"][1], nV=bV["n"][1])
        ops().sparse_ftrl_apply(
            uniq, count, gpu["W"], gpu["V"], gpu["zW"], gpu["nW"],
            gpu["zV"], gpu["nV"], gpu["gradW"], gpu["gradV"],
            ko.FTRL["alpha"], ko.FTRL["beta"], ko.FTRL["l1"], ko.FTRL["l2"],
            v_adagrad, V_OPT["v_lr"], V_OPT["v_eps"], V_OPT["v_l2"], Vh)
        after = _snapshot(gpu, Vh)
        for k, b in bounds.items():
            ko.check_bound("sparse_ftrl." + k, after[k], ref[k],
                           _full(ref[k].shape, live, b))
        _check_untouched(before, after, live)
        _check_mirror(after, live)
        # the dead zone, bit for bit
        inside = (bW["z"][0].abs() <= l1 - bW["z"][1])
        if rnd == 0:
            inside[:4] = True  # g = +-l1 (on the edge) and +-0.5 l1
            assert (after["W"][live[4:6]] != 0).all()
        assert int(inside.sum()) >= 4
        ko.check_bits("sparse_ftrl.dead_zone", after["W"][live][inside],
                      torch.zeros(int(inside.sum())))
        if not v_adagrad:
            insideV = (bV["z"][0].abs() <= l1 - bV["z"][1])
            if rnd == 0:
                insideV[:4] = True
                assert (after["V"][live[4:6]] != 0).all()
            ko.check_bits("sparse_ftrl.dead_zone_V",
                          after["V"][live][insideV],
                          torch.zeros(int(insideV.sum())))


@pytest.mark.parametrize("D", [8, 6])
def test_sparse_apply_count_zero_touches_nothing(D):
    """count = 0: every wave returns before reading uniq; all state and
    the gradients stay bit-identical."""
    st = ko.sparse_inputs(D, seed=D + 90, ftrl=True)
    gpu = _upload(st)
    uniq = st["uniq"].to(DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    Vh = gpu["V"].to(BF)
    before = _snapshot(gpu, Vh)
    ops().sparse_adagrad_apply(uniq, count, gpu["W"], gpu["V"], gpu["nW"],
                               gpu["nV"], gpu["gradW"], gpu["gradV"],
                               ADA["lr"], ADA["eps"], ADA["l2"], Vh)
    for v_adagrad in (1, 0):
        ops().sparse_ftrl_apply(
            uniq, count, gpu["W"], gpu["V"], gpu["zW"], gpu["nW"],
            gpu["zV"], gpu["nV"], gpu["gradW"], gpu["gradV"],
            ko.FTRL["alpha"], ko.FTRL["beta"], ko.FTRL["l1"], ko.FTRL["l2"],
            v_adagrad, V_OPT["v_lr"], V_OPT["v_eps"], V_OPT["v_l2"], Vh)
    after = _snapshot(gpu, Vh)
    for k in before:
        ko.check_bits("sparse.count0." + k, after[k], before[k])
