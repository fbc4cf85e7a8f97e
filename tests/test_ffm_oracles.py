"""CPU checks of the FFM float64 oracles in ``ffm_oracles.py`` and of what
the GPU parity tests in ``test_ffm_kernels_gpu.py`` can see.

Self-consistency: on the exact set the oracles equal ``ffm_ref`` (fp32,
exact there) element for element; on the float set they agree within the
sum rule; one CPU ``FFMModel.train_step`` lands on the oracle's update.

Mutation sensitivity: on the GPU tests' own inputs each deliberately wrong
reference differs from the right one in at least one element (the GPU
assertion on the exact set is equality), and on the float set the
dropped-partner and wrong-slice references leave the derived bound.
"""

import pytest
import torch

import ffm_oracles as fo
import kernel_oracles as ko
from lightctr_amd.models.ffm import FFMHyper, FFMModel
from lightctr_amd.ops import ffm_ref, fm_ref

CSR = ("row_ptr", "fields", "fids", "vals")


def csr(c):
    return tuple(c[k] for k in CSR)


def kinds_differ(K, shape, mutant, kinds=fo.ROW_KINDS, total_mutant=None,
                 which="V"):
    """kinds for which the mutant totals differ from the right ones in at
    least one of the two batches"""
    hit = []
    for kind in kinds:
        for c in fo.exact_cases(K, shape, kind):
            ref = fo.ffm_backward_totals_ref(c)
            mut = fo.ffm_backward_totals_ref(c, mutant=mutant,
                                             total_mutant=total_mutant)
            i = 1 if which == "V" else 0
            if ko.differs(mut[i], ref[i]):
                hit.append(kind)
                break
    return hit


# ---------------------------------------------------------------------------
# self-consistency
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", fo.KS)
@pytest.mark.parametrize("kind", fo.ROW_KINDS)
def test_exact_oracles_equal_ffm_ref(K, kind):
    for c in fo.exact_cases(K, "q1", kind):
        pred, mag, _ = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"])
        fo.assert_exact_fp32("forward", mag)
        assert torch.equal(pred.float(), ffm_ref.ffm_forward_ref(
            *csr(c), c["W"], c["V"]))
        gW, gV, magW, magV = fo.ffm_backward_totals_ref(c)
        fo.assert_exact_fp32("gradV", magV)
        rW, rV = ffm_ref.ffm_backward_ref(*csr(c), c["V"], c["dpred"])
        assert torch.equal(gW.float(), rW)
        assert torch.equal(gV.float().view_as(rV), rV)


@pytest.mark.parametrize("K", fo.KS)
def test_float_oracles_match_ffm_ref(K):
    c = fo.float_emit_case(K)
    pred, mag, nterms = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"])
    out = ffm_ref.ffm_forward_ref(*csr(c), c["W"], c["V"])
    assert ((out.double() - pred).abs() <= nterms * ko.U23 * mag).all()
    gW, gV, magW, magV = fo.ffm_backward_totals_ref(c)
    rW, rV = ffm_ref.ffm_backward_ref(*csr(c), c["V"], c["dpred"])
    n = c["fids"].numel()  # more terms than any one element sums
    assert ((rW.double() - gW).abs() <= n * ko.U23 * magW).all()
    assert ((rV.double().view_as(gV) - gV).abs() <= n * ko.U23 * magV).all()


def test_oracles_match_model_cpu_train_step():
    """one CPU Adagrad step of FFMModel equals adagrad_ref applied to the
    oracle's totals of the step's own dpred"""
    K, nf = 4, 5
    c = fo.float_case(K, nf, [3, 0, 7, 1, 12], seed=5)
    h = FFMHyper(num_features=fo.F_TABLE, num_fields=nf, k=K, lr=0.05)
    m = FFMModel(h)
    m.W.copy_(c["W"])
    m.V.copy_(c["V"])
    labels = torch.tensor([1.0, 0.0, 1.0, 0.0, 1.0])
    m.train_step(*csr(c), labels)
    pred = ffm_ref.ffm_forward_ref(*csr(c), c["W"], c["V"])
    _, dpred = fm_ref.logloss_grad_ref(pred, labels, 1.0 / 5)
    c = dict(c, dpred=dpred)
    gW, gV, magW, magV = fo.ffm_backward_totals_ref(c)
    live = torch.unique(c["fids"].long())
    rW = ko.adagrad_ref(c["W"][live], gW[live], torch.zeros(live.numel()),
                        h.lr, h.eps, h.l2)
    Vf = c["V"].view(fo.F_TABLE, -1)
    rV = ko.adagrad_ref(Vf[live], gV[live], torch.zeros_like(Vf[live]),
                        h.lr, h.eps, h.l2)

    def grad_slack(g64, mag, w):
        """the model's gradient is an fp32 sum of fewer than nnz terms:
        |dg| <= nnz 2^-23 sum|term| (sum rule). From n = 0 the step is
        lr g / sqrt(g^2 + eps) with g the gradient plus l2 w, whose slope
        lr eps / (g^2 + eps)^1.5 falls with |g|; taken at |g| - |dg| it
        bounds the step's change over the whole interval."""
        dg = c["fids"].numel() * ko.U23 * mag
        lo = ((g64 + ko.f32(h.l2) * w.double()).abs() - dg).clamp(min=0)
        return ko.f32(h.lr) * ko.f32(h.eps) \
            / (lo * lo + ko.f32(h.eps)) ** 1.5 * dg

    assert ((m.W[live].double() - rW["W"][0]).abs() <= rW["W"][1]
            + grad_slack(gW[live], magW[live], c["W"][live])).all()
    assert ((m.V.view(fo.F_TABLE, -1)[live].double() - rV["W"][0]).abs()
            <= rV["W"][1] + grad_slack(gV[live], magV[live], Vf[live])).all()
    rest = torch.ones(fo.F_TABLE, dtype=torch.bool)
    rest[live] = False
    assert torch.equal(m.V[rest], c["V"][rest])


def test_builders():
    rows = [[(5, 1, 2.0), (9, 0, 1.0)], [], [(5, 2, 1.0)]]
    row_ptr, fields, fids, vals = fo.make_ffm_csr(rows)
    assert row_ptr.tolist() == [0, 2, 2, 3]
    assert fids.tolist() == [5, 9, 5] and fields.tolist() == [1, 0, 2]
    sf, pm = fo.make_runs([3, 1, 2], 100, seed=1)
    assert sf.numel() == 6 and sorted(pm.tolist()) == list(range(6))
    _, counts = torch.unique_consecutive(sf, return_counts=True)
    assert counts.tolist() == [3, 1, 2] and (sf[1:] >= sf[:-1]).all()
    c = fo.csr_from_runs(fo.SORTED_RUNS, 3, 4, seed=2)
    _, counts = torch.unique_consecutive(fo.sort_entries(c["fids"])[0],
                                         return_counts=True)
    assert sorted(counts.tolist()) == sorted(fo.SORTED_RUNS)
    t = fo.touched_words(torch.tensor([0, 63, 64, 700]), 1024)
    assert [f for f in range(1024) if fo.bit_is_set(t, f)] == [0, 63, 64,
                                                               700]
    assert int(t[0]) < 0  # bit 63 set: the word is negative as int64
    # the x scaling doubles the last entry of rows with a partner only
    c = fo.float_case(4, 5, [3, 1, 0, 2], seed=9)
    s = fo.scale_last_x_until(c, lambda c: float(c["vals"].max()) >= 4.0)
    ratio = (s["vals"] / c["vals"]).tolist()
    assert ratio[2] in (4.0, 8.0)
    assert ratio == [1.0, 1.0, ratio[2], 1.0, 1.0, ratio[2]]


@pytest.mark.parametrize("K", fo.KS)
def test_row_kinds_are_what_they_say(K):
    """the direct-emit kinds are duplicate-free for n <= nfields; dup1 has
    exactly one repeated field; the samefid kinds repeat a fid"""
    for shape in fo.shape_names(K):
        nf = fo.SHAPES[K][shape]
        for kind in fo.ROW_KINDS:
            for c in fo.exact_cases(K, shape, kind):
                assert int(c["fields"].max()) < nf
                rp = c["row_ptr"].tolist()
                for r in range(len(rp) - 1):
                    fl = c["fields"][rp[r]:rp[r + 1]].tolist()
                    fd = c["fids"][rp[r]:rp[r + 1]].tolist()
                    n = len(fl)
                    if kind in ("ordered", "shuffled") and n <= nf:
                        assert len(set(fl)) == n
                        if kind == "ordered":
                            assert fl == sorted(fl)
                    if kind == "dup1" and 2 <= n <= nf + 1:
                        assert len(set(fl)) == n - 1
                    if kind == "onefield":
                        assert len(set(fl)) <= 1
                    if kind.startswith("samefid") and n >= 2:
                        assert fd[0] == fd[1]
                        assert (fl[0] == fl[1]) == (kind == "samefid1f"
                                                    or nf == 1)
                    else:
                        assert len(set(fd)) == n


# ---------------------------------------------------------------------------
# mutation sensitivity on the exact set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", fo.KS)
def test_forward_mutant_differs(K):
    for shape in ("q1", "q2"):
        hit = False
        for kind in fo.ROW_KINDS:
            for c in fo.exact_cases(K, shape, kind):
                ref = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"])[0]
                mut = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"],
                                           mutant="droppair")[0]
                hit |= ko.differs(mut, ref)
        assert hit, shape
    c = fo.long_row_case()
    ref, mag, _ = fo.ffm_forward_ref64(*csr(c), c["W"], c["V"])
    fo.assert_exact_fp32("n=1000", mag)


@pytest.mark.parametrize("K", fo.KS)
@pytest.mark.parametrize("mutant", ["droplastpartner", "wrongslice",
                                    "dupdrop", "self", "dropmaxn",
                                    "quadfield"])
def test_block_mutants_differ(K, mutant):
    """every row kind of the MAXQ 2 shape sees the mutant, in the per-entry
    blocks and in the per-fid totals. dupdrop needs a repeated field: the
    rows longer than nfields of every kind have one. wrongslice cannot show
    where every entry sits in one field (F_j = F_p)."""
    kinds = [k for k in fo.ROW_KINDS
             if not (mutant == "wrongslice" and k == "onefield")]
    for kind in kinds:
        seen_blocks = False
        for c in fo.exact_cases(K, "q2", kind):
            args = (*csr(c), c["V"], c["dpred"])
            ref = fo.ffm_entry_blocks_ref(*args)[1]
            mut = fo.ffm_entry_blocks_ref(*args, mutant=mutant)[1]
            seen_blocks |= ko.differs(mut, ref)
        assert seen_blocks, kind
    assert kinds_differ(K, "q2", mutant, kinds) == kinds


@pytest.mark.parametrize("K", fo.KS)
def test_emit_cases_are_exact_in_fp16(K):
    """|sum over same-field partners| * scale <= 2048 at every scale, for
    every shape the row emit runs"""
    for shape in fo.shape_names(K, row_emit=True):
        for scale in fo.SCALES:
            for c in fo.exact_cases(K, shape, "onefield", scale=scale):
                _, blocks, mag, _, _ = fo.ffm_entry_blocks_ref(
                    *csr(c), c["V"], c["dpred"])
                fo.assert_exact_fp16("emit", blocks, scale)
                fo.assert_exact_fp32("emit acc", mag * scale)


@pytest.mark.parametrize("mutant", ["droprunlast", "dropchunkfirst",
                                    "noinvscale", "droplastquad",
                                    "dropgwtail"])
def test_apply_mutants_differ(mutant):
    """on the hand-built apply inputs. dropchunkfirst needs more than one
    chunk; droplastquad is shown at D = 516; dropgwtail only moves gradW"""
    for D in fo.APPLY_DS:
        for name in fo.RUNS:
            a = fo.apply_inputs(D, name)
            nnz = a["sorted_fids"].numel()
            if mutant == "dropchunkfirst" and nnz <= fo.APPLY_CHUNK:
                continue
            if mutant == "droplastquad" and D != 516:
                continue
            args = (a["sorted_fids"], a["perm"], a["gblocks"], a["gw"],
                    a["F"], a["inv_scale"])
            ref = fo.ffm_totals_ref(*args)
            fo.assert_exact_fp32("apply", ref[3] / a["inv_scale"])
            mut = fo.ffm_totals_ref(*args, mutant=mutant)
            if mutant == "dropgwtail":
                assert ko.differs(mut[0], ref[0]), (D, name)
                assert not ko.differs(mut[1], ref[1])
            else:
                assert ko.differs(mut[1], ref[1]), (D, name)


def test_sorted_walk_mutants_differ():
    """chunk 32: the CSR built from runs of 31, 32, 33 and 70"""
    c = fo.csr_from_runs(fo.SORTED_RUNS, 65, 16, seed=65016)
    ref = fo.ffm_backward_totals_ref(c)
    for tm in ("droprunlast", "dropchunkfirst", "dropgwtail"):
        mut = fo.ffm_backward_totals_ref(c, total_mutant=tm,
                                         chunk=fo.SORTED_CHUNK)
        i = 0 if tm == "dropgwtail" else 1
        assert ko.differs(mut[i], ref[i]), tm


# ---------------------------------------------------------------------------
# float set: the derived row-emit bound catches the mutants
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K", fo.KS)
@pytest.mark.parametrize("v_is_fp32", [True, False])
def test_float_emit_bound_catches_mutants(K, v_is_fp32):
    c = fo.float_emit_case(K)
    V = c["V"] if v_is_fp32 else c["V"].to(torch.bfloat16).float()
    args = (*csr(c), V, c["dpred"])
    _, ref, mag, npart, cmag = fo.ffm_entry_blocks_ref(*args)
    bound = fo.row_emit_bound(mag, npart, cmag, 1.0, v_is_fp32)
    for m in ("droplastpartner", "wrongslice"):
        mut = fo.ffm_entry_blocks_ref(*args, mutant=m)[1]
        assert ko.differs(mut, ref, bound), m


def test_cpu_model_has_no_lds_limit():
    """the LDS limit of the sorted walk belongs to the device: a CPU model
    takes any (num_fields, k) pair and one step moves its weights"""
    m = FFMModel(FFMHyper(num_features=64, num_fields=160, k=64))
    assert m.backward_mode == "sorted"
    batch = fo.make_ffm_csr([[(1, 0, 1.0), (2, 159, 1.0), (3, 5, 0.5)],
                             [(4, 7, 1.0), (1, 3, 1.0)]])
    V0 = m.V.clone()
    m.train_step(*batch, torch.tensor([1.0, 0.0]))
    assert (m.V != V0).any()
