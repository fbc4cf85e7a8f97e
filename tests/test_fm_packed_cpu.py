"""FMModel(pack_linear=...) on the CPU: the layout of the linear state, the
reference train step on the column views, and checkpoints across layouts."""

import pytest
import torch

from lightctr_amd.models.fm import FMHyper, FMModel

F, K = 50, 8


def _hyper(opt="ftrl"):
    return FMHyper(num_features=F, k=K, optimizer=opt, seed=3)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    B, per = 6, 5
    fids = torch.randint(0, F, (B * per,), generator=g).int()
    row_ptr = (torch.arange(B + 1) * per).int()
    vals = torch.rand(B * per, generator=g) + 0.5
    labels = torch.randint(0, 2, (B,), generator=g).float()
    return row_ptr, fids, vals, labels


def _train(m, steps=3):
    return [m.train_step(*_batch(s)) for s in range(steps)]


def test_packed_views_share_lin_storage():
    m = FMModel(_hyper(), pack_linear=True)
    assert m.lin.shape == (F, 4) and m.lin.data_ptr() % 16 == 0
    for col, t in enumerate((m.W, m.nW, m.zW)):
        assert t.shape == (F,) and t.stride(0) == 4
        assert t.data_ptr() == m.lin.data_ptr() + 4 * col
        t[7] = col + 1.0
        assert m.lin[7, col] == col + 1.0
    a = FMModel(_hyper("adagrad"), pack_linear=True)
    assert not hasattr(a, "zW") and a.nW.data_ptr() == a.lin.data_ptr() + 4


def test_unpacked_tensors_are_contiguous():
    m = FMModel(_hyper(), pack_linear=False)
    assert m.lin is None
    for t in (m.W, m.nW, m.zW):
        assert t.shape == (F,) and t.is_contiguous()
    assert len({t.data_ptr() for t in (m.W, m.nW, m.zW)}) == 3


@pytest.mark.parametrize("opt", ["adagrad", "ftrl"])
def test_cpu_train_step_packed_equals_unpacked(opt):
    a = FMModel(_hyper(opt), pack_linear=True)
    b = FMModel(_hyper(opt), pack_linear=False)
    for la, lb in zip(_train(a), _train(b)):
        assert torch.equal(la, lb)
    sa, sb = a.state_dict(), b.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        if k != "hyper":
            assert torch.equal(sa[k], sb[k]), k
    assert a.W.abs().sum() > 0
    assert not a.lin[:, 3].any()


@pytest.mark.parametrize("src", [True, False])
@pytest.mark.parametrize("dst", [True, False])
def test_save_load_across_layouts(tmp_path, src, dst):
    a = FMModel(_hyper(), pack_linear=src)
    _train(a)
    path = str(tmp_path / "fm.pt")
    a.save(path)
    d = torch.load(path, weights_only=True)
    for k in ("W", "nW", "zW"):
        assert d[k].shape == (F,) and d[k].is_contiguous()
        assert d[k].untyped_storage().nbytes() == 4 * F
    b = FMModel(_hyper(), pack_linear=dst)
    b.load(path)
    for k in ("W", "nW", "zW", "V", "nV", "zV"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    for la, lb in zip(_train(a, 1), _train(b, 1)):
        assert torch.equal(la, lb)
