"""Synthetic Criteo-shaped sparse data generator.

BASELINE.json benchmarks run on "synthetic Criteo-1TB-shaped sparse" data:
39 fields per row (13 numeric-style + 26 categorical-style), one feature per
field, hashed feature ids in a large global id space with a skewed (power-law)
per-field popularity distribution, random-init weights. Labels are drawn from
a planted sparse-linear teacher so that training has a learnable signal and
test AUC is meaningful (> 0.5 and rising), matching how the reference's
bundled datasets behave under its FM trainer.

Generation happens on-device (GPU when available) so the data pipeline never
bottlenecks the benchmark; `data="synthetic"` is reported by bench.py.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

CRITEO_NUM_FIELDS = 39
# Per-field cardinality profile loosely shaped like Criteo: numeric fields are
# bucketized to small cardinalities; categorical fields range from tiny to
# multi-million. Scaled so the default total id space is ~16.7M (2^24).
_CARD_PROFILE = (
    [64] * 13  # bucketized numeric
    + [int(c) for c in [
        1 << 22, 1 << 21, 1 << 20, 1 << 20, 1 << 19, 1 << 18, 1 << 17,
        1 << 16, 1 << 16, 1 << 15, 1 << 14, 1 << 13, 1 << 13, 1 << 12,
        1 << 12, 1 << 11, 1 << 10, 1 << 10, 256, 256, 128, 128, 64, 32, 16, 8,
    ]]
)


@dataclass
class SyntheticCriteo:
    """Stateful generator; yields CSR-shaped batches with fixed nnz/row."""

    num_features: int = 1 << 24
    num_fields: int = CRITEO_NUM_FIELDS
    seed: int = 1234
    device: str = "cpu"
    teacher_dim: int = 1 << 16  # hashed teacher table size

    def __post_init__(self):
        dev = torch.device(self.device)
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        cards = torch.tensor(_CARD_PROFILE[: self.num_fields], dtype=torch.float64)
        # scale cardinalities to fill num_features
        scale = self.num_features / float(cards.sum())
        cards = (cards * scale).clamp(min=2).to(torch.int64)
        excess = int(cards.sum()) - self.num_features
        if excess > 0:  # clamping small fields can overshoot; shrink largest
            big = int(cards.argmax())
            cards[big] -= excess
            assert cards[big] >= 2, "num_features too small for field profile"
        offsets = torch.zeros(self.num_fields + 1, dtype=torch.int64)
        offsets[1:] = torch.cumsum(cards, 0)
        self.field_cards = cards.to(dev)
        self.field_offsets = offsets.to(dev)
        self.total_ids = int(offsets[-1].item())
        assert self.total_ids <= self.num_features
        # planted teacher: per-hashed-id logit contribution
        self.teacher = (torch.rand(self.teacher_dim, generator=g) - 0.5) * 2.0
        self.teacher = self.teacher.to(dev)
        self._gen = torch.Generator(device=dev if dev.type == "cuda" else "cpu")
        self._gen.manual_seed(self.seed + 1)
        self._dev = dev

    def batch(self, batch_size: int):
        """Returns (row_ptr i32 [B+1], fields i32 [nnz], fids i32 [nnz],
        vals f32 [nnz], labels f32 [B]) on self.device; nnz = B*num_fields."""
        B, F = batch_size, self.num_fields
        dev = self._dev
        u = torch.rand(B, F, generator=self._gen, device=self._gen.device).to(dev)
        # power-law skew within each field: id = floor(card * u^2) concentrates
        # mass on low ids (hot features), like real CTR traffic.
        local = (self.field_cards.view(1, F).to(torch.float32) * u * u).to(torch.int64)
        local = torch.minimum(local, (self.field_cards - 1).view(1, F))
        fids64 = self.field_offsets[:F].view(1, F) + local
        # teacher labels on hashed ids (golden-ratio multiplicative hash)
        h = ((fids64 * 2654435761) >> 8) & (self.teacher_dim - 1)
        logits = self.teacher[h].sum(dim=1) * (3.0 / F**0.5)
        labels = (
            torch.rand(B, generator=self._gen, device=self._gen.device).to(dev)
            < torch.sigmoid(logits)
        ).to(torch.float32)
        row_ptr = torch.arange(0, (B + 1) * F, F, dtype=torch.int32, device=dev)
        fields = (
            torch.arange(F, dtype=torch.int32, device=dev).view(1, F).expand(B, F).reshape(-1)
        )
        vals = torch.ones(B * F, dtype=torch.float32, device=dev)
        return row_ptr, fields.contiguous(), fids64.to(torch.int32).reshape(-1), vals, labels


@dataclass
class SyntheticMultiHot:
    """Multi-hot rows as real libffm data has them, for the field-addressed
    concat layout (``layout="field"`` of Wide&Deep / DeepFM).

    Per row every field is absent with probability ``p_missing``; the fields
    listed in ``multi`` carry 1..``max_multi`` values (uniform), the others
    one; the tokens of a row come in shuffled order. All fields share one id
    space (hashed ids), so a fid alone does not name its field: the planted
    teacher scores the pair (field, fid), mean-pooled over a field's values,
    and a model that lays the concat out by position cannot recover it.
    """

    num_features: int = 1 << 16
    num_fields: int = CRITEO_NUM_FIELDS
    multi: tuple = (3, 11, 20, 30)
    max_multi: int = 8
    p_missing: float = 0.1
    seed: int = 1234
    device: str = "cpu"
    teacher_dim: int = 1 << 16

    def __post_init__(self):
        assert all(0 <= c < self.num_fields for c in self.multi), self.multi
        assert self.max_multi >= 1 and 0.0 <= self.p_missing < 1.0
        dev = torch.device(self.device)
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        self.teacher = ((torch.rand(self.teacher_dim, generator=g) - 0.5)
                        * 2.0).to(dev)
        self._gen = torch.Generator(
            device=dev if dev.type == "cuda" else "cpu")
        self._gen.manual_seed(self.seed + 1)
        self._dev = dev
        is_multi = torch.zeros(self.num_fields, dtype=torch.bool)
        is_multi[list(self.multi)] = True
        self._is_multi = is_multi.to(dev)

    def _rand(self, *shape):
        return torch.rand(*shape, generator=self._gen,
                          device=self._gen.device).to(self._dev)

    def batch(self, batch_size: int):
        """(row_ptr i32 [B+1], fields i32 [nnz], fids i32 [nnz], vals f32
        [nnz], labels f32 [B]) on self.device, as SyntheticCriteo.batch."""
        B, nf, m = batch_size, self.num_fields, self.max_multi
        dev = self._dev
        present = self._rand(B, nf) >= self.p_missing
        n = 1 + (self._rand(B, nf) * m).to(torch.int64).clamp(max=m - 1)
        n = torch.where(self._is_multi.view(1, nf), n, torch.ones_like(n))
        n = n * present
        slot = torch.arange(m, device=dev).view(1, 1, m)
        live = slot < n.unsqueeze(2)                       # [B, nf, m]
        u = self._rand(B, nf, m)
        fid = (self.num_features * u * u).to(torch.int64).clamp(
            max=self.num_features - 1)                     # power-law skew
        field = torch.arange(nf, device=dev).view(1, nf, 1).expand(B, nf, m)
        # teacher on the pair (field, fid), mean over a field's values
        h = (((fid * nf + field) * 2654435761) >> 8) & (self.teacher_dim - 1)
        t = torch.where(live, self.teacher[h], torch.zeros((), device=dev))
        per_field = t.sum(dim=2) / n.clamp(min=1)
        logits = per_field.sum(dim=1) * (3.0 / nf ** 0.5)
        labels = (self._rand(B) < torch.sigmoid(logits)).to(torch.float32)
        # shuffled token order: sort the live slots of a row by a random key
        key = torch.where(live, self._rand(B, nf, m),
                          torch.full((), 2.0, device=dev)).view(B, nf * m)
        order = key.argsort(dim=1)
        counts = live.view(B, -1).sum(dim=1)
        keep = torch.arange(nf * m, device=dev).view(1, -1) \
            < counts.view(B, 1)
        fids = fid.reshape(B, nf * m).gather(1, order)[keep]
        fields = field.reshape(B, nf * m).gather(1, order)[keep]
        row_ptr = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        row_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
        vals = torch.ones(fids.numel(), dtype=torch.float32, device=dev)
        return (row_ptr, fields.to(torch.int32).contiguous(),
                fids.to(torch.int32).contiguous(), vals, labels)

    def write_libffm(self, path: str, rows: int) -> None:
        """`rows` rows as ``label field:fid:val`` lines"""
        row_ptr, fields, fids, vals, labels = (
            t.cpu().tolist() for t in self.batch(rows))
        with open(path, "w") as f:
            for r in range(rows):
                toks = [f"{fields[j]}:{fids[j]}:{vals[j]:g}"
                        for j in range(row_ptr[r], row_ptr[r + 1])]
                f.write(" ".join([str(int(labels[r]))] + toks) + "\n")


def synthetic_criteo_batch(
    batch_size: int,
    num_features: int = 1 << 24,
    num_fields: int = CRITEO_NUM_FIELDS,
    seed: int = 1234,
    device: str = "cpu",
):
    return SyntheticCriteo(num_features, num_fields, seed, device).batch(batch_size)
