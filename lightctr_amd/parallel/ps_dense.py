"""Dense-tensor tables for the asynchronous parameter server.

Parity with the reference PS's dense table (tensorShardTable,
reference distribut/paramserver.h:40-47; the 'T' branches of
its pull/push handlers :146-165, :220-240; tensor fusion buffers in
push.h / pull.h): the dense (MLP) weights of a model are fused into ONE flat
fp32 slab in spec order (the BufferFusion analogue, like ring.py's buckets),
the slab is split into contiguous per-shard ranges, and each shard applies
whole-range pushes with the same updater family as the sparse table.

DenseTable needs no torch.distributed, so it is testable in one process.
CPU path: plain torch (the oracle). GPU path: the streaming kernels in
ops/csrc/ps_dense_kernels.hip — check -> device flag, fused decode + updater
gated on the flag, and a pack kernel for pulls; no host synchronisation
between the finite check and the update.
"""

from __future__ import annotations

import math

import torch

_UPDATERS = {"sgd": 0, "adagrad": 1, "dcasgd": 2, "dcasgda": 3}
_WIRE_DTYPE = {"fp32": torch.float32, "fp16": torch.float16,
               "int8": torch.uint8}


def dense_offsets(spec):
    """spec: ordered ((name, shape), ...) -> ({name: (offset, shape)},
    total): where each tensor lives in the fused flat slab."""
    offs, off = {}, 0
    for name, shape in spec:
        shape = tuple(int(d) for d in shape)
        assert name not in offs, f"duplicate dense tensor {name!r}"
        offs[name] = (off, shape)
        off += math.prod(shape)
    return offs, off


def dense_total(spec) -> int:
    return dense_offsets(spec)[1]


def dense_range(total: int, ps_shards: int, s: int):
    """[lo, hi) of the fused slab owned by shard s: contiguous chunks of
    ceil(total / ps_shards) rounded up to a multiple of 8 elements (32 B, so
    every shard's range starts vector-aligned). Trailing shards may be empty
    (lo == hi); empty shards are never messaged."""
    chunk = (total + ps_shards - 1) // ps_shards
    chunk = (chunk + 7) // 8 * 8
    lo = min(s * chunk, total)
    return lo, min(lo + chunk, total)


def mlp_dense_spec(dims):
    """Dense spec of models.mlp.MLP(dims): layer order, W then b per layer —
    the order of MLP.flat_params / load_flat / flat_grads."""
    spec = []
    for i in range(len(dims) - 1):
        spec.append((f"layer{i}.W", (dims[i + 1], dims[i])))
        spec.append((f"layer{i}.b", (dims[i + 1],)))
    return tuple(spec)


def dense_codec(mode: str, device="cpu"):
    """Codec for dense int8 pushes (values pre-scaled into [-1, 1] by the
    push's max-abs). "custom" is a normal-CDF table with sigma = 1/4: the
    max of a few thousand near-normal gradient values sits near 4 sigma."""
    from ..utils.compress import QuantileCodec

    if mode == "custom":
        return QuantileCodec(mode="custom", mu=0.0, sigma=0.25,
                             device=device)
    return QuantileCodec(mode=mode, device=device)


class DenseTable:
    """Server-side dense slab of n fp32 elements with the sparse table's
    updater family applied elementwise (PSShard._apply math):

      sgd      w -= lr*g
      adagrad  a += g^2;               w -= lr*g/sqrt(a+eps)
      dcasgd   w -= lr*(g + lam*g^2*(w - shadow[wi]));  shadow[wi] = w
      dcasgda  a = .95a + .05g^2; lam' = lam/sqrt(a+eps); then dcasgd

    Drop rule: a push with any non-finite payload element (or a non-finite
    int8 scale) is dropped whole — slab, accumulator and shadows stay
    bit-identical and `dropped` goes up by one. An int8 push is judged on
    every codec table entry times the scale (all it could decode to), so a
    finite scale that overflows the largest entry drops the push too.
    """

    def __init__(self, n: int, updater: str = "dcasgd", lr: float = 0.05,
                 dc_lambda: float = 0.1, eps: float = 1e-8,
                 n_workers: int = 1, device="cpu", init=None,
                 init_sigma: float = 0.01, seed: int = 1234,
                 int8_mode: str = "log"):
        assert n >= 1
        assert updater in _UPDATERS, updater
        self.n = n
        self.updater = updater
        self.lr, self.dc_lambda, self.eps = lr, dc_lambda, eps
        self.n_workers = n_workers
        self.device = torch.device(device)
        if init is not None:
            assert init.numel() == n
            self.slab = init.detach().reshape(-1).to(
                self.device, torch.float32).clone()
        else:
            g = torch.Generator().manual_seed(seed)
            self.slab = (torch.randn(n, generator=g) * init_sigma).to(
                self.device)
        self.acc = None
        if updater in ("adagrad", "dcasgda"):
            self.acc = torch.zeros(n, device=self.device)
        self.shadow = None
        if updater in ("dcasgd", "dcasgda"):
            # rows padded to 4 elements so every worker's row starts
            # 16-byte aligned for the vector kernels
            n_pad = (n + 3) // 4 * 4
            self.shadow = torch.zeros(n_workers, n_pad,
                                      device=self.device)[:, :n]
        self._gpu = self.device.type == "cuda"
        self._int8_mode = int8_mode
        self._codec = None
        self._dropped = 0
        if self._gpu:
            from ..ops._extension import require_hip_ops

            require_hip_ops()
            # {corrupt-push flag, dropped counter}, both device-resident
            self._flags = torch.zeros(2, dtype=torch.int32,
                                      device=self.device)

    @property
    def codec(self):
        if self._codec is None:
            self._codec = dense_codec(self._int8_mode, self.device)
        return self._codec

    @property
    def dropped(self) -> int:
        """Dropped pushes so far (reads the device counter on GPU)."""
        return int(self._flags[1]) if self._gpu else self._dropped

    def _check_payload(self, payload, wire, scale):
        assert wire in _WIRE_DTYPE, wire
        assert payload.dtype == _WIRE_DTYPE[wire], (payload.dtype, wire)
        assert payload.numel() == self.n
        if wire == "int8":
            assert scale is not None and scale.numel() == 1

    def apply(self, wi: int, payload: torch.Tensor, wire: str = "fp32",
              scale: torch.Tensor | None = None) -> None:
        """One push from worker wi. payload: fp32 | fp16 | uint8 codes
        (codec table + 1-element `scale`, like the sparse int8 push)."""
        self._check_payload(payload, wire, scale)
        if self._gpu:
            self._apply_hip(wi, payload.reshape(-1), wire, scale)
        else:
            self._apply_torch(wi, payload.reshape(-1), wire, scale)

    def _apply_hip(self, wi, payload, wire, scale):
        from ..ops._extension import require_hip_ops

        ops = require_hip_ops()
        table = None
        if wire == "int8":
            table = self.codec.table
            scale = scale.reshape(1).to(self.device, torch.float32)
        else:
            scale = None
        payload = payload.contiguous()
        ops.ps_dense_check(payload, scale, table, self._flags)
        ops.ps_dense_apply(
            payload, scale, table, self.slab, self.acc,
            self.shadow[wi] if self.shadow is not None else None,
            self._flags, _UPDATERS[self.updater], self.lr, self.dc_lambda,
            self.eps)

    def _apply_torch(self, wi, payload, wire, scale):
        if wire == "int8":
            # validity is judged on every table entry times the scale (what
            # any code could decode to), exactly as ps_dense_check does
            # (a non-finite scale makes every entry non-finite)
            levels = self.codec.table * scale.reshape(1)
            g = levels[payload.long()]
        else:
            levels = g = payload.float()
        if not bool(torch.isfinite(levels).all()):
            self._dropped += 1
            return
        lr, w = self.lr, self.slab
        if self.updater == "sgd":
            w -= lr * g
        elif self.updater == "adagrad":
            self.acc += g * g
            w -= lr * g / (self.acc + self.eps).sqrt()
        else:
            lam = self.dc_lambda
            if self.updater == "dcasgda":
                self.acc.copy_(0.95 * self.acc + 0.05 * g * g)
                lam = self.dc_lambda / (self.acc + self.eps).sqrt()
            sh = self.shadow[wi]
            w.copy_(w - lr * (g + lam * g * g * (w - sh)))
            sh.copy_(w)

    def pack(self, wi: int, wire: str = "fp32") -> torch.Tensor:
        """Pull payload for worker wi: an fp32 copy of the slab, or fp16
        (parameters never travel as int8 — wire="int8" pulls go as fp32).
        For dcasgd* it also records shadow[wi] = slab in the same pass."""
        fp16 = wire == "fp16"
        sh = self.shadow[wi] if self.shadow is not None else None
        if self._gpu:
            from ..ops._extension import require_hip_ops

            return require_hip_ops().ps_dense_pack(self.slab, sh, fp16)
        out = self.slab.clone()
        if sh is not None:
            sh.copy_(out)
        return out.to(torch.float16) if fp16 else out
