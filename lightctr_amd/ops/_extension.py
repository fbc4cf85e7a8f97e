"""Loader for the in-tree HIP extension (lightctr_amd.ops._hip_ops).

The extension is built in-tree by ``python setup.py build_ext --inplace``
(driven by __graft_entry__.build()) so the .so ships with the repo snapshot
to GPU boxes. On a machine with a GPU, ops FAIL LOUDLY if the extension is
missing — no silent eager fallback on the compute path.
"""

from __future__ import annotations

import torch  # noqa: F401  -- loads libc10/libtorch before the extension

_hip_ops = None
_import_error: Exception | None = None

try:
    from . import _hip_ops as _ext  # type: ignore

    _hip_ops = _ext
except ImportError as e:  # extension not built (CPU-only dev box is fine)
    _import_error = e


def has_hip_ops() -> bool:
    return _hip_ops is not None


def require_hip_ops():
    if _hip_ops is None:
        raise ImportError(
            "lightctr_amd HIP extension (_hip_ops) is not built but a GPU "
            "op was requested. Build it in-tree with "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace`. "
            f"Original import error: {_import_error!r}"
        )
    return _hip_ops


class _LazyOps:
    """Attribute access proxy: hip_ops.fm_forward(...) resolves at call time."""

    def __getattr__(self, name):
        return getattr(require_hip_ops(), name)


hip_ops = _LazyOps()


def sort_end_bit(upper: int) -> int:
    """Bits a radix sort has to look at for ids known to be < upper."""
    return max(1, int(upper - 1).bit_length())


def sort_ids(fids, upper: int):
    """(sorted, perm int64) for nonnegative int32 ids known to be < upper —
    drop-in for torch.sort(fids) on the GPU hot path, but radix-sorts only
    the live bit range (2-3 passes instead of 4; see sort_kernels.hip)."""
    end_bit = sort_end_bit(upper)
    return require_hip_ops().radix_sort_index(fids, end_bit)


def sort_ids_rec(fids, rec, upper: int, impl: str = "onesweep", status=None):
    """(sorted, sorted_rec): the same bit-range sort carrying one 8-byte
    record per id (rec int32 [n, 2]) as its payload instead of an index.

    impl="onesweep": the single-purpose sort (one memset, one histogram
    kernel, one scatter kernel per 8-bit pass); status is the caller's int32
    word that a bounded look-back spin marks on give-up. impl="rocprim":
    rocPRIM's radix sort, also taken where the onesweep binding does not
    accept the arguments (end_bit 32, n >= 2^30). Both give the same stable
    permutation."""
    if impl not in ("onesweep", "rocprim"):
        raise ValueError(f"unknown sort impl {impl!r}")
    ops = require_hip_ops()
    end_bit = sort_end_bit(upper)
    if impl == "onesweep" and end_bit <= 31 and fids.numel() < (1 << 30):
        return ops.onesweep_sort_rec(fids, rec, end_bit, status)
    return ops.radix_sort_rec(fids, rec, end_bit)
