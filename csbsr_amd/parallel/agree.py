"""Do the replicas of a data-parallel run still hold the same bits?

Every rank fingerprints its tensors on its own device -- ONE launch of ``csbsr_fingerprint`` (csrc/multi_tensor.hip) over the chunk map and
the pinned staging table of the one-launch optimisers (csbsr_amd/multi_tensor.py) -- and the ranks compare the [T, 2] tables with a MIN and a MAX
all-reduce: a few KB on the wire where gathering the tensors themselves would be 357 MB per rank.  A row whose minimum and maximum differ
names a tensor that is not the same on every rank; every rank computes the same list.

The fingerprint of a tensor read as n 32-bit words w_j, unsigned 64-bit arithmetic that wraps:

    [0] = sum_j w_j              any change of a single word changes it
    [1] = sum_j w_j (j + 1)      any exchange of two unequal words changes it

It is a drift detector -- replicas that took different arithmetic somewhere (a schedule, a skipped step, a stray write) -- not a hash
against an adversary, and it says nothing about WHICH replica is right.  No CPU / torch fallback: tensors on a GPU only.
"""
import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

from .. import _lib as L
from .. import multi_tensor as MT

_FP_DT = np.dtype([("w", "<u8"), ("n", "<i8"), ("vec", "<i4"), ("pad", "<i4")])
assert _FP_DT.itemsize == 24

_host = {}          # device -> Staging of the table


class ReplicaMismatch(RuntimeError):
    """the replicas of a data-parallel run do not hold the same values; ``names`` lists the tensors that differ"""

    def __init__(self, message, names=()):
        super().__init__(message)
        self.names = list(names)


def _words(t, dev):
    """number of 32-bit words of an accepted tensor; raises for everything else"""
    if not torch.is_tensor(t):
        raise ValueError(f"csbsr_amd.parallel.agree: expected a tensor, got {type(t).__name__}")
    if t.is_sparse or not t.is_contiguous():
        raise ValueError("csbsr_amd.parallel.agree: dense contiguous tensors only")
    nbytes = t.numel() * t.element_size()
    if nbytes % 4:
        raise ValueError(f"csbsr_amd.parallel.agree: {nbytes} bytes ({t.dtype} x {t.numel()}) are not a whole number of 32-bit words")
    if not t.is_cuda:
        raise L.CsbsrHipError("csbsr_amd.parallel.agree: tensors on a GPU only: csbsr_amd has no fallback path")
    if t.device != dev:
        raise ValueError(f"csbsr_amd.parallel.agree: tensors on one device only ({t.device} and {dev})")
    return nbytes // 4


def fingerprint(tensors):
    """[T, 2] int64 on the tensors' device (the unsigned 64-bit sums, bit for bit; nothing is read back): row t is the fingerprint of
    ``tensors[t]``.  Accepted: tensors on one GPU, contiguous, of a byte length that is a multiple of 4 (fp32 parameters and buffers,
    the int64 ``num_batches_tracked``); a host tensor is a CsbsrHipError, anything else a ValueError.  An empty tensor has the row (0, 0)."""
    tensors = [t.detach() if torch.is_tensor(t) else t for t in tensors]
    if not tensors:
        raise ValueError("csbsr_amd.parallel.agree: nothing to fingerprint")
    dev = tensors[0].device if torch.is_tensor(tensors[0]) else None
    sizes = [_words(t, dev) for t in tensors]
    L.load()
    tab = np.zeros(len(tensors), dtype=_FP_DT)
    for i, (t, n) in enumerate(zip(tensors, sizes)):
        tab[i] = (t.data_ptr(), n, int(t.data_ptr() % 16 == 0), 0)
    with torch.cuda.device(dev):
        out = torch.zeros(len(tensors), 2, dtype=torch.int64, device=dev)          # (zeroed on the stream the kernel adds on)
        if not any(sizes):
            return out
        staging = _host.setdefault(str(dev), MT.Staging(dev))
        MT.launch("csbsr_fingerprint", staging, tab.view(np.uint8), sizes, dev, C.c_void_p(out.data_ptr()))
    return out


def _named(named_tensors):
    items = list(named_tensors.items()) if hasattr(named_tensors, "items") else list(named_tensors)
    return [str(k) for k, _ in items], [v for _, v in items]


def replicas_agree(named_tensors, process_group=None):
    """Names (in the order given) of the tensors of ``named_tensors`` -- a dict or an iterable of (name, tensor) -- that are not
    bit-identical on every rank of ``process_group``, as far as the fingerprint can tell: one launch, then a MIN and a MAX all-reduce of
    the [T, 2] table; a row differs where min != max.  Every rank must call it with the same list and every rank gets the same answer.
    Without an initialised process group there is one replica and the answer is []."""
    names, tensors = _named(named_tensors)
    if not names:
        return []
    lo = fingerprint(tensors)
    if not (dist.is_available() and dist.is_initialized()):
        return []
    hi = lo.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=process_group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=process_group)
    differs = (lo != hi).any(dim=1).tolist()
    return [n for n, d in zip(names, differs) if d]


def assert_replicas_agree(named_tensors, process_group=None, what="replicas"):
    """Raise ReplicaMismatch -- on EVERY rank, the answer is common -- when ``replicas_agree`` names a tensor; the message carries the
    first one and the count."""
    bad = replicas_agree(named_tensors, process_group)
    if bad:
        raise ReplicaMismatch(f"{what} differ between ranks: {bad[0]!r}" + (f" and {len(bad) - 1} more" if len(bad) > 1 else "")
                              + " (per-tensor fingerprints, csbsr_fingerprint)", bad)
