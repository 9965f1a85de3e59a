"""Do the replicas of a data-parallel run still hold the same bits?

Every rank fingerprints its tensors on its own device -- ONE launch of ``csbsr_fingerprint`` (csrc/elementwise.hip) over the chunk map and
the pinned staging table of the one-launch optimisers (csbsr_amd/optim.py) -- and the ranks compare the [T, 2] tables with a MIN and a MAX
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

_CHUNK = 8192          # 32-bit words per workgroup (the optimisers' chunk)
_FP_DT = np.dtype([("w", "<u8"), ("n", "<i8"), ("vec", "<i4"), ("pad", "<i4")])
assert _FP_DT.itemsize == 24

_maps = {}          # (word counts, device) -> (block_tensor, block_chunk) device int32 tensors
_host = {}          # device -> [pinned staging, device table, event after the last launch that read it]


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


def _block_maps(sizes, dev):
    key = (tuple(sizes), str(dev))
    mp = _maps.get(key)
    if mp is None:
        bt = [np.full((n + _CHUNK - 1) // _CHUNK, i, dtype=np.int32) for i, n in enumerate(sizes)]
        bc = [np.arange((n + _CHUNK - 1) // _CHUNK, dtype=np.int32) for n in sizes]
        mp = _maps[key] = (torch.from_numpy(np.concatenate(bt)).to(dev), torch.from_numpy(np.concatenate(bc)).to(dev))
    return mp


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
        bt, bc = _block_maps(sizes, dev)
        raw = torch.from_numpy(tab.view(np.uint8))
        host = _host.get(str(dev))
        if host is not None and host[0].numel() >= raw.numel():
            host[2].synchronize()          # the pinned bytes must not change under the previous call's copy
        else:
            n = max(raw.numel(), 4096)
            host = _host[str(dev)] = [torch.empty(n, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.uint8, device=dev),
                                      torch.cuda.Event()]
        host[0][:raw.numel()].copy_(raw)
        host[1][:raw.numel()].copy_(host[0][:raw.numel()], non_blocking=True)
        stream = torch.cuda.current_stream(dev)
        L.call("csbsr_fingerprint", C.c_void_p(host[1].data_ptr()), C.c_void_p(bt.data_ptr()), C.c_void_p(bc.data_ptr()), int(bt.numel()),
               C.c_void_p(out.data_ptr()), C.c_void_p(stream.cuda_stream))
        host[2].record(stream)
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
