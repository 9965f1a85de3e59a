"""What the multi-tensor kernels of csrc/multi_tensor.hip share on the host: the chunk map (one workgroup per CHUNK elements of one
tensor), the pinned staging of a per-call table, and the launch over both (csbsr_amd/optim.py, csbsr_amd/parallel/agree.py); the staging
alone also carries the selection rows of csbsr_amd/data/resident.py."""
import ctypes as C

import numpy as np
import torch

from . import _lib as L

CHUNK = 8192          # elements per workgroup: CSBSR_MT_CHUNK of csrc/multi_tensor.hip

_maps = {}          # (tensor sizes, device) -> (block_tensor, block_chunk) device int32 tensors


def chunk_maps(sizes, device):
    """(block_tensor, block_chunk) int32 on ``device``: workgroup b handles chunk ``block_chunk[b]`` of tensor ``block_tensor[b]``.  An
    empty tensor gets no workgroup.  Cached per (sizes, device)."""
    key = (tuple(sizes), str(device))
    mp = _maps.get(key)
    if mp is None:
        bt = [np.full((n + CHUNK - 1) // CHUNK, i, dtype=np.int32) for i, n in enumerate(sizes)]
        bc = [np.arange((n + CHUNK - 1) // CHUNK, dtype=np.int32) for n in sizes]
        mp = _maps[key] = (torch.from_numpy(np.concatenate(bt)).to(device), torch.from_numpy(np.concatenate(bc)).to(device))
    return mp


class Staging:
    """A ring of ``slots`` pinned host buffers, each with its device twin and an event.  ``stage`` hands out the next slot's host bytes,
    ``upload`` enqueues ONE non-blocking copy of them, ``record`` marks on the current stream the point after which the slot may be
    rewritten: the pinned bytes must not change under a copy in flight, so ``stage`` waits on that event before it hands the slot out
    again (the only host wait on the device here; it normally returns at once)."""

    def __init__(self, device, slots=1):
        self.device = torch.device(device)
        self._ring, self._next, self._cur = [None] * slots, 0, None

    def stage(self, nbytes, min_bytes):
        """The pinned uint8 [nbytes] view of the next slot, (re)allocated with max(nbytes, min_bytes) bytes where missing or too small."""
        i = self._next
        self._next = (i + 1) % len(self._ring)
        slot = self._ring[i]
        if slot is None or slot[0].numel() < nbytes:
            n = max(nbytes, min_bytes)
            slot = self._ring[i] = (torch.empty(n, dtype=torch.uint8).pin_memory(), torch.empty(n, dtype=torch.uint8, device=self.device),
                                    torch.cuda.Event())
        else:
            slot[2].synchronize()
        self._cur = (slot[0][:nbytes], slot[1][:nbytes], slot[2])
        return self._cur[0]

    def upload(self):
        """Enqueue the copy of the staged bytes on the current stream; returns their device view."""
        host, dev, _ = self._cur
        dev.copy_(host, non_blocking=True)
        return dev

    def record(self):
        self._cur[2].record(torch.cuda.current_stream(self.device))


def launch(name, staging, table_bytes, sizes, device, *scalars):
    """Upload ``table_bytes`` (uint8 view of the table with one row per tensor) through ``staging`` and run entry point ``name`` over the
    chunk map of ``sizes`` on the current stream of ``device``."""
    bt, bc = chunk_maps(sizes, device)
    raw = torch.from_numpy(table_bytes)
    staging.stage(raw.numel(), 4096).copy_(raw)
    with torch.cuda.device(device):
        tab = staging.upload()
        L.call(name, C.c_void_p(tab.data_ptr()), C.c_void_p(bt.data_ptr()), C.c_void_p(bc.data_ptr()), int(bt.numel()), *scalars,
               L.stream(device))
        staging.record()
