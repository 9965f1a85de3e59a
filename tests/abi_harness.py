"""Calling the library's C entry points from a test with every buffer guarded (a plain helper module: tests/test_metrics_exact_gpu.py
and tests/test_image_exact_gpu.py import it).

Every row: the shared reduction scratch is refilled with NaN before the call (a fold that reads a slot nobody wrote turns the result
into NaN); every input sits inside a NaN-filled allocation (a read outside the slice poisons the result instead of faulting); every
output sits inside a sentinel-filled allocation whose two margins are checked afterwards; the call runs twice and the two results
must be bit-identical.
"""
import ctypes as C

import numpy as np
import torch

PAD = 64                     # elements either side of every slice (keeps the slices 256-byte aligned like torch's own allocations)
SENT = -7.25                 # margin value of float outputs (fp16-exact, so that it serves fp16 outputs too)
ISENT = 0x5A5A5A5A           # ... of integer outputs


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def inp(x):
    """device copy of ``x`` (flattened) in the middle of a NaN-filled allocation"""
    if x is None:
        return None
    x = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x).to(torch.float32).reshape(-1)
    buf = torch.full((x.numel() + 2 * PAD,), float("nan"), dtype=torch.float32, device=_dev())
    v = buf[PAD:PAD + x.numel()]
    v.copy_(x)
    return v


class Out:
    """an output slice of ``n`` elements in the middle of a sentinel-filled allocation; ``init`` presets the slice (zeroed sums, a
    previous gradient), otherwise it holds the sentinel too and the kernel has to write all of it"""

    def __init__(self, n, dtype=torch.float32, init=None):
        self.sent = SENT if dtype.is_floating_point else ISENT
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), self.sent, dtype=dtype, device=_dev())
        self.v = self.buf[PAD:PAD + n]
        if init is not None:
            self.v.copy_(torch.as_tensor(init).reshape(-1)) if not np.isscalar(init) else self.v.fill_(init)

    @property
    def ptr(self):
        return _ptr(self.v)

    def get(self, *shape):
        return self.v.cpu().numpy().copy().reshape(shape if shape else (self.n,))

    def margins_intact(self):
        b = self.buf.cpu().numpy()
        return bool((b[:PAD] == self.sent).all() and (b[PAD + self.n:] == self.sent).all())

    def untouched(self):
        return bool((self.buf.cpu().numpy() == self.sent).all())


def call(name, *args):
    """one call into the library on a NaN-refilled reduction scratch"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import _reduction_scratch
    _reduction_scratch(_dev()).fill_(float("nan"))
    L.call(name, *args, _stream())
    torch.cuda.synchronize()


def same_bits(a, b):
    u = np.uint16 if a.dtype == np.float16 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


def twice(fn):
    """run a row twice; both runs must agree bit for bit"""
    r1, r2 = fn(), fn()
    for k in r1:
        assert same_bits(r1[k], r2[k]), f"{k}: two runs of the same call differ"
    return r1
