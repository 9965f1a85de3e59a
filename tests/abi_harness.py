"""Calling the library's C entry points from a test with every buffer guarded (a plain helper module: tests/test_metrics_exact_gpu.py,
tests/test_image_exact_gpu.py and tests/test_elementwise_exact_gpu.py import it).

Every row: the shared reduction scratch is refilled with NaN before the call (a fold that reads a slot nobody wrote turns the result
into NaN); every input sits inside a NaN-filled allocation (a read outside the slice poisons the result instead of faulting); every
output sits inside a sentinel-filled allocation whose two margins are checked afterwards (In16 / Out16: fp16 NHWC maps, whole or as a
channel slice of a wider buffer whose other channels are guarded the same way); the call runs twice and the two results
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


class In16:
    """device copy of an fp16 NHWC map ``x`` [npix, c] whose pixels are ``ld`` halves apart and start at channel ``c0`` of the buffer
    (ld = c, c0 = 0: a whole map; ld > c: a channel slice of a wider buffer).  Everything round the slice -- the two margins and the
    other channels of every pixel -- is NaN: a read outside the slice poisons the result"""

    def __init__(self, x, ld=None, c0=0):
        x = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
        assert x.dim() == 2, "In16 takes [npix, c]"
        self.npix, self.c = x.shape
        self.ld = self.c if ld is None else ld
        assert self.ld % 8 == 0 and c0 % 8 == 0 and c0 + self.c <= self.ld          # the kernels move 16-byte octets
        h = x.to(torch.float16)
        assert torch.equal(h.double(), x.double()), "In16: the values are not fp16-exact"
        self.buf = torch.full((self.npix * self.ld + 2 * PAD,), float("nan"), dtype=torch.float16, device=_dev())
        self.v = self.buf[PAD:PAD + self.npix * self.ld].view(self.npix, self.ld)[:, c0:c0 + self.c]
        self.v.copy_(h)

    @property
    def ptr(self):
        return C.c_void_p(self.v.data_ptr())


class Out16:
    """an fp16 NHWC output [npix, c] in the same two layouts, inside a sentinel-filled allocation; ``init`` presets the slice (a
    previous gradient).  intact(): the margins AND every element of the buffer outside the slice still hold the sentinel"""

    def __init__(self, npix, c, ld=None, c0=0, init=None):
        self.npix, self.c, self.c0 = npix, c, c0
        self.ld = c if ld is None else ld
        assert self.ld % 8 == 0 and c0 % 8 == 0 and c0 + c <= self.ld
        self.buf = torch.full((npix * self.ld + 2 * PAD,), SENT, dtype=torch.float16, device=_dev())
        self.v = self.buf[PAD:PAD + npix * self.ld].view(npix, self.ld)[:, c0:c0 + c]
        if init is not None:
            h = torch.as_tensor(np.ascontiguousarray(init) if isinstance(init, np.ndarray) else init).reshape(npix, c)
            assert torch.equal(h.to(torch.float16).double(), h.double()), "Out16: the preset is not fp16-exact"
            self.v.copy_(h.to(torch.float16))

    @property
    def ptr(self):
        return C.c_void_p(self.v.data_ptr())

    def get(self):
        return self.v.cpu().numpy().copy()

    def intact(self):
        b = self.buf.cpu().numpy()
        body = b[PAD:PAD + self.npix * self.ld].reshape(self.npix, self.ld)
        return bool((b[:PAD] == SENT).all() and (b[PAD + self.npix * self.ld:] == SENT).all()
                    and (body[:, :self.c0] == SENT).all() and (body[:, self.c0 + self.c:] == SENT).all())


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
