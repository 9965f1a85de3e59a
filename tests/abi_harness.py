"""Calling the library's C entry points from a test with every buffer guarded (a plain helper module: tests/test_metrics_exact_gpu.py,
tests/test_image_exact_gpu.py, tests/test_elementwise_exact_gpu.py and tests/test_step_tail_exact_gpu.py import it).

Every row: the shared reduction scratch is refilled with NaN before the call (a fold that reads a slot nobody wrote turns the result
into NaN); every input sits inside a NaN-filled allocation (a read outside the slice poisons the result instead of faulting); every
output sits inside a sentinel-filled allocation whose two margins are checked afterwards (In16 / Out16: fp16 NHWC maps, whole or as a
channel slice of a wider buffer whose other channels are guarded the same way; In16Split: the two planes of a split map in one such
allocation); a table of structs or an index array sits inside an 0xFF-filled allocation and is compared byte for byte afterwards
(Raw); the call runs twice and the two results must be bit-identical.
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


class In16Split:
    """the two planes of a split map (hi + lo, both [npix, c] fp16-exact) in the layout of In16, inside ONE NaN-filled allocation with a
    NaN gap between them; ``lo`` is the distance of the planes in halves, as the split entry points take it"""

    def __init__(self, hi, lo, ld=None, c0=0):
        hi, lo = (torch.as_tensor(np.ascontiguousarray(a)) for a in (hi, lo))
        assert hi.dim() == 2 and hi.shape == lo.shape, "In16Split takes two [npix, c]"
        self.npix, self.c = hi.shape
        self.ld = self.c if ld is None else ld
        assert self.ld % 8 == 0 and c0 % 8 == 0 and c0 + self.c <= self.ld
        plane = self.npix * self.ld
        self.lo = plane + PAD
        self.buf = torch.full((2 * plane + 3 * PAD,), float("nan"), dtype=torch.float16, device=_dev())
        for k, x in enumerate((hi, lo)):
            h = x.to(torch.float16)
            assert torch.equal(h.double(), x.double()), "In16Split: the values are not fp16-exact"
            v = self.buf[PAD + k * self.lo:PAD + k * self.lo + plane].view(self.npix, self.ld)[:, c0:c0 + self.c]
            v.copy_(h)
            if k == 0:
                self.v = v

    @property
    def ptr(self):
        return C.c_void_p(self.v.data_ptr())


class Raw:
    """device copy of a host array's BYTES (a table of structs, an index array) in the middle of an allocation filled with 0xFF (NaN as a
    float, -1 as an index), 256 bytes either side; unchanged(): the device still holds exactly these bytes, margins included"""

    def __init__(self, arr):
        self.host = torch.from_numpy(np.frombuffer(np.ascontiguousarray(arr).tobytes(), dtype=np.uint8).copy())
        n = self.host.numel()
        self.buf = torch.full((n + 512,), 0xFF, dtype=torch.uint8, device=_dev())
        self.v = self.buf[256:256 + n]
        self.v.copy_(self.host)

    @property
    def ptr(self):
        return C.c_void_p(self.v.data_ptr())

    def unchanged(self):
        b = self.buf.cpu()
        n = self.host.numel()
        return bool(torch.equal(b[256:256 + n], self.host) and (b[:256] == 0xFF).all() and (b[256 + n:] == 0xFF).all())


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
