"""The one uint8 pool of the HBM-resident datasets (resident.py, resident_test.py, resident_predict.py), the host validation of the
tables its gather kernels read (csrc/resident.hip) and the PIL decode of one file.  No CPU / torch fallback: a gather exists on a GPU only
(construction, ``sample`` and ``check_rows`` also work on ``device="cpu"``)."""
import numpy as np
import torch

from .. import _lib as L
from ..engine import _ptr


def _as_hwc(a, channels, what):
    a = np.asarray(a)
    if a.dtype != np.uint8:
        raise TypeError(f"{what}: expected uint8, got {a.dtype}")
    if channels == 1 and a.ndim == 2:
        a = a[:, :, None]
    if a.ndim != 3 or a.shape[2] != channels or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"{what}: expected H x W x {channels}, got {a.shape}")
    return a


def decode_u8(path, ndim, expected_text, what="", wrap=False):
    """``np.array(Image.open(path))`` as PIL decodes the file, without mode conversion; one that is not 8-bit of rank ``ndim`` (2: H x W,
    3: H x W x 3) is a ValueError that names the file (``what`` goes in front of the path) and says ``expected_text``.  ``wrap`` turns
    a failure of the decode itself into a ValueError too; otherwise PIL's exception passes through."""
    from PIL import Image
    try:
        a = np.array(Image.open(path))
    except Exception as e:
        if not wrap:
            raise
        raise ValueError(f"{path} does not decode: {e}") from e
    if a.dtype != np.uint8 or a.ndim != ndim or (ndim == 3 and a.shape[2] != 3):
        raise ValueError(f"{what}{path} decodes to {a.dtype} {a.shape}, expected {expected_text}")
    return a


class U8Pool:
    """uint8 H x W x C arrays packed back to back into one contiguous device pool, with the int64 byte-offset table and the int32 (H, W)
    table ``csbsr_gather_crop_u8`` and ``csbsr_gather_resize_u8`` read."""

    def __init__(self, arrays, channels, what, device):
        arrays = [_as_hwc(a, channels, f"{what} {i}") for i, a in enumerate(arrays)]
        self.channels, self.device = channels, torch.device(device)
        self.dims = np.array([a.shape[:2] for a in arrays], dtype=np.int32)                # host copy: table validation
        px = self.dims[:, 0].astype(np.int64) * self.dims[:, 1] * channels
        self.offsets = np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)
        self.pool = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).to(self.device)
        self.dims_dev = torch.from_numpy(self.dims).to(self.device)
        self.offsets_dev = torch.from_numpy(self.offsets).to(self.device)

    def sample(self, p):
        """uint8 H x W x C numpy copy of array ``p``."""
        H, W = (int(v) for v in self.dims[p])
        o = int(self.offsets[p])
        return self.pool[o:o + H * W * self.channels].cpu().numpy().reshape(H, W, self.channels)

    def check_rows(self, sel, h, w, what):
        """Raise unless every row of ``sel`` names a pooled array and a window inside it.  ``what`` = "selection": rows (index, y0, x0,
        mirror, vflip), an h x w window.  ``what`` = "window": rows (..., hs, ws), an hs x ws window that csbsr_gather_resize_u8 may resample
        to h x w: 1 <= hs <= 8 h, 1 <= ws <= 8 w (17 taps per axis).  The kernels clamp a bad row silently, so this runs before every upload."""
        cols = 7 if what == "window" else 5
        s = np.asarray(sel)
        if s.ndim != 2 or s.shape[1] != cols or s.shape[0] < 1 or not np.issubdtype(s.dtype, np.integer):
            raise ValueError(f"{what} table must be integer [B][{cols}], got {s.dtype} {s.shape}")
        s = s.astype(np.int64)
        bad = (s[:, 0] < 0) | (s[:, 0] >= len(self.dims))
        if bad.any():
            raise ValueError(f"{what} row {int(np.flatnonzero(bad)[0])}: image index {int(s[bad][0, 0])} outside the pool of {len(self.dims)}")
        d = self.dims[s[:, 0]].astype(np.int64)
        hs, ws = (s[:, 5], s[:, 6]) if cols == 7 else (np.full(len(s), h), np.full(len(s), w))
        bad = (hs < 1) | (ws < 1)
        if cols == 7 and bad.any():
            r = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{what} row {r}: window size {int(hs[r])} x {int(ws[r])} must be at least 1 x 1")
        bad = (s[:, 1] < 0) | (s[:, 1] + hs > d[:, 0]) | (s[:, 2] < 0) | (s[:, 2] + ws > d[:, 1])
        if bad.any():
            r = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{what} row {r}: window y0 {int(s[r, 1])} x0 {int(s[r, 2])} of {int(hs[r])} x {int(ws[r])} leaves image "
                             f"{int(s[r, 0])} ({int(d[r, 0])} x {int(d[r, 1])})")
        bad = (hs > 8 * h) | (ws > 8 * w)
        if cols == 7 and bad.any():
            r = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{what} row {r}: window {int(hs[r])} x {int(ws[r])} is more than 8 times the output {h} x {w}")
        bad = ((s[:, 3] != 0) & (s[:, 3] != 1)) | ((s[:, 4] != 0) & (s[:, 4] != 1))
        if bad.any():
            raise ValueError(f"{what} row {int(np.flatnonzero(bad)[0])}: mirror / vflip must be 0 or 1")

    def _out(self, B, h, w):
        if self.device.type != "cuda":
            raise L.CsbsrHipError("the resident test set needs its pools on a GPU to make a batch: csbsr_amd has no fallback path")
        return torch.empty(B, self.channels, h, w, dtype=torch.float32, device=self.device)

    def gather(self, sel_dev, B, h, w):
        """fp32 [B, channels, h, w] = pool bytes / 255 for the int32 [B][5] device table ``sel_dev`` (rows built from ``dims``)."""
        out = self._out(B, h, w)
        with torch.cuda.device(self.device):
            L.call("csbsr_gather_crop_u8", _ptr(self.pool), _ptr(self.offsets_dev), _ptr(self.dims_dev), self.channels, _ptr(sel_dev),
                   B, h, w, _ptr(out), L.stream(self.device))
        return out

    def gather_resized(self, sel_dev, B, h, w, antialias=True):
        """fp32 [B, channels, h, w]: the hs x ws window of each row of the int32 [B][7] device table ``sel_dev`` (validated by the caller,
        check_rows) resampled to h x w like F.interpolate(mode="bilinear", antialias=antialias), / 255."""
        if tuple(sel_dev.shape) != (B, 7) or sel_dev.dtype != torch.int32 or not sel_dev.is_contiguous():
            raise ValueError(f"window table must be a contiguous int32 [{B}][7] tensor, got {sel_dev.dtype} {tuple(sel_dev.shape)}")
        out = self._out(B, h, w)
        with torch.cuda.device(self.device):
            L.call("csbsr_gather_resize_u8", _ptr(self.pool), _ptr(self.offsets_dev), _ptr(self.dims_dev), self.channels, _ptr(sel_dev),
                   B, h, w, int(bool(antialias)), _ptr(out), L.stream(self.device))
        return out
