"""Prediction batches out of an HBM-resident set of unlabeled LR images of any size: the counterpart of resident_test.py for
``TTICrackDataSetTest`` + ``TestTransforms`` + ``SplitPatch`` (model/data/crack_dataset.py:145-172) behind ``test.py --tti_crack_dataset``.

The reference unfolds every LR image into ``IMAGE_SIZE`` patches -- the remainder rows and columns are silently dropped -- and convolves
each patch with zero padding at its own border.  Here ``plan_tiles`` is the single place that knows the tiling: a ceil grid of cores whose
last row / column is shifted inward, so every pixel has exactly one owner and every core reads real pixels, and an optional halo of real
context around every core, so all windows of all images have ONE size.  The decoded uint8 images live in one pool laid out like the pools of
resident_test.py; the windows are rows of the EXISTING ``csbsr_gather_crop_u8`` (csrc/resident.hip), whose per-pixel clamp replicates the
border for a window that leaves the image; the rows of ``csbsr_stitch_tiles_u8`` (csrc/eval_io.hip) say which rectangle of which output
patch goes where.  Both tables are built once per loader and stay on the device.  Iterating touches no host pixel.

No CPU / torch fallback: batches exist on a GPU only (construction, planning and grouping also work on ``device="cpu"``, for the host-side
tests).
"""
import glob
import os
from collections import namedtuple

import numpy as np
import torch

from .. import _lib as L
from .pool import U8Pool, decode_u8


def plan_tiles(h, w, ph, pw, halo, scale, index=0):
    """The tiling of one ``h x w`` LR image into cores of ``ph x pw`` with ``halo`` pixels of context, as two int32 tables with one row per
    tile, row-major over the grid ``ceil(h / ph) x ceil(w / pw)`` (the reference's patch order):

      gather [n][5] = (index, y0, x0, 0, 0)                          rows of csbsr_gather_crop_u8, LR pixels: the window's origin
      stitch [n][8] = (index, dst_y, dst_x, src_y, src_x, th, tw, 0)   rows of csbsr_stitch_tiles_u8, HR (x ``scale``) pixels

    Tile (iy, ix) owns rows [iy * ph, min((iy + 1) * ph, h)) and the matching columns; its core starts at min(iy * ph, max(h - ph, 0)), so
    the last row / column of cores is shifted inward instead of padded (an image smaller than a core keeps origin 0); its window is the core
    grown by ``halo`` on every side: (ph + 2 halo) x (pw + 2 halo) for every tile.  dst = scale * owned origin, src = scale * (owned origin
    - window origin), th, tw = scale * owned size.  With halo 0 and h, w multiples of ph, pw this is SplitPatch's unfold."""
    h, w, ph, pw, halo, scale = (int(v) for v in (h, w, ph, pw, halo, scale))
    if min(h, w, ph, pw, scale) < 1 or halo < 0:
        raise ValueError(f"plan_tiles: image {h} x {w}, core {ph} x {pw}, halo {halo}, scale {scale}")
    ny, nx = -(-h // ph), -(-w // pw)
    iy, ix = (v.reshape(-1) for v in np.divmod(np.arange(ny * nx, dtype=np.int64), nx))
    oy, ox = iy * ph, ix * pw                                           # owned origin
    oh, ow = np.minimum(oy + ph, h) - oy, np.minimum(ox + pw, w) - ox   # owned size
    wy, wx = np.minimum(oy, max(h - ph, 0)) - halo, np.minimum(ox, max(w - pw, 0)) - halo      # window origin
    z, idx = np.zeros_like(iy), np.full_like(iy, int(index))
    gather = np.stack([idx, wy, wx, z, z], axis=1)
    stitch = np.stack([idx, scale * oy, scale * ox, scale * (oy - wy), scale * (ox - wx), scale * oh, scale * ow, z], axis=1)
    PH, PW, H, W = scale * (ph + 2 * halo), scale * (pw + 2 * halo), scale * h, scale * w
    s = stitch
    ok = ((s[:, 3:5] >= 0).all() and (s[:, 5:7] > 0).all() and (s[:, 3] + s[:, 5] <= PH).all() and (s[:, 4] + s[:, 6] <= PW).all()
          and (s[:, 1:3] >= 0).all() and (s[:, 1] + s[:, 5] <= H).all() and (s[:, 2] + s[:, 6] <= W).all())
    # exact cover: the owned rectangles are the cells of a grid, so it is enough that the row bands and the column bands partition [0, H), [0, W)
    rows, cols = s[::nx], s[:nx]
    ok = ok and rows[0, 1] == 0 and (rows[1:, 1] == rows[:-1, 1] + rows[:-1, 5]).all() and rows[-1, 1] + rows[-1, 5] == H
    ok = ok and cols[0, 2] == 0 and (cols[1:, 2] == cols[:-1, 2] + cols[:-1, 6]).all() and cols[-1, 2] + cols[-1, 6] == W
    ok = ok and (s.reshape(ny, nx, 8)[:, :, [1, 5]] == rows[:, None, [1, 5]]).all() and (s.reshape(ny, nx, 8)[:, :, [2, 6]] == cols[None, :, [2, 6]]).all()
    if not ok or max(H, W, PH, PW) >= 1 << 24:
        raise ValueError(f"plan_tiles: no valid tiling of {h} x {w} with core {ph} x {pw}, halo {halo}, scale {scale}")
    return gather.astype(np.int32), stitch.astype(np.int32)


class ResidentImageSet:
    """Unlabeled LR images held in HBM: uint8 arrays h x w x 3 as PIL decodes them (sizes may differ) and their file names, packed into one
    pool with the int64 byte-offset table and the int32 (h, w) table ``csbsr_gather_crop_u8`` reads."""

    def __init__(self, images, names, device="cuda:0"):
        if len(images) == 0 or len(images) != len(names):
            raise ValueError(f"{len(images)} images, {len(names)} names")
        self.device = torch.device(device)
        self.names = [str(s) for s in names]
        self.lr = U8Pool(images, 3, "LR image", self.device)

    @classmethod
    def from_dir(cls, image_dir, pattern="*.png", device="cuda:0"):
        """Decode ``image_dir/<pattern>`` once with PIL, in sorted order (the reference takes ``Path.glob``'s order).  Files are taken as
        PIL decodes them, without mode conversion; one that does not decode to 8-bit RGB is an error that names the file."""
        names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(image_dir, pattern)))
        if not names:
            raise FileNotFoundError(f"no {pattern} under {image_dir}")
        images = [decode_u8(os.path.join(image_dir, n), 3, "8-bit RGB (h x w x 3)", wrap=True) for n in names]
        return cls(images, names, device=device)

    def __len__(self):
        return len(self.names)

    @property
    def nbytes(self):
        return int(self.lr.pool.numel())


# images [i0, i1), tile rows [t0, t1) of the loader's tables, output pixels (sum of H * W) of the unit
PredictUnit = namedtuple("PredictUnit", "i0 i1 t0 t1 npix")


class DevicePredictLoader:
    """Work units over a ``ResidentImageSet``.  ``patch`` = (ph, pw) is the LR core, ``halo`` the LR context around it: the model sees
    windows of (ph + 2 halo) x (pw + 2 halo) and returns ``scale`` times that.  A unit is a run of consecutive images whose tiles together
    number at most ``batch_patches``, or one image with more tiles than that; ``batches(unit)`` yields its model inputs, never more than
    ``batch_patches`` windows at a time.

    Tables, built once (host copies ``gather``, ``stitch``, ``out_dims``, ``pix_offsets`` beside the device ones):
      gather_dev int32 [T][5], stitch_dev int32 [T][8]   ``plan_tiles`` of every image, image column = index in the set
      out_dims_dev int32 [n][2]                           (scale h, scale w)
      off1_dev, off3_dev int64 [n]                        first element of image i in its UNIT's 1- and 3-channel output pools
    Iterating yields the ``PredictUnit`` tuples."""

    def __init__(self, imageset, patch, scale, halo=0, batch_patches=16):
        self.imageset, self.scale, self.halo, self.batch_patches = imageset, int(scale), int(halo), int(batch_patches)
        if self.scale == 1:
            raise NotImplementedError("SCALE_FACTOR 1 is not implemented on the device path")
        if self.scale < 1 or self.batch_patches < 1 or self.halo < 0:
            raise ValueError("scale and batch_patches must be positive, halo not negative")
        self.ph, self.pw = (int(patch), int(patch)) if np.isscalar(patch) else (int(patch[0]), int(patch[1]))
        if self.ph < 1 or self.pw < 1:
            raise ValueError(f"patch {self.ph} x {self.pw}")
        self.wh, self.ww = self.ph + 2 * self.halo, self.pw + 2 * self.halo            # the window the model sees, LR
        self.device, self.names = imageset.device, imageset.names
        dims = imageset.lr.dims.astype(np.int64)
        plans = [plan_tiles(d[0], d[1], self.ph, self.pw, self.halo, self.scale, index=i) for i, d in enumerate(dims)]
        self.gather = np.concatenate([p[0] for p in plans])
        self.stitch = np.concatenate([p[1] for p in plans])
        self.tile_start = np.concatenate([[0], np.cumsum([len(p[0]) for p in plans])]).astype(np.int64)
        self.out_dims = (dims * self.scale).astype(np.int32)
        npix = self.out_dims[:, 0].astype(np.int64) * self.out_dims[:, 1]
        self.units, self.pix_offsets = [], np.zeros(len(dims), np.int64)
        i0 = 0
        while i0 < len(dims):                                   # greedy: as many consecutive images as fit into one model call
            i1 = i0 + 1
            while i1 < len(dims) and self.tile_start[i1 + 1] - self.tile_start[i0] <= self.batch_patches:
                i1 += 1
            self.pix_offsets[i0:i1] = np.cumsum(npix[i0:i1]) - npix[i0:i1]
            self.units.append(PredictUnit(i0, i1, int(self.tile_start[i0]), int(self.tile_start[i1]), int(npix[i0:i1].sum())))
            i0 = i1
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.gather_dev, self.stitch_dev, self.out_dims_dev = dev(self.gather), dev(self.stitch), dev(self.out_dims)
        self.off1_dev, self.off3_dev = dev(self.pix_offsets), dev(self.pix_offsets * 3)

    @classmethod
    def from_cfg(cls, cfg, imageset, halo=0, batch_patches=16):
        """INPUT.IMAGE_SIZE is the LR patch here, as in TTICrackDataSetTest (``SplitPatch(batch_size, 3, *cfg.INPUT.IMAGE_SIZE)``, not
        divided by the scale as CrackDataSetTest divides it); MODEL.SCALE_FACTOR is the scale."""
        return cls(imageset, tuple(cfg.INPUT.IMAGE_SIZE), cfg.MODEL.SCALE_FACTOR, halo=halo, batch_patches=batch_patches)

    def __len__(self):
        return len(self.units)

    def __iter__(self):
        return iter(self.units)

    def chunks(self, unit):
        """The tile-row ranges [a, b) of the unit's model calls."""
        return [(a, min(a + self.batch_patches, unit.t1)) for a in range(unit.t0, unit.t1, self.batch_patches)]

    def batches(self, unit):
        """Yields (imgs fp32 [b - a, 3, wh, ww] on the device, a, b) per model call of ``unit``."""
        if self.device.type != "cuda":
            raise L.CsbsrHipError("DevicePredictLoader needs the image set on a GPU: csbsr_amd has no fallback path")
        L.load()
        for a, b in self.chunks(unit):
            yield self.imageset.lr.gather(self.gather_dev[a:b], b - a, self.wh, self.ww), a, b
