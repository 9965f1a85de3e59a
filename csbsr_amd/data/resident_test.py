"""Evaluation batches out of an HBM-resident test set: the counterpart of resident.py for ``CrackDataSetTest`` + ``TestTransforms`` +
``SplitPatch`` (model/data/crack_dataset.py:71-142, model/data/transforms/data_preprocess.py:48-60, model/data/samplers/patch_sampler.py)
behind test.py's ``SequentialSampler`` / ``BatchSampler(drop_last=False)`` (test.py:56-81).

The reference decodes four files per image in the loader, converts them to fp32 on the host, unfolds the LR image into patches and lets the
DataLoader collate pageable tensors.  Here the decoded uint8 pixels of the whole test set live on the device in three pools (HR image, mask,
LR image); a batch is three launches of the EXISTING ``csbsr_gather_crop_u8`` (csrc/resident.hip) over selection tables that are built once
per loader and stay on the device: one row ``(index, iy * ph, ix * pw, 0, 0)`` per LR patch, one row ``(index, 0, 0, 0, 0)`` per full HR
image / mask.  The kernel targets -- 441 values per image -- are computed once on the host by the reference's own expression and kept in
HBM as fp32.  Iterating touches no host pixel.

No CPU / torch fallback: batches exist on a GPU only (construction and validation also work on ``device="cpu"``, for the host-side tests).
"""
import glob
import os

import numpy as np
import torch

from .. import _lib as L
from .pool import U8Pool, _as_hwc, decode_u8

_U8Pool = U8Pool          # (the name this module had it under)


def kernel_target(kernel_u8):
    """uint8 K x K -> fp32 [1, K, K], by the reference's own expression on the host (crack_dataset.py:96-98 through TestTransforms):
    ``k = u8 / 255`` in fp32, then ``k / torch.sum(k)``."""
    k = torch.from_numpy(np.ascontiguousarray(kernel_u8)[:, :, np.newaxis].astype(np.float32)).permute(2, 0, 1) / 255
    return k / torch.sum(k)


class ResidentTestSet:
    """The test set of ``CrackDataSetTest`` held in HBM.  Arguments are lists of uint8 arrays as PIL decodes the files: HR images
    H x W x 3, masks H x W, LR images h x w x 3, blur kernels K x K (one K for the whole set), and the HR file names.  Sizes may differ
    between samples; what a loader can batch is the loader's check."""

    def __init__(self, hr_images, masks, lr_images, kernels, names, device="cuda:0"):
        n = len(hr_images)
        if n == 0 or not (len(masks) == len(lr_images) == len(kernels) == len(names) == n):
            raise ValueError(f"{n} images, {len(masks)} masks, {len(lr_images)} LR images, {len(kernels)} kernels, {len(names)} names")
        self.device = torch.device(device)
        self.names = [str(s) for s in names]
        self.hr = U8Pool(hr_images, 3, "image", self.device)
        self.mask = U8Pool(masks, 1, "mask", self.device)
        self.lr = U8Pool(lr_images, 3, "LR image", self.device)
        for i in range(n):
            if tuple(self.hr.dims[i]) != tuple(self.mask.dims[i]):
                raise ValueError(f"{self.names[i]}: image {tuple(self.hr.dims[i])} and mask {tuple(self.mask.dims[i])} differ in size")
        ks = [_as_hwc(k, 1, f"kernel {i}")[:, :, 0] for i, k in enumerate(kernels)]
        K = ks[0].shape[0]
        for i, k in enumerate(ks):
            if k.shape != (K, K):
                raise ValueError(f"kernel of {self.names[i]}: {k.shape}, expected {K} x {K} like the first")
        self.K = int(K)
        self.kernel_targets = torch.cat([kernel_target(k) for k in ks]).contiguous().to(self.device)        # fp32 [n][K][K]

    @classmethod
    def from_dirs(cls, image_dir, mask_dir, blur_dir, blur_name, device="cuda:0"):
        """Decode once with PIL, the reference's layout: names from ``image_dir/*.jpg`` (sorted), the same name under ``mask_dir``, the LR
        image and the kernel at ``<blur_dir>/<blur_name>/lr_images|kernels/<name with jpg -> png>``.  Files are taken as PIL decodes them,
        without mode conversion; one that does not decode to the expected 8-bit layout is an error that names the file."""
        names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(image_dir, "*.jpg")))
        if not names:
            raise FileNotFoundError(f"no *.jpg under {image_dir}")
        out = ([], [], [], [])
        for n in names:
            png = n.replace("jpg", "png")                       # (crack_dataset.py:94: every occurrence, as there)
            paths = (os.path.join(image_dir, n), os.path.join(mask_dir, n), os.path.join(blur_dir, blur_name, "lr_images", png),
                     os.path.join(blur_dir, blur_name, "kernels", png))
            for p, ndim, what, dst in zip(paths, (3, 2, 3, 2), ("8-bit RGB (H x W x 3)", "8-bit single-channel (H x W)",
                                                                "8-bit RGB (h x w x 3)", "8-bit single-channel (K x K)"), out):
                if not os.path.isfile(p):
                    raise FileNotFoundError(f"{p} (of image {paths[0]}) is missing")
                dst.append(decode_u8(p, ndim, what))
        return cls(*out, names, device=device)

    def __len__(self):
        return len(self.names)

    @property
    def nbytes(self):
        return int(self.hr.pool.numel() + self.mask.pool.numel() + self.lr.pool.numel() + 4 * self.kernel_targets.numel())


class DeviceTestLoader:
    """Iterating yields ``(imgs [B,nPatch,3,ph,pw], sr_targets [B,3,H,W], masks [B,1,H,W], kernel_targets [B,nPatch,K,K], fnames,
    img_unfold_shape, seg_unfold_shape)`` -- what the reference's DataLoader collates from ``CrackDataSetTest``, all tensors on the device,
    ``fnames`` the ``.png`` names, the two shapes the 1-D int arrays of crack_dataset.py:109-112 (entry 0 the constructor's ``batch_size``,
    entries 5 and 6 scaled by ``scale``, entries 1 and 4 of the segmentation shape ``num_classes``): the arguments of
    ``csbsr_amd.inference.evaluate_batch``.  Order is sequential and the last batch may be short.  ``ph, pw = int(image_size / scale)``.

    Checked at construction, with the file names in the message: H and W are multiples of ``image_size`` (the reference's unfold would
    silently drop the remainder and then fail in PSNR), the LR image is H / scale x W / scale, and the images of one batch have one size."""

    def __init__(self, testset, image_size, scale, batch_size, num_classes=1):
        self.testset, self.scale, self.batch_size, self.num_classes = testset, int(scale), int(batch_size), int(num_classes)
        if self.scale == 1:
            raise NotImplementedError("SCALE_FACTOR 1 (the test images themselves as the input) is not implemented on the device path")
        if self.scale < 1 or self.batch_size < 1:
            raise ValueError("scale and batch_size must be positive")
        ih, iw = (int(image_size), int(image_size)) if np.isscalar(image_size) else (int(image_size[0]), int(image_size[1]))
        self.ph, self.pw = int(ih / self.scale), int(iw / self.scale)
        if self.ph < 1 or self.pw < 1 or self.ph * self.scale != ih or self.pw * self.scale != iw:
            raise ValueError(f"image_size {ih} x {iw} must be positive multiples of the scale {self.scale}")
        names, hr, lr = testset.names, testset.hr.dims.astype(np.int64), testset.lr.dims.astype(np.int64)
        bad = [n for n, d in zip(names, hr) if d[0] % ih or d[1] % iw]
        if bad:
            raise ValueError(f"image size is not a multiple of IMAGE_SIZE {ih} x {iw}: {', '.join(bad)}")
        bad = [n for n, d, e in zip(names, hr, lr) if d[0] != e[0] * self.scale or d[1] != e[1] * self.scale]
        if bad:
            raise ValueError(f"LR image is not the image size / {self.scale}: {', '.join(bad)}")
        self.batches = []                                       # (first image, one past the last, first patch row)
        patch_rows, row = [], 0
        for i0 in range(0, len(names), self.batch_size):
            i1 = min(i0 + self.batch_size, len(names))
            if (hr[i0:i1] != hr[i0]).any():
                raise ValueError(f"the images of one batch differ in size: {', '.join(names[i0:i1])}")
            nH, nW = int(hr[i0, 0] // ih), int(hr[i0, 1] // iw)
            iy, ix = np.divmod(np.arange(nH * nW), nW)
            for i in range(i0, i1):
                patch_rows.append(np.stack([np.full(nH * nW, i), iy * self.ph, ix * self.pw, 0 * iy, 0 * iy], axis=1))
            self.batches.append((i0, i1, row))
            row += (i1 - i0) * nH * nW
        self.device = testset.device
        full = np.zeros((len(names), 5), np.int32)
        full[:, 0] = np.arange(len(names))
        self.patch_sel = torch.from_numpy(np.concatenate(patch_rows).astype(np.int32)).to(self.device)
        self.full_sel = torch.from_numpy(full).to(self.device)
        self.fnames = [n.replace("jpg", "png") for n in names]

    @classmethod
    def from_cfg(cls, cfg, testset, batch_size):
        """INPUT.IMAGE_SIZE, MODEL.SCALE_FACTOR and MODEL.NUM_CLASSES of a reference-style config tree; the batch size is test.py's
        command-line argument."""
        return cls(testset, tuple(cfg.INPUT.IMAGE_SIZE), cfg.MODEL.SCALE_FACTOR, batch_size, num_classes=cfg.MODEL.NUM_CLASSES)

    def __len__(self):
        return len(self.batches)

    def unfold_shapes(self, i0):
        """(img_unfold_shape, seg_unfold_shape) of the batch that starts at image ``i0``."""
        H, W = (int(v) for v in self.testset.hr.dims[i0])
        ih, iw = self.ph * self.scale, self.pw * self.scale
        img = np.array([self.batch_size, 1, H // ih, W // iw, 3, ih, iw], dtype=np.int64)
        seg = img.copy()
        seg[[1, 4]] = self.num_classes
        return img, seg

    def __iter__(self):
        ts = self.testset
        if self.device.type != "cuda":
            raise L.CsbsrHipError("DeviceTestLoader needs the test set on a GPU: csbsr_amd has no fallback path")
        L.load()
        for i0, i1, row in self.batches:
            B = i1 - i0
            img_shape, seg_shape = self.unfold_shapes(i0)
            nP, H, W = int(img_shape[2] * img_shape[3]), int(ts.hr.dims[i0, 0]), int(ts.hr.dims[i0, 1])
            imgs = ts.lr.gather(self.patch_sel[row:row + B * nP], B * nP, self.ph, self.pw).view(B, nP, 3, self.ph, self.pw)
            sr_targets = ts.hr.gather(self.full_sel[i0:i1], B, H, W)
            masks = ts.mask.gather(self.full_sel[i0:i1], B, H, W)
            kt = ts.kernel_targets[i0:i1, None].expand(B, nP, ts.K, ts.K).contiguous()
            yield imgs, sr_targets, masks, kt, self.fnames[i0:i1], img_shape, seg_shape
