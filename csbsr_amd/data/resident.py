"""Training batches out of an HBM-resident dataset: index -> mirror -> crop -> /255 -> blur kernel -> blur -> bicubic down -> SDF.

The reference feeds ``JointModelWithLoss`` from ``CrackDataSet.__getitem__`` in loader worker processes (train.py:57-63,
model/data/crack_dataset.py:40-64): a PIL decode, numpy flips, a crop, ``image / 255``, a blur on "cuda" from inside the worker, a
bicubic resize and a pageable fp32 copy of four tensors per sample.  Here the decoded uint8 pixels of the whole dataset live on the
device (10^4 images of 448^2 are 6 GB of pixels + 2 GB of masks), a batch is selected by ONE kernel per pool
(``csbsr_gather_crop_u8``, csrc/resident.hip) on the training stream, and everything after the gathered ``hr`` / ``mask`` is
``csbsr_amd.data.degrade.DeviceDegradation`` unchanged.  Per step the host contributes a table of 32 bytes per sample through a pinned
staging buffer: no worker process, no pixel traffic over PCIe, no host float conversion, no wait for the batch's own device work.

``resized_crop=`` (or a non-identity ``RandomResizedCrop`` entry of the augmentation list) turns the fixed-size window into the
reference's RandomResizedCrop (transforms.py:607-622): a window of random area and aspect per sample, resampled to the crop size by
``csbsr_gather_resize_u8`` in the same single launch per pool; the row per sample grows to 40 bytes.

Kernels: csbsr_gather_crop_u8, csbsr_gather_resize_u8 + those of DeviceDegradation.  No CPU / torch fallback: batches exist on a GPU only (the pool, the
sampler and the table validation also work on ``device="cpu"``, which is what the host-side tests use).
"""
import glob
import os

import numpy as np
import torch

from .. import _lib as L
from ..config.defaults import check_downscale
from ..engine import _ptr
from ..multi_tensor import Staging
from .degrade import DeviceDegradation
from .pool import U8Pool, _as_hwc, decode_u8          # noqa: F401  (_as_hwc stays importable from this module)

# cfg.DATASET.DATA_AUGMENTATION of the shipped config/config_csbsr_pspnet.yaml (yaml's bare None arrives as the string "None")
DEFAULT_AUGMENTATION = (("ConvertFromInts", None), ("RandomMirror", None), ("ToTensor", None), ("RandomVerticalFlip", 0.3), ("RandomCrop", None))

# every name `eval(func)` resolves in model/data/transforms/transforms.py: an entry with one of these names and a non-None argument is
# constructed and thrown away by TrainTransforms; any other name is a NameError there and a NotImplementedError here
_REFERENCE_TRANSFORMS = frozenset((
    "Compose", "RandomResize", "Resize", "ToTensor", "ToNumpy", "ConvertFromInts", "ConvertToInts", "SubtractMeans", "Normalize",
    "Denormalize", "RandomSaturation", "RandomValue", "RandomHue", "RandomLightingNoise", "ConvertColor", "RandomContrast",
    "RandomBrightness", "RandomMirror", "SwapChannels", "PhotometricDistort", "Clamp", "CenterCrop", "ConstantPadding", "MakeHeatmap",
    "FactorResize", "RandomCrop", "PriorBox", "RandomResizedCrop", "RandomSampleCrop", "ToPercentCoords", "RandomVerticalFlip",
    "RandomGrayscale"))


def _is_none(a):
    return a is None or a == "None"


def interpret_augmentation(augmentation, crop, dims):
    """cfg.DATASET.DATA_AUGMENTATION -> {"mirror_p", "crop"}, read the way TrainTransforms.__init__ reads it
    (model/data/transforms/data_preprocess.py:17-28), quirks included:

      ConvertFromInts, ToTensor   folded into the gather kernel (uint8 -> fp32, HWC -> CHW)
      RandomMirror                p = 0.5 (np.random.randint(2))
      RandomCrop                  a crop of INPUT.IMAGE_SIZE at a uniform offset; its resized_crop to the same size is the identity
      RandomResizedCrop           scale (1, 1), ratio (1, 1) only, and only when every image already has the crop size (then it is the
                                  identity); anything else is NotImplementedError HERE: DeviceTrainLoader takes a non-identity entry
                                  out of the list itself (split_resized_crop) and hands this function a RandomCrop in its place
      any other entry with an argument (the yaml's ["RandomVerticalFlip", 0.3])
                                  the reference's ``else: eval(func)(args)`` constructs the transform and DROPS it: no effect there, none
                                  here.  Vertical flips are available through DeviceTrainLoader's explicit ``vflip_p``.
      unknown names, and argument-less transforms other than the three above
                                  NotImplementedError

    ``dims`` [n][2] are the (H, W) of the images the loader will draw from, ``crop`` = (h, w)."""
    h, w = crop
    out = {"mirror_p": 0.0, "crop": False}
    for entry in augmentation:
        func, args = entry
        if func not in _REFERENCE_TRANSFORMS:
            raise NotImplementedError(f"unknown augmentation {func!r}")
        acts = func in ("RandomResizedCrop", "RandomCrop") or (_is_none(args) and func not in ("ConvertFromInts", "ToTensor"))
        if out["crop"] and acts:           # (an entry the reference constructs and drops has no effect wherever it stands)
            raise NotImplementedError(f"{func!r} after the crop: the gather kernel crops last")
        if func == "RandomResizedCrop":
            kw = args[0] if isinstance(args, (list, tuple)) else args
            kw = dict(kw or {})
            scale, ratio = tuple(kw.get("scale", (0.5, 1.0))), tuple(kw.get("ratio", (1.0, 1.0)))
            if scale != (1.0, 1.0) or ratio != (1.0, 1.0) or not all(int(H) == h and int(W) == w for H, W in dims):
                raise NotImplementedError("RandomResizedCrop is supported only where it is the identity: scale (1, 1), ratio (1, 1) and "
                                          "every image already of the crop size")
            out["crop"] = True
        elif func == "RandomCrop":
            out["crop"] = True
        elif _is_none(args):
            if func == "RandomMirror":
                out["mirror_p"] = 0.5
            elif func not in ("ConvertFromInts", "ToTensor"):
                raise NotImplementedError(f"augmentation {func!r} is not implemented on the device path"
                                          + (" (use vflip_p)" if func == "RandomVerticalFlip" else ""))
        # else: constructed and dropped by the reference
    if not out["crop"] and not all(int(H) == h and int(W) == w for H, W in dims):
        raise ValueError("the augmentation list has no crop, so every image must already have the crop size")
    return out


def _resized_crop_args(rc):
    """{"scale": (lo, hi), "ratio": (lo, hi)} with the reference's class defaults (transforms.py:608) -> ((lo, hi), (lo, hi)), validated."""
    rc = dict(rc or {})
    unknown = set(rc) - {"scale", "ratio"}
    if unknown:
        raise ValueError(f"resized_crop: unknown keys {sorted(unknown)}")
    scale, ratio = tuple(float(v) for v in rc.get("scale", (0.5, 1.0))), tuple(float(v) for v in rc.get("ratio", (1.0, 1.0)))
    if len(scale) != 2 or not 0.0 < scale[0] <= scale[1] or not np.isfinite(scale[1]):
        raise ValueError(f"resized_crop: need 0 < scale_lo <= scale_hi, got {scale}")
    if len(ratio) != 2 or not 0.0 < ratio[0] <= ratio[1] or not np.isfinite(ratio[1]):
        raise ValueError(f"resized_crop: need 0 < ratio_lo <= ratio_hi, got {ratio}")
    return scale, ratio


def split_resized_crop(augmentation):
    """(augmentation', resized_crop): a ``RandomResizedCrop`` entry that is not the identity case of interpret_augmentation (scale or
    ratio other than (1, 1)) is replaced by ``("RandomCrop", None)`` -- so the ordering rules of interpret_augmentation still apply to
    the place it stood in -- and its scale / ratio are returned; (augmentation, None) when there is no such entry."""
    out, rc = [], None
    for entry in augmentation:
        func, args = entry
        if func == "RandomResizedCrop":
            kw = args[0] if isinstance(args, (list, tuple)) else args
            kw = dict(kw or {}) if not _is_none(kw) else {}
            scale, ratio = tuple(kw.get("scale", (0.5, 1.0))), tuple(kw.get("ratio", (1.0, 1.0)))
            if scale != (1.0, 1.0) or ratio != (1.0, 1.0):
                if rc is None:
                    rc = {"scale": scale, "ratio": ratio}
                out.append(("RandomCrop", None))          # (a second one is refused by interpret_augmentation: a crop after the crop)
                continue
        out.append(entry)
    return out, rc


class ResidentDataset:
    """uint8 images (H x W x 3) and masks (H x W or H x W x 1) packed back to back into one contiguous device pool per kind, with an
    int64 byte-offset table and an int32 (H, W) table.  Sizes may differ between samples, not within a pair.  ``subset`` / ``split``
    return views on the same pools.

    ``masks=None`` is the image-only dataset of SR pretraining (the reference's SRPretrainDataSet): there is no mask pool (``mask`` and its
    aliases are None), ``sample`` returns ``(image, None)``, the gathers return ``(hr, None)`` and a DeviceTrainLoader over it yields
    ``(x, hr, k)``."""

    def __init__(self, images, masks=None, device="cuda:0"):
        if (masks is not None and len(images) != len(masks)) or len(images) == 0:
            raise ValueError(f"{len(images)} images, {'no' if masks is None else len(masks)} masks")
        self.device = torch.device(device)
        self.image = U8Pool(images, 3, "image", self.device)
        self.mask = None if masks is None else U8Pool(masks, 1, "mask", self.device)
        for i, (a, m) in enumerate(zip(self.image.dims, () if self.mask is None else self.mask.dims)):
            if tuple(a) != tuple(m):
                raise ValueError(f"sample {i}: image {tuple(int(v) for v in a)} and mask {tuple(int(v) for v in m)} differ in size")
        # the pools' tensors and tables under this class's names (plain aliases: ``subset`` copies them with __dict__)
        self.image_pool, self.image_offsets, self.image_offsets_dev = self.image.pool, self.image.offsets, self.image.offsets_dev
        self.mask_pool, self.mask_offsets, self.mask_offsets_dev = (None, None, None) if self.mask is None else \
            (self.mask.pool, self.mask.offsets, self.mask.offsets_dev)
        self.dims, self.dims_dev = self.image.dims, self.image.dims_dev
        self.indices = np.arange(len(images), dtype=np.int64)                             # pool indices this view holds

    @classmethod
    def from_dirs(cls, image_dir, mask_dir, pattern="*.jpg", device="cuda:0"):
        """Decode once with PIL: file names from ``image_dir``, the same names under ``mask_dir`` (crack_dataset.py:33-47).  Files are
        taken as PIL decodes them, without mode conversion: an image that does not decode to 8-bit H x W x 3 (grey, palette, RGBA) or
        a mask that does not decode to 8-bit H x W (bilevel, RGB, 16-bit) is an error that names the file.  (A palette mask decodes to
        its 8-bit indices, here as in the reference's ``np.array(Image.open(...))``.)"""
        names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(image_dir, pattern)))
        if not names:
            raise FileNotFoundError(f"no {pattern} under {image_dir}")
        images, masks = [], []
        for n in names:
            mp = os.path.join(mask_dir, n)
            if not os.path.isfile(mp):
                raise FileNotFoundError(f"mask {mp} of image {os.path.join(image_dir, n)} is missing")
            images.append(decode_u8(os.path.join(image_dir, n), 3, "8-bit RGB (H x W x 3)", what="image "))       # as is, like the reference
            masks.append(decode_u8(mp, 2, "8-bit single-channel (H x W)", what="mask "))
        ds = cls(images, masks, device=device)
        ds.names = names
        return ds

    @classmethod
    def from_image_dir(cls, image_dir, pattern="*.png", device="cuda:0"):
        """The image-only dataset of SR pretraining: every ``pattern`` file under ``image_dir`` (the reference's SRPretrainDataSet globs
        ``*.png``), decoded once with PIL as ``from_dirs`` decodes its images."""
        names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(image_dir, pattern)))
        if not names:
            raise FileNotFoundError(f"no {pattern} under {image_dir}")
        ds = cls([decode_u8(os.path.join(image_dir, n), 3, "8-bit RGB (H x W x 3)", what="image ") for n in names], None, device=device)
        ds.names = names
        return ds

    def __len__(self):
        return len(self.indices)

    @property
    def nbytes(self):
        return int(self.image_pool.numel() + (0 if self.mask is None else self.mask_pool.numel()))

    def subset(self, indices):
        """A view on the same pools holding ``indices`` (positions in this view)."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError("subset index out of range")
        v = object.__new__(type(self))
        v.__dict__.update(self.__dict__)
        v.indices = self.indices[idx]
        return v

    def split(self, ratio, seed):
        """Two disjoint views of int(n * ratio) and n - int(n * ratio) samples (train.py:52-57), chosen by a seeded permutation."""
        n = len(self)
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed))).numpy()
        k = int(n * ratio)
        return self.subset(perm[:k]), self.subset(perm[k:])

    def sample(self, i):
        """(image H x W x 3, mask H x W x 1) uint8 numpy copies of sample ``i`` of this view; the mask is None without a mask pool."""
        p = int(self.indices[i])
        return self.image.sample(p), None if self.mask is None else self.mask.sample(p)

    def check_selection(self, sel, h, w):
        """Raise unless every row (index, y0, x0, mirror, vflip) of ``sel`` names a pooled image and an h x w window inside it."""
        self.image.check_rows(sel, h, w, "selection")

    def check_windows(self, sel, h, w):
        """The 7-column sibling: rows (..., hs, ws) with an hs x ws window inside the image that may be resampled to h x w."""
        self.image.check_rows(sel, h, w, "window")

    def gather_resized(self, sel_dev, B, h, w, antialias=True):
        """(hr [B,3,h,w], mask [B,1,h,w]) fp32: the hs x ws window of each row of the int32 [B][7] device table ``sel_dev`` (validated by
        the caller, check_windows) resampled to h x w like F.interpolate(mode="bilinear", antialias=antialias), / 255.  The mask goes
        through the same resample (transforms.py:619-620) and comes out soft; None, and no launch, without a mask pool."""
        if self.device.type != "cuda":
            raise L.CsbsrHipError("ResidentDataset.gather_resized needs the pool on a GPU: csbsr_amd has no fallback path")
        return self.image.gather_resized(sel_dev, B, h, w, antialias), None if self.mask is None else self.mask.gather_resized(sel_dev, B, h, w, antialias)

    def gather(self, sel_dev, B, h, w):
        """(hr [B,3,h,w], mask [B,1,h,w]) fp32 = pool bytes / 255 for the int32 [B][5] device table ``sel_dev`` (validated by the caller);
        the mask is None, and no launch, without a mask pool."""
        if self.device.type != "cuda":
            raise L.CsbsrHipError("ResidentDataset.gather needs the pool on a GPU: csbsr_amd has no fallback path")
        return self.image.gather(sel_dev, B, h, w), None if self.mask is None else self.mask.gather(sel_dev, B, h, w)


_ROW = 32          # staged bytes per sample: int32 [5] selection row, then fp32 [3] blur parameters (40 with the [7] rows of resized_crop)
_TRIES = 10        # RandomResizedCrop.get_params draws at most ten windows before its central fallback
_SLOTS = 4         # staging ring: a slot is rewritten four batches after its upload was enqueued


class DeviceTrainLoader:
    """Iterating yields ``(x_lr, hr, mask, kernels, sdf)`` on the device, the argument order of
    ``JointModelWithLoss.forward(iter, x, sr_targets, segment_targets, kernel_targets, segment_sdf=)``.  Over an image-only dataset
    (``ResidentDataset(images)``) it yields ``(x_lr, hr, kernels)``, the reference's ONLY_IMAGES tuple and the argument order of
    ``SRModelWithLoss.forward(iter, x, sr_targets, kernel_targets)``: no mask is gathered and no SDF computed, every decision (indices,
    windows, flips, blur parameters) is the one a loader over the same images with masks takes for the same seed, and ``x``, ``hr`` and
    ``k`` are the same bytes.  ``shard=`` with world > 1 is refused there: data-parallel pretraining is not built.

    Sampling (train.py:60-62): one permutation of the shard's samples per epoch, without replacement (RandomSampler); batches of
    ``batch_size``, the last of an epoch short unless ``drop_last`` (BatchSampler); epochs repeat until ``num_iterations`` batches have
    been produced (IterationBasedBatchSampler), one epoch when it is None.  ``shuffle=False`` takes the shard's samples in dataset order
    instead (SequentialSampler + BatchSampler, train.py:65-67: the validation loader); the crop, mirror and blur draws stay, as the
    reference's validation split goes through the train transforms.  ``state_dict()`` / ``load_state_dict()`` carry the sequence over to
    another loader (a resumed run).  ``shard=(rank, world)`` keeps the samples at positions
    ``i % world == rank`` of ``dataset``, so data-parallel ranks see disjoint data.

    ``shard_mode="batch"`` shards the BATCH instead of the dataset: every rank runs the decision sequence of ONE loader with batch
    ``world * batch_size`` over the whole dataset -- the same seeded generator, the same permutation, the same window, flip and blur
    draws -- and keeps rows ``[rank * batch_size, (rank + 1) * batch_size)`` of each global batch.  The rows of step t, concatenated over
    the ranks, are therefore exactly what the single loader with ``batch_size = world * b`` and the same seed yields: a data-parallel run
    IS the single-GPU experiment with the same global batch (under ``"sample"``, the default, each rank permutes its own subset and the
    samples of step t depend on the world size).  The generator advances identically on every rank and ``state_dict()`` is the same on
    every rank; it carries ``"global_batch"``, and loads into a loader of any ``world`` whose ``world * batch_size`` is that number (a
    run continued on another number of GPUs) and into no other.  ``len()`` and ``produced`` count global batches.  Ranks must present
    equal shards to the gradient exchange, so ``shuffle=True`` with ``world > 1`` needs ``drop_last=True`` (ValueError otherwise).
    ``shuffle=False`` (validation) may end with a short global batch; it is split by the same contiguous rule, a rank's slice may be
    shorter or empty, and for a global batch of which the rank holds nothing the loader yields ``None`` in place of a batch.

    Every draw comes from ONE seeded host ``torch.Generator`` (the blur parameters too: DeviceDegradation.draw_params is handed the same
    generator).  A crop offset is uniform on [0, H-h] x [0, W-w], as torchvision's RandomCrop.get_params draws it; the mirror has p = 0.5.
    ``draw(B)`` makes the decisions of the next batch -- a [B,5] int32 table (pool index, y0, x0, mirror, vflip) and the [B,3] blur
    parameters (sigma_x, sigma_y, theta) -- and ``batch(sel, blur_params)`` turns decisions into tensors, so callers can force them.
    The random streams are not NumPy's or torchvision's; the distributions are.

    ``augmentation`` is a list in the format of cfg.DATASET.DATA_AUGMENTATION, by default the shipped yaml's, and is interpreted as
    TrainTransforms does, quirks included (see interpret_augmentation): in particular the yaml's ``["RandomVerticalFlip", 0.3]`` has NO
    effect in the reference and none here.  ``vflip_p`` is the explicit way to flip vertically and is the probability that the flip
    HAPPENS (the reference's RandomVerticalFlip(p) class flips with probability 1 - p).  Flips act on the whole image and the window is
    taken afterwards (RandomMirror -> ToTensor -> crop).

    ``resized_crop={"scale": (lo, hi), "ratio": (lo, hi)}`` (defaults (0.5, 1.0) / (1.0, 1.0), the reference's class defaults) replaces
    the fixed window by RandomResizedCrop (transforms.py:607-622): per sample a window of area ``U(scale) * H * W`` and aspect
    ``exp(U(log ratio))``, drawn as torchvision's published RandomResizedCrop.get_params draws it (ten tries, then the central fallback),
    and resampled to the crop size by ``csbsr_gather_resize_u8`` -- image AND mask, bilinear with torchvision's antialias default, so the
    mask comes out soft.  ``draw`` then returns [b,7] rows (..., hs, ws) from a fixed number of uniforms per sample (24), whatever is
    accepted, and ``batch`` takes such rows.  A non-identity ``RandomResizedCrop`` entry of ``augmentation`` means the same (see
    split_resized_crop); the explicit argument wins.  Images may be smaller than the crop in this mode (the window is upsampled) but not
    larger than 8 times the crop per side, the kernel's limit on a window.

    The mask is ``bytes / 255`` like the reference's (``mask / 255``, data_preprocess.py:44), so a {0, 255} mask becomes {0, 1}.
    ``blur=False`` (crack_dataset.py:55-58): the kernel target is a delta at the centre, the LR image the down-scaled unblurred crop.

    ``interpolation`` is FactorResize's mode (SOLVER.DOWNSCALE_INTERPOLATION; ``from_cfg`` reads it): "bicubic", or "area", the f x f box
    mean, on both LR paths; ``antialias`` has no meaning with "area".  It changes no draw and no ``state_dict()``.  The model's loss must
    use the same mode (``model.downscale``): the trainer's loops compare the two before the first step.
    """

    def __init__(self, dataset, crop, scale, ksize=21, *, batch_size, num_iterations=None, blur=True, isotropic=False, augmentation=None,
                 vflip_p=0.0, antialias=True, drop_last=False, seed=None, shard=(0, 1), shuffle=True, resized_crop=None,
                 shard_mode="sample", interpolation="bicubic"):
        self.dataset = dataset
        self.interpolation = check_downscale(interpolation)
        self.h, self.w = (int(crop), int(crop)) if np.isscalar(crop) else (int(crop[0]), int(crop[1]))
        self.scale, self.K = int(scale), int(ksize)
        if self.h < 1 or self.w < 1 or self.h % self.scale or self.w % self.scale:
            raise ValueError(f"crop {self.h} x {self.w} must be positive multiples of the scale {self.scale}")
        self.batch_size, self.num_iterations = int(batch_size), None if num_iterations is None else int(num_iterations)
        if self.batch_size < 1:
            raise ValueError("batch_size must be positive")
        self.blur, self.drop_last, self.shuffle = bool(blur), bool(drop_last), bool(shuffle)
        self.vflip_p = float(vflip_p)
        if not 0.0 <= self.vflip_p <= 1.0:
            raise ValueError("vflip_p must be a probability")
        rank, world = (int(v) for v in shard)
        if not 0 <= rank < world:
            raise ValueError(f"shard {shard}: need 0 <= rank < world")
        if shard_mode not in ("sample", "batch"):
            raise ValueError(f"shard_mode {shard_mode!r}: 'sample' or 'batch'")
        self.shard_mode, self.rank, self.world = shard_mode, rank, world
        self.image_only = getattr(dataset, "mask", None) is None
        if self.image_only and world > 1:
            raise NotImplementedError("an image-only dataset feeds SR pretraining, which is single-GPU: shard=(rank, world > 1) is not built")
        if shard_mode == "batch":
            if self.shuffle and world > 1 and not self.drop_last:
                raise ValueError("shard_mode='batch' with shuffle=True and world > 1 needs drop_last=True: a short global batch at the end "
                                 "of an epoch would leave the ranks unequal shards")
            self.indices = np.asarray(dataset.indices, dtype=np.int64)                      # the whole dataset: the rank keeps rows, not samples
            self._step_batch = world * self.batch_size                                      # rows one step of the decision sequence draws
        else:
            self.indices = np.asarray(dataset.indices[rank::world], dtype=np.int64)         # pool indices of this shard
            self._step_batch = self.batch_size
        if len(self.indices) == 0:
            raise ValueError(f"shard {shard} of a dataset of {len(dataset)} is empty")
        dims = dataset.dims[self.indices]
        augmentation, listed = split_resized_crop(DEFAULT_AUGMENTATION if augmentation is None else augmentation)
        if resized_crop is None:
            resized_crop = listed
        self.resized_crop = None if resized_crop is None else _resized_crop_args(resized_crop)
        if self.resized_crop is None:
            if (dims[:, 0] < self.h).any() or (dims[:, 1] < self.w).any():
                raise ValueError(f"an image is smaller than the crop {self.h} x {self.w}")
        elif (dims[:, 0] > 8 * self.h).any() or (dims[:, 1] > 8 * self.w).any():
            raise ValueError(f"an image is more than 8 times the crop {self.h} x {self.w} per side: its windows could exceed what "
                             "csbsr_gather_resize_u8 resamples")
        # (with resized_crop the entry that stood for it is a RandomCrop by now, or the list has its own crop; the sizes interpret_augmentation
        # sees only matter for a list without a crop, which resized_crop supplies)
        aug = interpret_augmentation(augmentation, (self.h, self.w), dims if self.resized_crop is None else np.array([[self.h, self.w]]))
        self.mirror_p = aug["mirror_p"]
        self.gen = torch.Generator(device="cpu")
        if seed is not None:
            self.gen.manual_seed(int(seed))
        self.device = dataset.device
        self.deg = DeviceDegradation(self.scale, ksize=self.K, isotropic=isotropic, antialias=antialias, device=self.device,
                                     interpolation=self.interpolation)
        self.deg.gen = self.gen          # one generator for every draw
        self.antialias = bool(antialias)
        self.resize_antialias = True          # of the window's resample: torchvision's default for tensors since 0.17
        self._perm, self._cursor, self._produced, self._resumed = None, 0, 0, False
        self._staging = Staging(self.device, slots=_SLOTS)

    @classmethod
    def from_cfg(cls, cfg, dataset, **kw):
        """Arguments from a reference-style config tree: INPUT.IMAGE_SIZE, MODEL.SCALE_FACTOR, BLUR.*, SOLVER.BATCH_SIZE / MAX_ITER, and
        DATASET.DATA_AUGMENTATION when the tree has that node (it is not in the default tree: the shipped yaml's list then applies)."""
        args = dict(crop=tuple(cfg.INPUT.IMAGE_SIZE), scale=cfg.MODEL.SCALE_FACTOR, ksize=cfg.BLUR.KERNEL_SIZE_OUTPUT,
                    batch_size=cfg.SOLVER.BATCH_SIZE, num_iterations=cfg.SOLVER.MAX_ITER, blur=cfg.BLUR.FLAG, isotropic=cfg.BLUR.ISOTROPIC,
                    interpolation=cfg.SOLVER.get("DOWNSCALE_INTERPOLATION", "bicubic"))
        node = cfg.get("DATASET") if hasattr(cfg, "get") else None
        if node is not None and "DATA_AUGMENTATION" in node:
            args["augmentation"] = node["DATA_AUGMENTATION"]
        args.update(kw)
        return cls(dataset, **args)

    # ------------------------------------------------------------------------------------------------------------- decisions (host)
    def _next_indices(self, B):
        """The next <= B pool indices of the running epoch; a new permutation starts when the epoch is used up."""
        if self._perm is None or self._cursor >= len(self._perm):
            self._perm = self.indices[torch.randperm(len(self.indices), generator=self.gen).numpy()] if self.shuffle else self.indices
            self._cursor = 0
        idx = self._perm[self._cursor:self._cursor + B]
        self._cursor += len(idx)
        return idx

    def draw(self, B=None):
        """Decisions of the next batch: (sel int32 [b,5] = (pool index, y0, x0, mirror, vflip), blur_params fp32 [b,3]) with b <= B
        (b < B only at the end of an epoch).  With ``resized_crop`` the rows are [b,7]: (..., hs, ws), the window's size.  B defaults to
        what one step draws: ``batch_size``, or under ``shard_mode="batch"`` the GLOBAL batch (``shard_rows`` takes the rank's rows)."""
        idx = self._next_indices(self._step_batch if B is None else int(B))
        b = len(idx)
        dims = self.dataset.dims[idx].astype(np.int64)
        if self.resized_crop is not None:
            return self._draw_windows(idx, dims), self.deg.draw_params(b)
        u = torch.rand(b, 4, generator=self.gen, dtype=torch.float64).numpy()
        span_y, span_x = dims[:, 0] - self.h, dims[:, 1] - self.w
        sel = np.empty((b, 5), dtype=np.int32)
        sel[:, 0] = idx
        sel[:, 1] = np.minimum((u[:, 0] * (span_y + 1)).astype(np.int64), span_y)
        sel[:, 2] = np.minimum((u[:, 1] * (span_x + 1)).astype(np.int64), span_x)
        sel[:, 3] = u[:, 2] < self.mirror_p
        sel[:, 4] = u[:, 3] < self.vflip_p
        return torch.from_numpy(sel), self.deg.draw_params(b)

    def _draw_windows(self, idx, dims):
        """[b,7] rows for the pool indices ``idx``: RandomResizedCrop.get_params per sample out of 24 uniforms -- (area, aspect) of
        _TRIES tries, the offset pair, the two flips -- all drawn whatever is accepted, so the generator advances by the same amount for
        every batch of b samples.  The first try whose rounded window fits the image is taken, else the central fallback."""
        b = len(idx)
        (s_lo, s_hi), (r_lo, r_hi) = self.resized_crop
        u = torch.rand(b, 2 * _TRIES + 4, generator=self.gen, dtype=torch.float64).numpy()
        H, W = dims[:, 0], dims[:, 1]
        t = (H * W)[:, None] * (s_lo + (s_hi - s_lo) * u[:, 0:2 * _TRIES:2])
        r = np.exp(np.log(r_lo) + (np.log(r_hi) - np.log(r_lo)) * u[:, 1:2 * _TRIES:2])
        ws, hs = np.rint(np.sqrt(t * r)).astype(np.int64), np.rint(np.sqrt(t / r)).astype(np.int64)
        ok = (ws > 0) & (ws <= W[:, None]) & (hs > 0) & (hs <= H[:, None])
        first = np.argmax(ok, axis=1)
        took = ok[np.arange(b), first]
        hs, ws = hs[np.arange(b), first], ws[np.arange(b), first]
        # the fallback: the largest central window whose aspect is inside the ratio range
        in_ratio = W / H
        fb_w = np.where(in_ratio > r_hi, np.rint(H * r_hi).astype(np.int64), W)
        fb_h = np.where(in_ratio < r_lo, np.rint(W / r_lo).astype(np.int64), H)
        hs, ws = np.where(took, hs, fb_h), np.where(took, ws, fb_w)
        span_y, span_x = H - hs, W - ws
        sel = np.empty((b, 7), dtype=np.int32)
        sel[:, 0] = idx
        sel[:, 1] = np.where(took, np.minimum((u[:, -4] * (span_y + 1)).astype(np.int64), span_y), span_y // 2)
        sel[:, 2] = np.where(took, np.minimum((u[:, -3] * (span_x + 1)).astype(np.int64), span_x), span_x // 2)
        sel[:, 3] = u[:, -2] < self.mirror_p
        sel[:, 4] = u[:, -1] < self.vflip_p
        sel[:, 5], sel[:, 6] = hs, ws
        return torch.from_numpy(sel)

    # ------------------------------------------------------------------------------------------------------------- tensors (device)
    def _upload(self, sel, params):
        """sel int32 [B,5] (or [B,7]) + params fp32 [B,3] -> device views, through a pinned staging slot and ONE non-blocking copy.  Before a
        slot is rewritten the host waits for the upload issued from it _SLOTS batches earlier (the pinned bytes must not change under a
        copy in flight: multi_tensor.Staging): the only host wait on the device here, and one that blocks only a host running more
        than _SLOTS batches ahead of the device."""
        B, cols = sel.shape
        row = 4 * cols + 12          # = _ROW for the [5] rows
        host = self._staging.stage(B * row, self.batch_size * row)
        host[:B * 4 * cols].view(torch.int32).view(B, cols).copy_(sel)
        host[B * 4 * cols:].view(torch.float32).view(B, 3).copy_(params)
        dev = self._staging.upload()
        self._staging.record()
        return dev[:B * 4 * cols].view(torch.int32).view(B, cols), dev[B * 4 * cols:].view(torch.float32).view(B, 3)

    def batch(self, sel, blur_params=None):
        """Decisions -> (x_lr [B,3,h/s,w/s], hr [B,3,h,w], mask [B,1,h,w], kernels [B,1,K,K], sdf [B,1,h,w]), or (x_lr, hr, kernels) over an
        image-only dataset.  ``sel`` ([B,5], or [B,7] with
        ``resized_crop``) is validated on the host first.  No wait on the batch's own work: the host may only block on the upload issued four batches earlier (_upload)."""
        sel = torch.as_tensor(sel)
        if self.resized_crop is not None:
            self.dataset.check_windows(sel.numpy(), self.h, self.w)
        else:
            self.dataset.check_selection(sel.numpy(), self.h, self.w)
        if self.device.type != "cuda":
            raise L.CsbsrHipError("DeviceTrainLoader.batch needs the dataset on a GPU: csbsr_amd has no fallback path")
        sel = sel.to(torch.int32)
        B = sel.shape[0]
        if self.blur:
            if blur_params is None:
                raise ValueError("blur=True needs the [B,3] blur parameters")
            params = torch.as_tensor(blur_params, dtype=torch.float32).reshape(B, 3)
        else:
            params = torch.zeros(B, 3)
        with torch.cuda.device(self.device):
            sel_dev, params_dev = self._upload(sel, params)
            if self.resized_crop is not None:
                hr, mask = self.dataset.gather_resized(sel_dev, B, self.h, self.w, self.resize_antialias)
            else:
                hr, mask = self.dataset.gather(sel_dev, B, self.h, self.w)
            if self.blur:
                out = self.deg(hr, mask, params=params_dev)
                return (out[0], out[1], out[3]) if self.image_only else out
            k = torch.zeros(B, 1, self.K, self.K, dtype=torch.float32, device=self.device)
            k[:, :, self.K // 2, self.K // 2] = 1.0
            x = self.deg.downscale(hr)
            return (x, hr, k) if self.image_only else (x, hr, mask, k, self.deg.sdf(mask))

    def __len__(self):
        if self.num_iterations is not None:
            return self.num_iterations
        n = len(self.indices)
        return n // self._step_batch if self.drop_last else -(-n // self._step_batch)

    @property
    def produced(self):
        """batches (global batches under ``shard_mode="batch"``) produced so far by the running (or loaded) sequence"""
        return self._produced

    def shard_rows(self, sel, params):
        """This rank's rows of a global batch's decisions, or None when it holds none of them (a short last validation batch)."""
        lo = self.rank * self.batch_size
        sel, params = sel[lo:lo + self.batch_size], params[lo:lo + self.batch_size]
        return None if sel.shape[0] == 0 else (sel, params)

    def iter_decisions(self):
        """The (sel, blur_params) sequence __iter__ turns into batches (host only).  Under ``shard_mode="batch"`` every rank steps
        through the same global sequence and an item is the rank's rows of it, or None."""
        if self.shard_mode == "batch":
            return (self.shard_rows(sel, params) for sel, params in self._iter_steps())
        return self._iter_steps()

    def _iter_steps(self):
        if self._resumed:          # a loaded state continues: same permutation, cursor and count (the generator was restored with them)
            self._resumed = False
            if self.num_iterations is None and self._perm is not None and self._cursor >= len(self._perm):
                return             # (saved after the last batch of the single pass)
        else:
            self._perm, self._produced = None, 0
        if self.drop_last and len(self.indices) < self._step_batch:
            return
        while self.num_iterations is None or self._produced < self.num_iterations:
            sel, params = self.draw(self._step_batch)
            last = self._cursor >= len(self._perm)
            if not (self.drop_last and sel.shape[0] < self._step_batch):
                self._produced += 1
                yield sel, params
            if last and self.num_iterations is None:
                return

    def state_dict(self):
        """What the decision sequence depends on, taken between two batches: the generator, the running epoch's permutation (pool
        indices), the cursor in it and the number of batches produced.  Tensors and ints only.  Under ``shard_mode="batch"`` also
        ``"global_batch"`` = world * batch_size, and the whole dict is the same on every rank."""
        state = {"generator": self.gen.get_state().clone(), "perm": None if self._perm is None else torch.from_numpy(np.array(self._perm)),
                 "cursor": int(self._cursor), "produced": int(self._produced), "samples": len(self.indices)}
        if self.shard_mode == "batch":
            state["global_batch"] = int(self._step_batch)
        return state

    def load_state_dict(self, state):
        """Continue another loader's sequence: the next ``iter_decisions`` / ``__iter__`` of this loader goes on where that one stopped
        instead of starting over.  The loader must have been built over the same shard with the same arguments -- under
        ``shard_mode="batch"``: over the same dataset with the same GLOBAL batch, whatever the world size."""
        if (self.shard_mode == "batch") != ("global_batch" in state):
            raise ValueError(f"loader state of shard_mode {'batch' if 'global_batch' in state else 'sample'!r}, this loader's is {self.shard_mode!r}")
        if self.shard_mode == "batch" and int(state["global_batch"]) != self._step_batch:
            raise ValueError(f"loader state of global batch {int(state['global_batch'])}, this loader's is {self.world} x {self.batch_size} = "
                             f"{self._step_batch}")
        perm = state["perm"]
        if int(state["samples"]) != len(self.indices) or (perm is not None and len(perm) != len(self.indices)):
            raise ValueError(f"loader state of a shard of {int(state['samples'])} samples, this shard has {len(self.indices)}")
        if perm is not None and not np.isin(np.asarray(perm), self.indices).all():
            raise ValueError("loader state names samples outside this shard")
        self.gen.set_state(torch.as_tensor(state["generator"], dtype=torch.uint8).cpu())
        self._perm = None if perm is None else np.asarray(perm, dtype=np.int64).copy()
        self._cursor, self._produced, self._resumed = int(state["cursor"]), int(state["produced"]), True

    def __iter__(self):
        for item in self.iter_decisions():
            yield None if item is None else self.batch(*item)

