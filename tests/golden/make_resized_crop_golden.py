"""Generate the resized-crop fixture from the REFERENCE's own transforms (/root/reference/model/data/transforms: ConvertFromInts,
RandomMirror, ToTensor, RandomVerticalFlip, RandomResizedCrop and Compose, followed by the ``image / 255, mask / 255`` of
data_preprocess.py:44), run on CPU in the build container with every random decision forced and recorded.

    python tests/golden/make_resized_crop_golden.py          # rewrites tests/golden/resized_crop_batch.npz

What the fixture pins FROM THE REFERENCE: the order of the operations (mirror on the HWC array -> HWC to CHW -> vertical flip on the
tensor -> resized crop -> / 255), that the window is in the flipped image's coordinates, that the mask goes through the same resample
as the image (transforms.py:619-620), the argument order of ``resized_crop(image, *params, size=)`` and the fp32 ``/ 255`` at the end.
Samples without a vertical flip go through Compose([ConvertFromInts, RandomMirror, ToTensor, RandomResizedCrop(CROP)]), samples with one
through the same list with the reference's RandomVerticalFlip(p=0.0) before the crop (it flips when p <= rand(): always).

What is NOT the reference's: cv2 and torchvision are not installed, so this file supplies stand-ins -- an empty ``cv2``, and of
torchvision.transforms the surface those classes touch: ``RandomResizedCrop(size).get_params`` (returns the forced window),
``RandomVerticalFlip(p=1)`` (a flip of the row axis) and ``functional.resized_crop``: a slice followed by
``torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=True)``, which is what torchvision >= 0.17 does for a
float tensor by default.  THE RESAMPLE IS THE STAND-IN'S (torch's CPU kernel), NOT THE REFERENCE'S OWN CODE.

Only data is written: the uint8 inputs, the forced decisions and the fp32 outputs.
"""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resized_crop_cases as RZ  # noqa: E402

REF = "/root/reference"
CROP = RZ.CROP
SIZES = RZ.SIZES

_forced = {"window": None, "mirror": None, "calls": 0}


class _RandomResizedCrop:
    def __init__(self, size):
        self.size = tuple(size)

    @staticmethod
    def get_params(img, scale, ratio):
        i, j, h, w = _forced["window"]
        assert 0 <= i and i + h <= img.shape[-2] and 0 <= j and j + w <= img.shape[-1] and h >= 1 and w >= 1
        return i, j, h, w


def _resized_crop(img, top, left, height, width, size, **kw):
    assert not kw and img.dtype == torch.float32 and img.dim() == 3
    _forced["calls"] += 1
    win = img[..., top:top + height, left:left + width]
    return F.interpolate(win[None], size=tuple(size), mode="bilinear", align_corners=False, antialias=True)[0]


class _RandomVerticalFlip:
    def __init__(self, p=0.5):
        assert p == 1.0

    def __call__(self, img):
        return img.flip(-2)


def install_stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("cv2")
    tv = mod("torchvision")
    tv.transforms = mod("torchvision.transforms", RandomCrop=object, RandomVerticalFlip=_RandomVerticalFlip, RandomResizedCrop=_RandomResizedCrop)
    tv.transforms.functional = mod("torchvision.transforms.functional", InterpolationMode=object, resized_crop=_resized_crop)
    sys.path.insert(0, REF)


def decisions():
    """(image, y0, x0, mirror, vflip, hs, ws): all four flip combinations; windows smaller and larger than the crop in either direction,
    one of exactly the crop size, a whole image, windows touching every edge."""
    rows = [
        (0, 0, 0, 0, 0, 29, 40),          # a whole image
        (2, 4, 2, 1, 0, 25, 22),          # down in y, up in x
        (3, 0, 10, 0, 1, 21, 30),         # top to bottom
        (4, 6, 0, 1, 1, 32, 31),          # left to right, 2x down in y
        (1, 0, 0, 0, 0, 16, 24),          # the crop size: the identity
        (5, 3, 9, 1, 0, 9, 13),           # up in both
        (6, 1, 12, 0, 1, 25, 24),         # identity in x only
        (7, 15, 0, 1, 1, 16, 25),         # identity in y only, bottom edge
        (0, 9, 17, 1, 0, 20, 23),         # bottom right corner
        (3, 5, 40, 0, 1, 3, 7),           # a sliver
        (5, 0, 0, 1, 1, 17, 52),          # a whole wide image
        (4, 11, 5, 0, 0, 11, 26),
    ]
    return np.array(rows, dtype=np.int32)


def main():
    install_stand_ins()
    from model.data.transforms import transforms as T

    real_randint = np.random.randint
    np.random.randint = lambda *a, **k: _forced["mirror"]           # RandomMirror: `if np.random.randint(2)`
    try:
        plain = T.Compose([T.ConvertFromInts(), T.RandomMirror(), T.ToTensor(), T.RandomResizedCrop(list(CROP))])
        flipped = T.Compose([T.ConvertFromInts(), T.RandomMirror(), T.ToTensor(), T.RandomVerticalFlip(p=0.0), T.RandomResizedCrop(list(CROP))])
        rng = np.random.default_rng(20241018)
        images = [rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8) for H, W in SIZES]
        masks = [(255 * (rng.random((H, W)) < 0.3)).astype(np.uint8) for H, W in SIZES]
        for i in (5, 7):                                             # two masks with arbitrary bytes (a JPEG mask is not {0, 255})
            masks[i] = rng.integers(0, 256, size=SIZES[i], dtype=np.uint8)
        sel = decisions()
        out_i, out_m = [], []
        for idx, y0, x0, mirror, vflip, hs, ws in sel.tolist():
            _forced["window"], _forced["mirror"] = (y0, x0, hs, ws), mirror
            a, m = (flipped if vflip else plain)(images[idx], masks[idx][:, :, np.newaxis])      # crack_dataset.py:44-47
            a, m = a / 255, m / 255                                  # data_preprocess.py:44
            out_i.append(a.contiguous().numpy())
            out_m.append(m.contiguous().numpy())
    finally:
        np.random.randint = real_randint
    out_i, out_m = np.stack(out_i), np.stack(out_m)
    assert _forced["calls"] == 2 * len(sel)
    assert out_i.dtype == np.float32 and out_i.shape == (len(sel), 3) + CROP and out_m.shape == (len(sel), 1) + CROP

    # the conditions the tests rely on
    assert {(int(r[3]), int(r[4])) for r in sel} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(r[5] > CROP[0] for r in sel) and any(r[5] < CROP[0] for r in sel) and any(r[6] > CROP[1] for r in sel) and any(r[6] < CROP[1] for r in sel)
    for arrays, out in ((images, out_i), (masks, out_m)):
        r64 = RZ.gather_resize_numpy(arrays, sel, *CROP, True, np.float64)
        print("fixture against the fp64 restatement: max |diff| %.3e" % np.abs(out - r64).max())
        assert np.abs(out - r64).max() < 1e-5
    soft = out_m[(out_m > 0) & (out_m < 1)]
    assert soft.size > 100, "the masks do not come out soft"

    arrays = {"n_images": np.int32(len(images)), "sel": sel, "crop": np.array(CROP, np.int32), "out_image": out_i, "out_mask": out_m}
    for i, (a, m) in enumerate(zip(images, masks)):
        arrays[f"image_{i}"], arrays[f"mask_{i}"] = a, m
    np.savez_compressed(RZ.GOLDEN, **arrays)
    print(f"wrote {RZ.GOLDEN}: {os.path.getsize(RZ.GOLDEN)} bytes, {len(sel)} samples from {len(images)} images")


if __name__ == "__main__":
    main()
