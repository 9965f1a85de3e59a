"""Generate the resident-loader fixture from the REFERENCE's own transforms (/root/reference/model/data/transforms: ConvertFromInts,
RandomMirror, ToTensor, RandomVerticalFlip, RandomCrop, Compose and TrainTransforms, the last followed by its ``image / 255, mask / 255``),
run on CPU in the build container with every random decision forced and recorded.

    python tests/golden/make_resident_golden.py          # rewrites tests/golden/resident_batch.npz

What the fixture pins FROM THE REFERENCE: the order of the operations (mirror on the HWC array -> HWC to CHW -> vertical flip on the
tensor -> crop -> / 255), the mirror itself, the HWC -> CHW change and the fp32 ``/ 255``.  For the samples without a vertical flip the
pipeline is the reference's TrainTransforms built from the shipped yaml's DATA_AUGMENTATION list, so the fixture also pins that its
``["RandomVerticalFlip", 0.3]`` entry has no effect.  The samples with a vertical flip go through a Compose of the same classes with the
reference's RandomVerticalFlip(p=0.0) (which flips always: it flips when p <= rand()) before the crop.

What is NOT the reference's: cv2 and torchvision are not installed, so this file supplies stand-ins -- an empty ``cv2``, and of
torchvision.transforms the surface those classes touch: ``RandomCrop(size).get_params`` (returns the forced window),
``functional.resized_crop`` (a plain slice; the requested size equals the window, so no resampling exists to restate) and
``RandomVerticalFlip(p=1)`` (a flip of the row axis).  THE CROP ARITHMETIC IS THE STAND-IN'S.

Only data is written: the uint8 inputs, the forced decisions and the fp32 outputs.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resident_cases as RC  # noqa: E402

REF = "/root/reference"
CROP = (16, 24)                                            # h x w: not square, so H and W cannot be swapped unnoticed
SIZES = [(29, 40), (16, 24), (33, 27), (21, 47), (38, 31), (17, 52), (26, 36), (31, 25)]
YAML_AUGMENTATION = [["ConvertFromInts", "None"], ["RandomMirror", "None"], ["ToTensor", "None"], ["RandomVerticalFlip", 0.3],
                     ["RandomCrop", "None"]]              # config/config_csbsr_pspnet.yaml:28-33 as yaml.safe_load delivers it

_forced = {"window": None, "mirror": None}


class _RandomCrop:
    def __init__(self, size):
        self.size = tuple(size)

    @staticmethod
    def get_params(img, output_size):
        i, j = _forced["window"]
        h, w = output_size
        assert 0 <= i and i + h <= img.shape[-2] and 0 <= j and j + w <= img.shape[-1]
        return i, j, h, w


def _resized_crop(img, top, left, height, width, size, **kw):
    assert tuple(size) == (height, width), "the fixture only crops at the output size"
    return img[..., top:top + height, left:left + width]


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
    tv.transforms = mod("torchvision.transforms", RandomCrop=_RandomCrop, RandomVerticalFlip=_RandomVerticalFlip, RandomResizedCrop=object)
    tv.transforms.functional = mod("torchvision.transforms.functional", InterpolationMode=object, resized_crop=_resized_crop)
    sys.path.insert(0, REF)


def decisions():
    """(image, y0, x0, mirror, vflip): all four flip combinations, offsets 0 and maximal in each direction, an image of exactly the
    crop size, and interior offsets."""
    h, w = CROP
    rows = []
    for s, (img, (H, W)) in enumerate(zip([0, 2, 3, 4, 1, 5, 6, 7, 0, 3, 5, 4], [SIZES[i] for i in [0, 2, 3, 4, 1, 5, 6, 7, 0, 3, 5, 4]])):
        my, mx = H - h, W - w
        y0 = [0, my, 0, my, 0, my // 2, my, 1, my, 0, my - 1, my // 3][s]
        x0 = [0, 0, mx, mx, 0, mx // 2, 1, mx, mx, mx // 3, 0, mx - 1][s]
        rows.append((img, y0, x0, s & 1, (s >> 1) & 1))
    return np.array(rows, dtype=np.int32)


def main():
    install_stand_ins()
    from model.data.transforms import transforms as T
    from model.data.transforms.data_preprocess import TrainTransforms

    real_randint = np.random.randint
    np.random.randint = lambda *a, **k: _forced["mirror"]           # RandomMirror: `if np.random.randint(2)`
    try:
        cfg = types.SimpleNamespace(DATASET=types.SimpleNamespace(DATA_AUGMENTATION=YAML_AUGMENTATION), INPUT=types.SimpleNamespace(IMAGE_SIZE=list(CROP)))
        shipped = TrainTransforms(cfg)
        assert [type(t).__name__ for t in shipped.augment.transforms] == ["ConvertFromInts", "RandomMirror", "ToTensor", "RandomCrop"]
        flipped = T.Compose([T.ConvertFromInts(), T.RandomMirror(), T.ToTensor(), T.RandomVerticalFlip(p=0.0), T.RandomCrop(list(CROP))])

        rng = np.random.default_rng(20240427)
        images, masks = RC.random_pairs(rng, SIZES)
        for i in (5, 7):                                             # two masks with arbitrary bytes (a JPEG mask is not {0, 255})
            masks[i] = rng.integers(0, 256, size=SIZES[i], dtype=np.uint8)
        sel = decisions()
        out_i, out_m, path = [], [], []
        for idx, y0, x0, mirror, vflip in sel.tolist():
            _forced["window"], _forced["mirror"] = (y0, x0), mirror
            img, msk = images[idx], masks[idx][:, :, np.newaxis]     # crack_dataset.py:44-47
            if vflip:
                a, m = flipped(img, msk)
                a, m = a / 255, m / 255                              # data_preprocess.py:44
            else:
                a, m = shipped(img, msk)
            out_i.append(a.contiguous().numpy())
            out_m.append(m.contiguous().numpy())
            path.append(int(vflip))
    finally:
        np.random.randint = real_randint
    out_i, out_m = np.stack(out_i), np.stack(out_m)
    assert out_i.dtype == np.float32 and out_i.shape == (len(sel), 3) + CROP and out_m.shape == (len(sel), 1) + CROP

    # the conditions the tests rely on
    assert len(set(SIZES)) == len(SIZES) >= 6 and all(H != W for H, W in SIZES) and CROP[0] != CROP[1]
    assert {(int(r[3]), int(r[4])) for r in sel} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    spans = np.array([[SIZES[r[0]][0] - CROP[0], SIZES[r[0]][1] - CROP[1]] for r in sel])
    assert (sel[:, 1] == 0).any() and (sel[:, 2] == 0).any() and ((sel[:, 1] == spans[:, 0]) & (spans[:, 0] > 0)).any() \
        and ((sel[:, 2] == spans[:, 1]) & (spans[:, 1] > 0)).any()
    seen = np.unique(np.round(out_i * 255).astype(np.int64))
    assert len(seen) == 256, f"only {len(seen)} byte values reach a cropped output"
    assert np.array_equal(RC.gather_numpy(images, sel, *CROP), out_i) and np.array_equal(RC.gather_numpy(masks, sel, *CROP), out_m)

    arrays = {"n_images": np.int32(len(images)), "sel": sel, "crop": np.array(CROP, np.int32), "out_image": out_i, "out_mask": out_m,
              "path": np.array(path, np.int32)}
    for i, (a, m) in enumerate(zip(images, masks)):
        arrays[f"image_{i}"], arrays[f"mask_{i}"] = a, m
    np.savez_compressed(RC.GOLDEN, **arrays)
    print(f"wrote {RC.GOLDEN}: {os.path.getsize(RC.GOLDEN)} bytes, {len(sel)} samples from {len(images)} images")


if __name__ == "__main__":
    main()
