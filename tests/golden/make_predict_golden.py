"""Generate the prediction fixture from the REFERENCE's own unlabeled-image dataset: ``TTICrackDataSetTest.__getitem__`` with
``TestTransforms`` and ``SplitPatch`` (/root/reference/model/data/crack_dataset.py:145-172, transforms/data_preprocess.py:48-60,
samplers/patch_sampler.py), iterated under torch's DataLoader with its default collate the way test.py iterates its test sets
(SequentialSampler, BatchSampler(drop_last=False)), on the CPU, over three seeded tiny PNGs this file writes into a temporary directory.

    python tests/golden/make_predict_golden.py          # rewrites tests/golden/predict_tti.npz

What the fixture pins FROM THE REFERENCE: that INPUT.IMAGE_SIZE is the LR patch on this path (not divided by the scale), HWC -> CHW, the fp32
``/ 255``, the patch order of the unfold, the unfold-shape arrays with entries 5 and 6 scaled, the collated batch layout, and where
``JointPatch`` puts every value of a batch of output patches (a ramp: fp32 arange over [B * nPatch, 3, scale * ph, scale * pw]).

What is NOT the reference's: the stand-in modules of make_eval_golden.py (nothing of them is called on this path), and the ORDER of the
files: the reference takes ``Path.glob``'s order, the fixture sorts ``fnames`` before it iterates, as the loader does.  The image sizes are
multiples of the 16-pixel patch (the reference's unfold drops any remainder); images 0 and 1 share a size so that the default collate can
batch them, image 2 is smaller and makes the short last batch.

Only data is written: the decoded uint8 inputs, the names and the reference's collated outputs.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import predict_cases as PC  # noqa: E402
from make_eval_golden import install_stand_ins  # noqa: E402

SCALE, PATCH, BATCH = 2, [16, 16], 2
IMAGES = {"tti_b.png": (32, 48), "tti_a.png": (32, 48), "tti_c.png": (16, 32)}


def main():
    install_stand_ins()
    from torch.utils.data import DataLoader
    from torch.utils.data.sampler import BatchSampler, SequentialSampler
    from model.data.crack_dataset import TTICrackDataSetTest
    from model.data.samplers.patch_sampler import JointPatch
    from model.data.transforms.data_preprocess import TestTransforms

    rng = np.random.default_rng(20251)
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (h, w) in IMAGES.items():
            Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(tmp, name))
        cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(SCALE_FACTOR=SCALE, NUM_CLASSES=1), INPUT=types.SimpleNamespace(IMAGE_SIZE=PATCH))
        ds = TTICrackDataSetTest(cfg, tmp, BATCH, transforms=TestTransforms(cfg))
        ds.fnames = sorted(ds.fnames)                                       # (the order is ours, see above)
        assert ds.fnames == sorted(IMAGES)
        loader = DataLoader(ds, num_workers=0, batch_sampler=BatchSampler(sampler=SequentialSampler(ds), batch_size=BATCH, drop_last=False))
        dec = [np.array(Image.open(os.path.join(tmp, n))) for n in ds.fnames]
        joint = JointPatch()
        nb = 0
        for j, (imgs, fname, img_shape, seg_shape) in enumerate(loader):
            assert imgs.dtype == torch.float32 and (img_shape.numpy() == img_shape[0].numpy()).all()
            flat = imgs.view(-1, *imgs.shape[2:])
            ramp = torch.from_numpy(PC.ramp_patches(flat.shape[0], 3, SCALE * PATCH[0], SCALE * PATCH[1]))
            arrays[f"b{j}_imgs"] = imgs.numpy()
            arrays[f"b{j}_img_unfold_shape"], arrays[f"b{j}_seg_unfold_shape"] = img_shape[0].numpy(), seg_shape[0].numpy()
            arrays[f"b{j}_fnames"] = np.array(list(fname))
            arrays[f"b{j}_joint_ramp"] = joint(ramp, img_shape[0], batch_size=len(img_shape)).numpy()      # (as inference.py:250 calls it)
            nb += 1
        arrays.update({"n": np.int32(len(dec)), "nbatch": np.int32(nb), "names": np.array(ds.fnames), "scale": np.int32(SCALE),
                       "patch": np.array(PATCH, np.int32), "batch_size": np.int32(BATCH)})
        for i, a in enumerate(dec):
            assert a.dtype == np.uint8 and a.shape == IMAGES[ds.fnames[i]] + (3,)
            arrays[f"lr_{i}"] = a
    # the conditions the tests rely on
    assert arrays["b0_imgs"].shape == (2, 6, 3, 16, 16) and arrays["b1_imgs"].shape == (1, 2, 3, 16, 16) and nb == 2
    assert list(arrays["b0_img_unfold_shape"]) == [BATCH, 1, 2, 3, 3, 32, 32] and arrays["b0_joint_ramp"].shape == (2, 3, 64, 96)
    np.savez_compressed(PC.GOLDEN, **arrays)
    size = os.path.getsize(PC.GOLDEN)
    assert size < 200_000, size
    print(f"wrote {PC.GOLDEN}: {size} bytes")


if __name__ == "__main__":
    main()
