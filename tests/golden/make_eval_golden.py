"""Generate the resident-test-set fixture from the REFERENCE's own evaluation dataset: ``CrackDataSetTest.__getitem__`` with
``TestTransforms`` and ``SplitPatch`` (/root/reference/model/data/crack_dataset.py:71-142, transforms/data_preprocess.py:48-60,
samplers/patch_sampler.py), iterated as test.py:69-71 iterates it (SequentialSampler, BatchSampler(drop_last=False), torch's DataLoader
and its default collate), on the CPU, over a tiny test set this file writes into a temporary directory with PIL.

    python tests/golden/make_eval_golden.py          # rewrites tests/golden/eval_testset.npz

What the fixture pins FROM THE REFERENCE: which file feeds which tensor (image, mask, lr_images/<png>, kernels/<png>, the ``jpg`` ->
``png`` rename of every occurrence), HWC -> CHW, the fp32 ``/ 255``, the kernel's ``k / torch.sum(k)``, the patch order of the unfold, the
expansion of the kernel target over the patches, the two unfold-shape arrays and the collated batch layout with a short last batch.

What is NOT the reference's: cv2, skimage and torchvision are not installed, and tqdm / matplotlib are not needed, so this file puts EMPTY
stand-in modules under those names (``skimage.draw.disk``, ``torchvision.transforms.functional.InterpolationMode`` and ``tqdm.tqdm`` exist
as names only); nothing of them is called on this path.  The ORDER of the files is ours as well: the reference takes ``Path.glob``'s
order, the fixture sorts ``fnames`` before it iterates (the loader sorts too, and the tests match by name).

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
import eval_io_cases as EC  # noqa: E402

REF = "/root/reference"
SCALE, HR, K = 4, (32, 48), 21
SETS = {"A": dict(n=6, image_size=[16, 24], batch_size=4, names=["crack_00.jpg", "crack_01.jpg", "crack_02.jpg", "jpg_03.jpg", "crack_04.jpg",
                                                                  "crack_05.jpg"]),
        "B": dict(n=3, image_size=[32, 48], batch_size=3, names=["wall_2.jpg", "wall_0.jpg", "wall_1.jpg"])}


def install_stand_ins():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("cv2")
    mod("skimage").draw = mod("skimage.draw", disk=None)
    tv = mod("torchvision")
    tv.transforms = mod("torchvision.transforms")
    tv.transforms.functional = mod("torchvision.transforms.functional", InterpolationMode=object)
    mod("tqdm", tqdm=None)
    mod("matplotlib").pyplot = mod("matplotlib.pyplot")
    sys.path.insert(0, REF)


def write_set(root, spec, seed):
    """image_dir/<name>.jpg, mask_dir/<name>.jpg (JPEG masks: bytes other than 0 / 255 appear by themselves), blur/<blur_name>/lr_images and
    kernels/<png name>."""
    rng = np.random.default_rng(seed)
    dirs = {k: os.path.join(root, *k.split("/")) for k in ("images", "masks", "blur/set1/lr_images", "blur/set1/kernels")}
    for d in dirs.values():
        os.makedirs(d)
    kernels = EC.anisotropic_kernels(spec["n"], K, first=seed % 5)
    for i, name in enumerate(spec["names"]):
        hr = rng.integers(0, 256, size=HR + (3,), dtype=np.uint8)
        mask = (255 * (rng.random(HR) < 0.3)).astype(np.uint8)
        lr = rng.integers(0, 256, size=(HR[0] // SCALE, HR[1] // SCALE, 3), dtype=np.uint8)
        png = name.replace("jpg", "png")
        Image.fromarray(hr).save(os.path.join(dirs["images"], name), quality=100, subsampling=0)
        Image.fromarray(mask).save(os.path.join(dirs["masks"], name), quality=90)
        Image.fromarray(lr).save(os.path.join(dirs["blur/set1/lr_images"], png))
        Image.fromarray(kernels[i]).save(os.path.join(dirs["blur/set1/kernels"], png))
    return dirs


def main():
    install_stand_ins()
    from torch.utils.data import DataLoader
    from torch.utils.data.sampler import BatchSampler, SequentialSampler
    from model.data.crack_dataset import CrackDataSetTest
    from model.data.transforms.data_preprocess import TestTransforms

    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        for si, (s, spec) in enumerate(SETS.items()):
            dirs = write_set(os.path.join(tmp, s), spec, 20250 + si)
            cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(SCALE_FACTOR=SCALE, NUM_CLASSES=1),
                                        INPUT=types.SimpleNamespace(IMAGE_SIZE=spec["image_size"]))
            ds = CrackDataSetTest(cfg, dirs["images"], dirs["masks"], os.path.join(tmp, s, "blur"), "set1", spec["batch_size"],
                                  transforms=TestTransforms(cfg), sr_transforms=None)
            ds.fnames = sorted(ds.fnames)                                   # (the order is ours, see above)
            assert ds.fnames == sorted(spec["names"])
            loader = DataLoader(ds, num_workers=0, batch_sampler=BatchSampler(sampler=SequentialSampler(ds), batch_size=spec["batch_size"],
                                                                             drop_last=False))
            names = ds.fnames
            dec = {"hr": [np.array(Image.open(os.path.join(dirs["images"], n))) for n in names],
                   "mask": [np.array(Image.open(os.path.join(dirs["masks"], n))) for n in names],
                   "lr": [np.array(Image.open(os.path.join(dirs["blur/set1/lr_images"], n.replace("jpg", "png")))) for n in names],
                   "kernel": [np.array(Image.open(os.path.join(dirs["blur/set1/kernels"], n.replace("jpg", "png")))) for n in names]}
            nb, seen = 0, 0
            for j, (imgs, sr_t, seg_t, kern, fname, img_shape, seg_shape) in enumerate(loader):
                B = len(fname)
                # the NumPy restatement reproduces the reference's tensors exactly
                items = [EC.reference_item_numpy(dec["hr"][seen + b], dec["mask"][seen + b], dec["lr"][seen + b], dec["kernel"][seen + b],
                                                 spec["image_size"], SCALE, spec["batch_size"]) for b in range(B)]
                for t, col in zip((imgs, sr_t, seg_t, kern, img_shape, seg_shape), range(6)):
                    want = np.stack([it[col] for it in items])
                    assert t.numpy().dtype == want.dtype and np.array_equal(t.numpy(), want), (s, j, col)
                assert list(fname) == [n.replace("jpg", "png") for n in names[seen:seen + B]]
                assert kern.is_contiguous() and imgs.dtype == torch.float32
                for k, t in (("imgs", imgs), ("sr_targets", sr_t), ("masks", seg_t), ("kernel_targets", kern)):
                    arrays[f"{s}_b{j}_{k}"] = t.numpy()
                arrays[f"{s}_b{j}_img_unfold_shape"], arrays[f"{s}_b{j}_seg_unfold_shape"] = img_shape[0].numpy(), seg_shape[0].numpy()
                assert (img_shape.numpy() == img_shape[0].numpy()).all() and (seg_shape.numpy() == seg_shape[0].numpy()).all()
                arrays[f"{s}_b{j}_fnames"] = np.array(list(fname))
                seen += B
                nb += 1
            assert seen == spec["n"]
            arrays.update({f"{s}_n": np.int32(spec["n"]), f"{s}_nbatch": np.int32(nb), f"{s}_names": np.array(names),
                           f"{s}_image_size": np.array(spec["image_size"], np.int32), f"{s}_scale": np.int32(SCALE),
                           f"{s}_batch_size": np.int32(spec["batch_size"])})
            for k, lst in dec.items():
                for i, a in enumerate(lst):
                    assert a.dtype == np.uint8
                    arrays[f"{s}_{k}_{i}"] = a

            # the conditions the tests rely on
            assert len(np.unique(np.concatenate([a.reshape(-1) for a in dec["hr"]]))) == 256, "an HR byte value is missing"
            assert any(((m != 0) & (m != 255)).any() for m in dec["mask"])
            assert all(k.shape == (K, K) and k.max() == 255 for k in dec["kernel"])
            assert len({k.tobytes() for k in dec["kernel"]}) == spec["n"] and all(not np.array_equal(k, k.T) for k in dec["kernel"])
    assert [int(arrays[f"A_b{j}_imgs"].shape[0]) for j in range(2)] == [4, 2] and arrays["A_b0_imgs"].shape[1:] == (4, 3, 4, 6)
    assert arrays["B_b0_imgs"].shape == (3, 1, 3, 8, 12) and int(arrays["B_nbatch"]) == 1
    np.savez_compressed(EC.GOLDEN, **arrays)
    size = os.path.getsize(EC.GOLDEN)
    assert size < 200_000, size
    print(f"wrote {EC.GOLDEN}: {size} bytes")


if __name__ == "__main__":
    main()
