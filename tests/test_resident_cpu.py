"""Host side of the HBM-resident training loader (csbsr_amd/data/resident.py), no GPU: the ABI declaration, the fixture recorded from
the reference's transforms against the NumPy restatement, the sampler, the augmentation table of TrainTransforms, from_dirs, split and
the host validation of the selection table."""
import os
import re

import numpy as np
import pytest
import torch

import resident_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(40, 52), (31, 45), (24, 32), (50, 33), (37, 64), (29, 41), (44, 36)]


@pytest.fixture(scope="module")
def R():
    from csbsr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "csbsr_amd", "csrc"), "-j8"], check=True)
    from csbsr_amd.data import resident
    return resident


def make_dataset(R, sizes=SIZES, seed=0):
    images, masks = RC.random_pairs(np.random.default_rng(seed), sizes)
    return R.ResidentDataset(images, masks, device="cpu"), images, masks


def test_header_and_signatures_name_the_gather():
    from csbsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    assert re.search(r"\bint\s+csbsr_gather_crop_u8\s*\(", hdr)
    res, args = _lib.SIGNATURES["csbsr_gather_crop_u8"]
    assert res is _lib.i32 and len(args) == 10
    assert "resident.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()


def test_fixture_conditions():
    g = RC.load_golden()
    sizes = [a.shape[:2] for a in g["images"]]
    h, w = g["crop"]
    assert len(sizes) >= 6 and len(set(sizes)) == len(sizes) and all(H != W for H, W in sizes) and h != w
    sel = g["sel"]
    assert {(int(r[3]), int(r[4])) for r in sel} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    span = np.array([[sizes[r[0]][0] - h, sizes[r[0]][1] - w] for r in sel])
    assert (sel[:, 1] == 0).any() and (sel[:, 2] == 0).any()
    assert ((sel[:, 1] == span[:, 0]) & (span[:, 0] > 0)).any() and ((sel[:, 2] == span[:, 1]) & (span[:, 1] > 0)).any()
    assert len(np.unique(np.round(g["out_image"] * 255).astype(np.int64))) == 256          # a reciprocal multiply cannot pass
    assert os.path.getsize(RC.GOLDEN) < 200 * 1024


def test_numpy_restatement_reproduces_the_fixture():
    g = RC.load_golden()
    h, w = g["crop"]
    assert np.array_equal(RC.gather_numpy(g["images"], g["sel"], h, w), g["out_image"])
    assert np.array_equal(RC.gather_numpy(g["masks"], g["sel"], h, w), g["out_mask"])
    # and the fixture does tell a reciprocal multiply from the division
    recip = RC.gather_numpy(g["images"], g["sel"], h, w) * 0 + np.float32(1.0 / 255) * np.round(g["out_image"] * 255).astype(np.float32)
    assert not np.array_equal(recip, g["out_image"])


def test_pool_layout(R):
    ds, images, masks = make_dataset(R)
    assert len(ds) == len(SIZES)
    px = sum(H * W for H, W in SIZES)
    assert ds.nbytes == 4 * px and ds.image_pool.numel() == 3 * px and ds.mask_pool.numel() == px
    assert ds.image_pool.dtype == torch.uint8 and ds.image_pool.is_contiguous()
    assert np.array_equal(ds.dims, np.array(SIZES, np.int32))
    for i in range(len(ds)):
        a, m = ds.sample(i)
        assert np.array_equal(a, images[i]) and np.array_equal(m[:, :, 0], masks[i])
        o = int(ds.image_offsets[i])
        assert np.array_equal(ds.image_pool[o:o + a.size].numpy(), images[i].reshape(-1))
    with pytest.raises(ValueError):
        R.ResidentDataset(images[:2], [masks[1], masks[0]], device="cpu")              # sizes differ within a pair
    with pytest.raises(TypeError):
        R.ResidentDataset([images[0].astype(np.float32)], masks[:1], device="cpu")


def test_subset_and_split(R):
    ds, images, _ = make_dataset(R, sizes=[(20 + i, 30 + 2 * i) for i in range(23)])
    sub = ds.subset([5, 2, 9])
    assert len(sub) == 3 and sub.image_pool.data_ptr() == ds.image_pool.data_ptr()
    assert np.array_equal(sub.sample(1)[0], images[2])
    assert np.array_equal(sub.subset([2]).sample(0)[0], images[9])
    a, b = ds.split(0.8, seed=3)
    assert len(a) == int(23 * 0.8) and len(b) == 23 - int(23 * 0.8)
    assert not set(a.indices) & set(b.indices) and set(a.indices) | set(b.indices) == set(range(23))
    a2, b2 = ds.split(0.8, seed=3)
    assert np.array_equal(a.indices, a2.indices) and np.array_equal(b.indices, b2.indices)
    assert not np.array_equal(a.indices, ds.split(0.8, seed=4)[0].indices)
    assert a.image_pool.data_ptr() == ds.image_pool.data_ptr()
    with pytest.raises(IndexError):
        ds.subset([23])


def epoch_indices(loader):
    return [sel[:, 0].tolist() for sel, _ in loader.iter_decisions()]


def test_epoch_is_a_permutation_and_last_batch_short(R):
    ds, _, _ = make_dataset(R, sizes=[(20 + i % 5, 30 + i % 7) for i in range(23)])
    ld = R.DeviceTrainLoader(ds, (16, 24), 4, batch_size=6, seed=1)
    batches = epoch_indices(ld)
    assert [len(b) for b in batches] == [6, 6, 6, 5] and len(ld) == 4
    assert sorted(sum(batches, [])) == list(range(23))
    assert sum(batches, []) != list(range(23))
    ld = R.DeviceTrainLoader(ds, (16, 24), 4, batch_size=6, seed=1, drop_last=True)
    batches = epoch_indices(ld)
    assert [len(b) for b in batches] == [6, 6, 6] and len(ld) == 3 and len(set(sum(batches, []))) == 18


def test_num_iterations_across_epochs(R):
    ds, _, _ = make_dataset(R, sizes=[(20 + i % 5, 30 + i % 7) for i in range(10)])
    ld = R.DeviceTrainLoader(ds, (16, 24), 4, batch_size=4, num_iterations=8, seed=2)
    batches = epoch_indices(ld)
    assert [len(b) for b in batches] == [4, 4, 2, 4, 4, 2, 4, 4] and len(ld) == 8             # batches never span an epoch
    assert sorted(sum(batches[:3], [])) == list(range(10)) and sorted(sum(batches[3:6], [])) == list(range(10))
    assert sum(batches[:3], []) != sum(batches[3:6], [])                                   # a fresh permutation per epoch
    ld = R.DeviceTrainLoader(ds, (16, 24), 4, batch_size=4, num_iterations=5, seed=2, drop_last=True)
    assert [len(b) for b in epoch_indices(ld)] == [4] * 5
    ld = R.DeviceTrainLoader(ds, (16, 24), 4, batch_size=4, num_iterations=2, seed=2)
    assert [len(b) for b in epoch_indices(ld)] == [4, 4]


def test_shards_are_disjoint_and_cover(R):
    ds, _, _ = make_dataset(R, sizes=[(20 + i % 5, 30 + i % 7) for i in range(23)])
    sub = ds.subset(list(range(22, 0, -1)))
    seen = []
    for rank in range(3):
        ld = R.DeviceTrainLoader(sub, (16, 24), 4, batch_size=4, seed=5, shard=(rank, 3))
        mine = sum(epoch_indices(ld), [])
        assert sorted(mine) == sorted(sub.indices[rank::3].tolist())
        seen.append(set(mine))
    assert not (seen[0] & seen[1]) and not (seen[0] & seen[2]) and not (seen[1] & seen[2])
    assert seen[0] | seen[1] | seen[2] == set(range(1, 23))
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(sub, (16, 24), 4, batch_size=4, shard=(3, 3))


def test_same_seed_same_tables(R):
    ds, _, _ = make_dataset(R)
    mk = lambda seed: R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=3, num_iterations=7, seed=seed, vflip_p=0.4)
    a, b, c = (list(mk(s).iter_decisions()) for s in (11, 11, 12))
    assert len(a) == len(b) == 7
    for (s1, p1), (s2, p2) in zip(a, b):
        assert s1.dtype == torch.int32 and p1.dtype == torch.float32 and p1.shape == (s1.shape[0], 3)
        assert torch.equal(s1, s2) and torch.equal(p1, p2)
    assert any(not torch.equal(s1, s3) for (s1, _), (s3, _) in zip(a, c))


def test_offsets_in_range_and_reach_both_ends(R):
    ds, _, _ = make_dataset(R)
    h, w = 24, 32                                      # image 2 is exactly the crop
    ld = R.DeviceTrainLoader(ds, (h, w), 4, batch_size=7, num_iterations=400, seed=4, vflip_p=0.5)
    rows = np.concatenate([sel.numpy() for sel, _ in ld.iter_decisions()])
    ds.check_selection(rows, h, w)
    span = ds.dims[rows[:, 0]] - np.array([h, w])
    assert (rows[:, 1] >= 0).all() and (rows[:, 1] <= span[:, 0]).all() and (rows[:, 2] >= 0).all() and (rows[:, 2] <= span[:, 1]).all()
    for i in range(len(ds)):
        r = rows[rows[:, 0] == i]
        assert set(r[:, 1]) == set(range(SIZES[i][0] - h + 1)) and set(r[:, 2]) == set(range(SIZES[i][1] - w + 1))
    _, params = ld.draw(5)
    assert ((params[:, :2] >= 0.2) & (params[:, :2] <= 4.0)).all() and ((params[:, 2] >= 0) & (params[:, 2] <= np.pi)).all()


def test_mirror_and_vflip_frequencies(R):
    ds, _, _ = make_dataset(R)
    n = 20000
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=7, seed=9, vflip_p=0.3)
    rows = []
    while sum(len(r) for r in rows) < n:
        rows.append(ld.draw(7)[0].numpy())
    rows = np.concatenate(rows)[:n]
    sd = lambda p: np.sqrt(p * (1 - p) / n)
    assert abs(rows[:, 3].mean() - 0.5) <= 5 * sd(0.5)
    assert abs(rows[:, 4].mean() - 0.3) <= 5 * sd(0.3)          # vflip_p is the probability that the flip happens
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=7, seed=9)
    assert not np.concatenate([ld.draw(7)[0].numpy() for _ in range(50)])[:, 4].any()


# ---------------------------------------------------------------------------------------------------- augmentation table
def test_augmentation_default_is_the_shipped_yaml(R):
    dims = np.array(SIZES)
    want = [("ConvertFromInts", None), ("RandomMirror", None), ("ToTensor", None), ("RandomVerticalFlip", 0.3), ("RandomCrop", None)]
    assert [tuple(e) for e in R.DEFAULT_AUGMENTATION] == want
    assert R.interpret_augmentation(R.DEFAULT_AUGMENTATION, (24, 32), dims) == {"mirror_p": 0.5, "crop": True}


def test_augmentation_folded_entries_and_yaml_none(R):
    same = np.array([(24, 32)] * 3)
    assert R.interpret_augmentation([["ConvertFromInts", "None"], ["ToTensor", "None"]], (24, 32), same) == {"mirror_p": 0.0, "crop": False}
    assert R.interpret_augmentation([["ConvertFromInts", None], ["RandomMirror", "None"], ["ToTensor", None]], (24, 32), same)["mirror_p"] == 0.5
    with pytest.raises(ValueError):                    # no crop entry: the images must already have the crop size
        R.interpret_augmentation([["ConvertFromInts", None], ["ToTensor", None]], (24, 32), np.array(SIZES))


def test_augmentation_random_crop(R):
    out = R.interpret_augmentation([["ToTensor", None], ["RandomCrop", None]], (24, 32), np.array(SIZES))
    assert out == {"mirror_p": 0.0, "crop": True}


def test_augmentation_random_resized_crop_identity_only(R):
    same = np.array([(24, 32)] * 3)
    entry = ["RandomResizedCrop", [{"scale": (1.0, 1.0), "ratio": (1.0, 1.0)}]]
    assert R.interpret_augmentation([["ToTensor", None], entry], (24, 32), same)["crop"]
    assert R.interpret_augmentation([["RandomResizedCrop", {"scale": [1.0, 1.0], "ratio": [1.0, 1.0]}]], (24, 32), same)["crop"]
    with pytest.raises(NotImplementedError):           # images of other sizes: it would resample
        R.interpret_augmentation([entry], (24, 32), np.array(SIZES))
    with pytest.raises(NotImplementedError):
        R.interpret_augmentation([["RandomResizedCrop", [{"scale": (0.5, 1.0), "ratio": (1.0, 1.0)}]]], (24, 32), same)


def test_augmentation_entry_with_argument_is_dropped(R):
    """the yaml's ["RandomVerticalFlip", 0.3] is constructed and thrown away by the reference: no vertical flip is ever drawn"""
    ds, _, _ = make_dataset(R)
    aug = [["ConvertFromInts", None], ["RandomMirror", None], ["ToTensor", None], ["RandomVerticalFlip", 0.3], ["RandomGrayscale", {"p": 0.25}],
           ["RandomCrop", None]]
    assert R.interpret_augmentation(aug, (24, 32), ds.dims) == {"mirror_p": 0.5, "crop": True}
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=7, seed=1, augmentation=aug)
    rows = np.concatenate([ld.draw(7)[0].numpy() for _ in range(100)])
    assert not rows[:, 4].any() and rows[:, 3].any() and not rows[:, 3].all()
    # a dropped entry has no effect wherever it stands, after the crop included; an entry that would act there is refused
    late = [["ConvertFromInts", None], ["RandomMirror", None], ["ToTensor", None], ["RandomCrop", None], ["RandomVerticalFlip", 0.3]]
    assert R.interpret_augmentation(late, (24, 32), ds.dims) == {"mirror_p": 0.5, "crop": True}
    with pytest.raises(NotImplementedError):
        R.interpret_augmentation([["ToTensor", None], ["RandomCrop", None], ["RandomMirror", None]], (24, 32), ds.dims)
    with pytest.raises(NotImplementedError):
        R.interpret_augmentation([["ToTensor", None], ["RandomCrop", None], ["RandomCrop", None]], (24, 32), ds.dims)


def test_augmentation_unknown_and_unsupported_names(R):
    dims = np.array(SIZES)
    with pytest.raises(NotImplementedError):
        R.interpret_augmentation([["ToTensor", None], ["RandomRotate90", None], ["RandomCrop", None]], (24, 32), dims)
    with pytest.raises(NotImplementedError):           # unknown even with an argument: eval(func) fails in the reference too
        R.interpret_augmentation([["NoSuchTransform", 0.5], ["RandomCrop", None]], (24, 32), dims)
    with pytest.raises(NotImplementedError):           # a real transform of the reference that no shipped config enables
        R.interpret_augmentation([["PhotometricDistort", None], ["RandomCrop", None]], (24, 32), dims)
    with pytest.raises(NotImplementedError):
        R.DeviceTrainLoader(make_dataset(R)[0], (24, 32), 4, batch_size=2, augmentation=[["RandomRotate90", None], ["RandomCrop", None]])


def test_from_cfg_reads_the_augmentation_node(R):
    from csbsr_amd.config import cfg as base
    assert "DATASET" not in base                        # the default tree gains no keys
    ds, _, _ = make_dataset(R, sizes=[(448, 448)] * 2 + [(450, 460)])
    c = base.clone()
    ld = R.DeviceTrainLoader.from_cfg(c, ds, seed=0)
    assert (ld.h, ld.w, ld.scale, ld.K, ld.batch_size, ld.num_iterations, ld.mirror_p) == (448, 448, 4, 21, 8, 300000, 0.5)
    c._merge({"DATASET": {"DATA_AUGMENTATION": [["ConvertFromInts", "None"], ["ToTensor", "None"], ["RandomCrop", "None"]]}})
    assert R.DeviceTrainLoader.from_cfg(c, ds, seed=0).mirror_p == 0.0


# ---------------------------------------------------------------------------------------------------- files
def test_from_dirs_round_trip(R, tmp_path):
    from PIL import Image
    images, masks = RC.random_pairs(np.random.default_rng(8), SIZES[:4])
    (tmp_path / "images").mkdir()
    (tmp_path / "masks").mkdir()
    names = ["b.png", "a.png", "d.png", "c.png"]
    for n, a, m in zip(names, images, masks):
        Image.fromarray(a).save(tmp_path / "images" / n)
        Image.fromarray(m).save(tmp_path / "masks" / n)
    ds = R.ResidentDataset.from_dirs(str(tmp_path / "images"), str(tmp_path / "masks"), pattern="*.png", device="cpu")
    assert len(ds) == 4 and ds.names == sorted(names)
    for i, n in enumerate(ds.names):
        a, m = ds.sample(i)
        assert np.array_equal(a, images[names.index(n)]) and np.array_equal(m[:, :, 0], masks[names.index(n)])
    os.remove(tmp_path / "masks" / "c.png")
    with pytest.raises(FileNotFoundError, match="c.png"):
        R.ResidentDataset.from_dirs(str(tmp_path / "images"), str(tmp_path / "masks"), pattern="*.png", device="cpu")
    with pytest.raises(FileNotFoundError):
        R.ResidentDataset.from_dirs(str(tmp_path / "images"), str(tmp_path / "masks"), device="cpu")      # no *.jpg there


@pytest.mark.parametrize("which,mode", [("images", "L"), ("images", "RGBA"), ("images", "P"), ("masks", "1"), ("masks", "RGB"), ("masks", "I;16")])
def test_from_dirs_rejects_other_pixel_formats_by_name(R, tmp_path, which, mode):
    """files are taken as PIL decodes them (the reference's np.array(Image.open(...))): nothing is converted silently"""
    from PIL import Image
    images, masks = RC.random_pairs(np.random.default_rng(8), SIZES[:2])
    (tmp_path / "images").mkdir()
    (tmp_path / "masks").mkdir()
    for n, a, m in zip(["a.png", "odd.png"], images, masks):
        ia, im = Image.fromarray(a), Image.fromarray(m)
        if n == "odd.png":
            if which == "images":
                ia = ia.convert(mode)
            else:
                im = im.convert(mode)
        ia.save(tmp_path / "images" / n)
        im.save(tmp_path / "masks" / n)
    with pytest.raises(ValueError, match="odd.png"):
        R.ResidentDataset.from_dirs(str(tmp_path / "images"), str(tmp_path / "masks"), pattern="*.png", device="cpu")


# ---------------------------------------------------------------------------------------------------- host validation
@pytest.mark.parametrize("row", [(7, 0, 0, 0, 0), (-1, 0, 0, 0, 0), (0, -1, 0, 0, 0), (0, 0, -1, 0, 0), (0, 17, 0, 0, 0), (0, 0, 21, 0, 0),
                                 (2, 1, 0, 0, 0), (2, 0, 1, 1, 1), (0, 0, 0, 2, 0), (0, 0, 0, 0, -1)])
def test_bad_selection_rows_are_rejected(R, row):
    ds, _, _ = make_dataset(R)                          # image 0 is 40 x 52, image 2 exactly 24 x 32
    ds.check_selection(np.array([(0, 16, 20, 1, 1), (2, 0, 0, 0, 1)], np.int32), 24, 32)
    with pytest.raises(ValueError):
        ds.check_selection(np.array([(0, 16, 20, 1, 1), row], np.int32), 24, 32)
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=2, seed=0)
    with pytest.raises(ValueError):                    # batch() validates before anything is uploaded
        ld.batch(torch.tensor([row], dtype=torch.int32), torch.ones(1, 3))


def test_selection_table_shape_and_type(R):
    ds, _, _ = make_dataset(R)
    with pytest.raises(ValueError):
        ds.check_selection(np.zeros((2, 4), np.int32), 24, 32)
    with pytest.raises(ValueError):
        ds.check_selection(np.zeros((2, 5), np.float32), 24, 32)


def test_loader_argument_checks(R):
    ds, _, _ = make_dataset(R)
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(ds, (24, 30), 4, batch_size=2)          # not a multiple of the scale
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(ds, (28, 32), 4, batch_size=2)          # image 2 is smaller than the crop
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=2, vflip_p=1.5)


def test_no_batches_without_a_gpu(R):
    """the pool may sit on the host for the tests above, but there is no host path for the batch itself"""
    from csbsr_amd._lib import CsbsrHipError
    ds, _, _ = make_dataset(R)
    ld = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=2, seed=0)
    with pytest.raises(CsbsrHipError):
        ld.batch(*ld.draw(2))
