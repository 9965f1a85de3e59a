"""Host side of the whole-test-set evaluation (csbsr_amd/data/resident_test.py, csbsr_amd/inference.py: evaluate_dataset, csrc/eval_io.hip):
the ABI declarations, the fixture recorded from the reference's CrackDataSetTest, the NumPy restatements of the two kernels against the
CPU torch chains they replace, the loader's validation, the summary formulas and the csv layout.  No GPU."""
import csv
import os
import re

import numpy as np
import pytest
import torch

import eval_io_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_declare_both_symbols():
    from csbsr_amd import _lib
    header = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    for name, nargs in (("csbsr_stitch_clip_u8", 11), ("csbsr_threshold_planes_u8", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/csbsr_hip.h"
        assert len(m.group(1).split(",")) == nargs
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.i32 and len(args) == nargs
    assert "eval_io.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()


def test_fixture_conditions():
    g = EC.load_golden()
    a, b = g["A"], g["B"]
    assert len(a["names"]) == 6 and len(b["names"]) == 3 and a["names"] == sorted(a["names"]) and b["names"] == sorted(b["names"])
    assert [len(x["fnames"]) for x in a["batches"]] == [4, 2] and [len(x["fnames"]) for x in b["batches"]] == [3]
    assert a["batches"][0]["imgs"].shape == (4, 4, 3, 4, 6) and b["batches"][0]["imgs"].shape == (3, 1, 3, 8, 12)
    assert a["batches"][0]["img_unfold_shape"].tolist() == [4, 1, 2, 2, 3, 16, 24]
    assert a["batches"][1]["seg_unfold_shape"].tolist() == [4, 1, 2, 2, 1, 16, 24]           # entry 0 stays the constructor's batch size
    assert b["batches"][0]["img_unfold_shape"].tolist() == [3, 1, 1, 1, 3, 32, 48]
    for s in (a, b):
        assert all(h.shape == (32, 48, 3) and h.dtype == np.uint8 for h in s["hr"]) and all(l.shape == (8, 12, 3) for l in s["lr"])
        assert len(np.unique(np.concatenate([h.reshape(-1) for h in s["hr"]]))) == 256
        assert any(((m != 0) & (m != 255)).any() for m in s["mask"])
        assert all(k.shape == (21, 21) and k.max() == 255 for k in s["kernel"]) and len({k.tobytes() for k in s["kernel"]}) == len(s["kernel"])
        assert any("jpg" not in f and f.endswith(".png") for x in s["batches"] for f in x["fnames"])
    assert "png_03.png" in a["batches"][1]["fnames"]                                          # every "jpg" of a name is replaced
    assert os.path.getsize(EC.GOLDEN) < 200_000


def test_restatement_reproduces_the_reference_fixture():
    g = EC.load_golden()
    for s in g.values():
        i = 0
        for x in s["batches"]:
            B = len(x["fnames"])
            items = [EC.reference_item_numpy(s["hr"][i + b], s["mask"][i + b], s["lr"][i + b], s["kernel"][i + b], s["image_size"], s["scale"],
                                             s["batch_size"]) for b in range(B)]
            for col, k in enumerate(("imgs", "sr_targets", "masks", "kernel_targets")):
                assert np.array_equal(np.stack([it[col] for it in items]), x[k]), k
            assert np.array_equal(items[0][4], x["img_unfold_shape"]) and np.array_equal(items[0][5], x["seg_unfold_shape"])
            i += B


def test_quantisation_is_mul_255_byte():
    x = torch.rand(1 << 20, generator=torch.Generator().manual_seed(0))
    assert np.array_equal(np.trunc(x.numpy() * np.float32(255)).astype(np.uint8), x.mul(255).byte().numpy())


@pytest.mark.parametrize("shape", EC.STITCH_SHAPES)
def test_stitch_restatement_equals_the_torch_chain(shape):
    v = EC.stitch_values(shape, seed=sum(shape))
    for clip in (0, 1):
        f32, u8 = EC.stitch_numpy(v, *shape, clip)
        tf, tu = EC.stitch_torch(v, *shape, clip)
        assert np.array_equal(f32.view(np.int32), tf.numpy().view(np.int32)) and np.array_equal(u8, tu.numpy())
    assert (v == 0).any() and (v == 1).any() and np.signbit(v[v == 0]).any() and (v == np.float32(1e-40)).any()
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    if v.size >= 3 * 772:
        assert np.isin(k, v).all() and np.isin(np.nextafter(k, np.float32(2)), v).all() and np.isin(np.nextafter(k, np.float32(-1)), v).all()


@pytest.mark.parametrize("hw", EC.PLANE_HW)
@pytest.mark.parametrize("S", [1, 11, 16])
def test_planes_restatement_equals_the_torch_predicate(hw, S):
    th = EC.plane_thresholds(S)
    v = EC.plane_values(3, hw, th, seed=hw + S)
    assert np.isnan(v).any() and np.isin(th, v).all()
    assert np.array_equal(EC.planes_numpy(v, th), EC.planes_torch(v, th).numpy())
    if S == 11:
        assert np.array_equal(th, torch.Tensor(EC.THRESHOLDS).numpy()[EC.SAVE_IDX])
    if S == 16:
        assert (np.diff(th) < 0).all()


def _testset(**kw):
    from csbsr_amd.data.resident_test import ResidentTestSet
    hr, masks, lr, kernels, names = EC.make_testset(3, 5, 64, 96, 4)
    d = dict(hr=hr, masks=masks, lr=lr, kernels=kernels, names=names)
    d.update(kw)
    return ResidentTestSet(d["hr"], d["masks"], d["lr"], d["kernels"], d["names"], device="cpu")


def test_loader_validation():
    from csbsr_amd import _lib
    from csbsr_amd.data.resident_test import DeviceTestLoader
    ts = _testset()
    assert ts.kernel_targets.shape == (5, 21, 21) and ts.kernel_targets.dtype == torch.float32
    ld = DeviceTestLoader(ts, (32, 48), 4, 2)
    assert len(ld) == 3 and (ld.ph, ld.pw) == (8, 12) and ld.fnames[0] == "img_00.png"
    assert ld.patch_sel.shape == (20, 5) and ld.patch_sel[5].tolist() == [1, 0, 12, 0, 0] and ld.patch_sel[6].tolist() == [1, 8, 0, 0, 0]
    with pytest.raises(_lib.CsbsrHipError):                                  # no fallback: iteration needs the GPU
        next(iter(ld))
    with pytest.raises(NotImplementedError):
        DeviceTestLoader(ts, (32, 48), 1, 2)
    with pytest.raises(ValueError, match="img_00.jpg"):                     # 64 x 96 is no multiple of 48 x 48
        DeviceTestLoader(ts, (48, 48), 4, 2)
    hr, masks, lr, kernels, names = EC.make_testset(3, 5, 64, 96, 4)
    lr[3] = lr[3][:, :20]
    with pytest.raises(ValueError, match=r"LR image.*img_03.jpg"):
        DeviceTestLoader(_testset(lr=lr), (32, 48), 4, 2)
    hr2, masks2, lr2, _, _ = EC.make_testset(4, 1, 32, 96, 4)
    hr[2], masks[2], lr = hr2[0], masks2[0], EC.make_testset(3, 5, 64, 96, 4)[2]
    lr[2] = lr2[0]
    mixed = _testset(hr=hr, masks=masks, lr=lr)
    with pytest.raises(ValueError, match=r"one batch differ.*img_02.jpg, img_03.jpg"):
        DeviceTestLoader(mixed, (32, 48), 4, 2)
    assert len(DeviceTestLoader(mixed, (32, 48), 4, 1)) == 5                 # alone in its batch the smaller image is fine


def test_from_cfg_and_from_dirs(tmp_path):
    from PIL import Image
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    g = EC.load_golden()["A"]
    dirs = {k: tmp_path / k for k in ("images", "masks", "blur/b1/lr_images", "blur/b1/kernels")}
    for d in dirs.values():
        d.mkdir(parents=True)
    for i, n in enumerate(g["names"]):                                      # (lossless containers under the reference's names)
        png = n.replace("jpg", "png")
        Image.fromarray(g["hr"][i]).save(dirs["images"] / n, format="PNG")
        Image.fromarray(g["mask"][i]).save(dirs["masks"] / n, format="PNG")
        Image.fromarray(g["lr"][i]).save(dirs["blur/b1/lr_images"] / png)
        Image.fromarray(g["kernel"][i]).save(dirs["blur/b1/kernels"] / png)
    ts = ResidentTestSet.from_dirs(str(dirs["images"]), str(dirs["masks"]), str(tmp_path / "blur"), "b1", device="cpu")
    assert ts.names == g["names"] and len(ts) == 6
    assert np.array_equal(ts.hr.pool.numpy(), np.concatenate([a.reshape(-1) for a in g["hr"]]))
    assert np.array_equal(ts.lr.pool.numpy(), np.concatenate([a.reshape(-1) for a in g["lr"]]))
    want = np.concatenate([x["kernel_targets"][:, 0] for x in g["batches"]])
    assert np.array_equal(ts.kernel_targets.numpy(), want)                  # the reference's k / torch.sum(k), bit for bit
    os.remove(dirs["blur/b1/kernels"] / "png_03.png")
    with pytest.raises(FileNotFoundError, match="png_03.png"):
        ResidentTestSet.from_dirs(str(dirs["images"]), str(dirs["masks"]), str(tmp_path / "blur"), "b1", device="cpu")
    cfg = base_cfg.clone()
    ld = DeviceTestLoader.from_cfg(cfg, ResidentTestSet([np.zeros((448, 896, 3), np.uint8)], [np.zeros((448, 896), np.uint8)],
                                                        [np.zeros((112, 224, 3), np.uint8)], [np.eye(21, dtype=np.uint8)], ["a.jpg"],
                                                        device="cpu"), 12)
    img, seg = ld.unfold_shapes(0)
    assert img.tolist() == [12, 1, 1, 2, 3, 448, 448] and seg.tolist() == [12, 1, 1, 2, 1, 448, 448] and (ld.ph, ld.pw) == (112, 112)


def test_summary_formulas():
    from csbsr_amd.inference import summarize
    rng = np.random.default_rng(0)
    psnr, ssim, kps = rng.random(7).astype(np.float32) * 30, rng.random(7).astype(np.float32), rng.random(28).astype(np.float32) * 40
    iou = rng.random((7, 99)).astype(np.float32)
    hd, msd = rng.random((7, 99)) * 50, rng.random((7, 99)) * 20
    s = summarize(psnr, ssim, kps, iou, hd, msd)
    f = lambda a: a.astype(np.float64)
    want = {"PSNR_mean": f(psnr).mean(), "SSIM_mean": f(ssim).mean(), "PSNR(Kernel)_mean": f(kps).mean(), "AIU_mean": f(iou).mean(),
            "IoU_max": f(iou).mean(0).max(), "HD95_mean": hd.mean(), "MSD_mean": msd.mean(), "HD95_median": np.median(hd),
            "MSD_median": np.median(msd), "HD95_min": hd.mean(0).min()}
    assert set(s) == set(want) and all(s[k] == want[k] and isinstance(s[k], float) for k in want)
    assert set(summarize(psnr, ssim, kps, iou)) == {"PSNR_mean", "SSIM_mean", "PSNR(Kernel)_mean", "AIU_mean", "IoU_max"}
    # the best threshold of the MEAN curve, not the mean of the per-image optima
    iou2 = np.array([[0.9, 0.5, 0.1], [0.1, 0.5, 0.9]], np.float32)
    hd2 = np.array([[1.0, 5.0, 9.0], [9.0, 5.0, 1.0]])
    s2 = summarize([1.0], [1.0], [1.0], iou2, hd2, hd2)
    assert s2["IoU_max"] == np.float64(np.float32(0.5)) and f(iou2).max(1).mean() > 0.89
    assert s2["HD95_min"] == 5.0 and hd2.min(1).mean() == 1.0


def test_classification_scores_equal_the_reference_formulas():
    from csbsr_amd.inference import classification_counts, classification_scores
    rng = np.random.default_rng(1)
    masks = torch.from_numpy(rng.choice(np.array([0, 7, 254, 255], np.uint8), size=(3, 1, 9, 11)).astype(np.float32)) / 255
    masks[1] = 0                                                            # no ground pixel: sens is 0 / 0
    seg = torch.from_numpy(rng.random((3, 1, 9, 11)).astype(np.float32))
    th = torch.tensor(0.5, dtype=torch.float32)
    acc, sens, spec = classification_scores(classification_counts(seg, masks, th).numpy())
    want = EC.retinal_numpy((seg[:, 0] - th > 0).float().numpy(), masks.numpy())
    for a, w in zip((acc, sens, spec), want):
        assert a.dtype == np.float64 and np.array_equal(a, w, equal_nan=True)
    assert np.isnan(sens[1]) and not np.isnan(sens[[0, 2]]).any()


def test_csv_layout(tmp_path):
    from csbsr_amd.inference import write_iou_log
    rng = np.random.default_rng(2)
    iou = rng.random((4, 99)).astype(np.float32)
    iou[0, 0], iou[1, 1] = 1e-5, 1.0
    names = [f"img_{i}.png" for i in range(4)]
    path = tmp_path / "iou_log.csv"
    write_iou_log(str(path), iou, EC.THRESHOLDS, names)
    rows = list(csv.reader(open(path, newline="")))
    assert len(rows) == 5 and all(len(r) == 100 for r in rows) and rows[0][0] == ""
    assert [float(c) for c in rows[0][1:]] == EC.THRESHOLDS
    assert [r[0] for r in rows[1:]] == names
    assert np.array_equal(np.array([[np.float32(c) for c in r[1:]] for r in rows[1:]]), iou)


def test_stub_conditions():
    """What the GPU test of evaluate_dataset relies on: the stub's map gives at least 30 distinct IoU columns and no saved plane is
    constant for more than 2 of the 11 thresholds; the SR output leaves [0, 1] on both sides."""
    hr, masks, lr, kernels, names = EC.make_testset(11, 5, 64, 96, 4, zero_mask=3)
    th = EC.thresholds32()
    for i in range(5):
        it = EC.reference_item_numpy(hr[i], masks[i], lr[i], kernels[i], (32, 48), 4, 2)
        c = EC.cpu_chain([it], 1)
        assert (c["planes"].reshape(11, -1).min(1) == c["planes"].reshape(11, -1).max(1)).sum() <= 2
        sr_raw = EC.stitch_torch(EC.stub_model(torch.from_numpy(it[0]))[0], 1, 3, 2, 2, 32, 48, False)[0]
        assert float(sr_raw.max()) > 1 and float(sr_raw.min()) < 0
        if i != 3:
            seg, m = c["seg"].numpy().reshape(-1), it[2].reshape(-1) > 0.5
            bi = (seg[None, :] - th[:, None]) > 0
            iou = (bi & m).sum(1) / (bi | m).sum(1)
            assert len(np.unique(iou)) >= 30
    assert not masks[3].any() and any(((m != 0) & (m != 255)).any() for m in masks)
