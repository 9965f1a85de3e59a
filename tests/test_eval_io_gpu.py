"""Whole-test-set evaluation on the device (csrc/eval_io.hip, csbsr_amd/data/resident_test.py, csbsr_amd/inference.py: evaluate_dataset):
the two kernels against the CPU torch chains they replace, bit for bit and with guard bands; the loader against the fixture recorded from
the reference's CrackDataSetTest; evaluate_dataset against per-batch evaluate_batch, the reference's report formulas and the files
``test.py --sf_save_image`` writes."""
import csv
import ctypes as C
import os

import numpy as np
import pytest
import torch

import eval_io_cases as EC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256


def guarded(shape, dtype):
    """(view, whole): a tensor of ``shape`` inside a larger 0xA5-filled byte buffer, 256 bytes of guard on either side."""
    nb = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    whole = torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return whole[GUARD:GUARD + nb].view(dtype).view(*shape), whole


def guards_intact(whole):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[-GUARD:] == 0xA5).all())


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("shape", EC.STITCH_SHAPES)
def test_stitch_equals_the_torch_chain(shape):
    from csbsr_amd import _lib as L
    B, Cc, nH, nW, ph, pw = shape
    v = EC.stitch_values(shape, seed=sum(shape))
    p = torch.from_numpy(v).to(DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for clip in (0, 1):
        want_f, want_u = EC.stitch_torch(v, *shape, clip)
        for f_on, u_on in ((True, True), (True, False), (False, True)):
            f32, wf = guarded((B, Cc, nH * ph, nW * pw), torch.float32)
            u8, wu = guarded((B, nH * ph, nW * pw, Cc), torch.uint8)
            L.call("csbsr_stitch_clip_u8", _ptr(p), B, Cc, nH, nW, ph, pw, clip, _ptr(f32 if f_on else None), _ptr(u8 if u_on else None), st)
            torch.cuda.synchronize()
            assert guards_intact(wf) and guards_intact(wu)
            if f_on:
                assert torch.equal(f32.cpu(), want_f) and torch.equal(f32.cpu().view(torch.int32), want_f.view(torch.int32))
            else:
                assert bool((wf == 0xA5).all())
            if u_on:
                assert torch.equal(u8.cpu(), want_u)
            else:
                assert bool((wu == 0xA5).all())
    with pytest.raises(L.CsbsrHipError):
        L.call("csbsr_stitch_clip_u8", _ptr(p), B, Cc, nH, nW, ph, pw, 1, None, None, st)
    with pytest.raises(L.CsbsrHipError):
        L.call("csbsr_stitch_clip_u8", _ptr(p), B, 2, nH, nW, ph, pw, 1, _ptr(p), None, st)


def test_stitch_nan_and_the_python_wrapper():
    from csbsr_amd.inference import stitch_clip_u8
    shape = (2, 3, 2, 3, 8, 12)
    v = EC.stitch_values(shape, seed=5)
    v.reshape(-1)[[3, 700, 2001]] = np.nan
    f32, u8 = stitch_clip_u8(torch.from_numpy(v).to(DEV), (7, 1, 2, 3, 3, 8, 12), clip=True, want_u8=True)
    want_f, want_u = EC.stitch_numpy(v, *shape, 1)
    assert np.array_equal(f32.cpu().numpy(), want_f, equal_nan=True) and int(np.isnan(want_f).sum()) == 3
    assert np.array_equal(u8.cpu().numpy(), want_u) and (want_u[np.isnan(want_f).transpose(0, 2, 3, 1)] == 0).all()


@pytest.mark.parametrize("hw", EC.PLANE_HW)
@pytest.mark.parametrize("S", [1, 11, 16])
def test_threshold_planes_equal_the_torch_predicate(hw, S):
    from csbsr_amd import _lib as L
    th = EC.plane_thresholds(S)
    v = EC.plane_values(3, hw, th, seed=hw + S)
    out, whole = guarded((3, S, hw), torch.uint8)
    p, t = torch.from_numpy(v).to(DEV), torch.from_numpy(th).to(DEV)
    L.call("csbsr_threshold_planes_u8", _ptr(p), _ptr(t), 3, hw, S, _ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert guards_intact(whole)
    assert torch.equal(out.cpu(), EC.planes_torch(v, th))
    for bad in (0, 17):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_threshold_planes_u8", _ptr(p), _ptr(t), 3, hw, bad, _ptr(out), None)


@pytest.mark.parametrize("which", ["A", "B"])
def test_loader_reproduces_the_reference_fixture(which):
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    g = EC.load_golden()[which]
    ts = ResidentTestSet(g["hr"], g["mask"], g["lr"], g["kernel"], g["names"], device=DEV)
    ld = DeviceTestLoader(ts, g["image_size"], g["scale"], g["batch_size"])
    got = list(ld)
    assert [len(b[4]) for b in got] == [len(x["fnames"]) for x in g["batches"]] == ([4, 2] if which == "A" else [3])
    for b, x in zip(got, g["batches"]):
        imgs, sr_t, masks, kt, fnames, img_shape, seg_shape = b
        assert list(fnames) == x["fnames"]
        for t, k in ((imgs, "imgs"), (sr_t, "sr_targets"), (masks, "masks"), (kt, "kernel_targets")):
            assert t.is_cuda and t.dtype == torch.float32 and torch.equal(t.cpu(), torch.from_numpy(x[k])), k
        assert np.array_equal(img_shape, x["img_unfold_shape"]) and np.array_equal(seg_shape, x["seg_unfold_shape"])
        assert img_shape.ndim == 1 and img_shape.dtype == x["img_unfold_shape"].dtype
        assert kt.is_contiguous() and kt.view(-1, 1, 21, 21).shape[0] == imgs.shape[0] * imgs.shape[1]


@pytest.fixture(scope="module")
def stub_set():
    hr, masks, lr, kernels, names = EC.make_testset(11, 5, 64, 96, 4, zero_mask=3)
    items = [EC.reference_item_numpy(hr[i], masks[i], lr[i], kernels[i], (32, 48), 4, 2) for i in range(5)]
    return dict(hr=hr, masks=masks, lr=lr, kernels=kernels, names=names, items=items)


def _loader(d, idx, batch=2, image_size=(32, 48)):
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    ts = ResidentTestSet(*[[d[k][i] for i in idx] for k in ("hr", "masks", "lr", "kernels", "names")], device=DEV)
    return DeviceTestLoader(ts, image_size, 4, batch)


def _per_batch(model, loader, **kw):
    from csbsr_amd.inference import evaluate_batch
    return [evaluate_batch(model, imgs, s1, s2, sr_t, m, kt, ksize=21, **kw) for imgs, sr_t, m, kt, _, s1, s2 in loader]


def test_evaluate_dataset_with_the_stub(stub_set, tmp_path):
    from PIL import Image
    from csbsr_amd.inference import evaluate_dataset, summarize
    d, idx = stub_set, list(range(5))
    out = evaluate_dataset(EC.stub_model, _loader(d, idx), classification=True, save_dir=str(tmp_path))
    plain = evaluate_dataset(EC.stub_model, _loader(d, idx))
    ref = _per_batch(EC.stub_model, _loader(d, idx))
    assert out["fnames"] == [f"img_{i:02d}.png" for i in range(5)] and len(ref) == 3
    for k, shape in (("psnr", (5,)), ("ssim", (5,)), ("kernel_psnr", (20,)), ("iou", (5, 99))):
        want = np.concatenate([r[k] for r in ref])
        assert out[k].shape == shape and out[k].dtype == want.dtype and out[k].tobytes() == want.tobytes(), k
        assert plain[k].tobytes() == want.tobytes(), k
    assert out["summary"] == summarize(out["psnr"], out["ssim"], out["kernel_psnr"], out["iou"]) == plain["summary"]
    assert out["summary"]["AIU_mean"] == np.mean(out["iou"].astype(np.float64))
    assert out["summary"]["IoU_max"] == out["iou"].astype(np.float64).mean(0).max()
    assert set(plain) == {"fnames", "psnr", "ssim", "kernel_psnr", "iou", "summary"}
    assert len(np.unique(out["iou"][0])) >= 30

    # per-batch CPU chain: the stub on the reference's restated tensors, JointPatch, masked clips, mul(255).byte()
    chains = [EC.cpu_chain(d["items"][i0:i0 + 2], len(d["items"][i0:i0 + 2])) for i0 in (0, 2, 4)]
    seg = torch.cat([c["seg"] for c in chains])
    masks = torch.from_numpy(np.stack([it[2] for it in d["items"]]))
    th49 = torch.from_numpy(EC.thresholds32())[49]
    want = EC.retinal_numpy((seg[:, 0] - th49 > 0).float().numpy(), masks.numpy())
    for k, w in zip(("acc", "sens", "spec"), want):
        assert out[k].dtype == np.float64 and np.array_equal(out[k], w, equal_nan=True), k
    assert np.isnan(out["sens"][3]) and np.isfinite(np.delete(out["sens"], 3)).all()

    th_dirs = [f"th_{EC.THRESHOLDS[i]:.2f}" for i in EC.SAVE_IDX]
    assert sorted(os.listdir(tmp_path / "masks")) == sorted(th_dirs + ["th_-1.00"]) and len(th_dirs) == 11
    assert th_dirs[:3] == ["th_0.01", "th_0.10", "th_0.20"] and th_dirs[-1] == "th_0.99"
    assert sorted(os.listdir(tmp_path)) == ["images", "iou_log.csv", "kernels", "kernels_origin", "masks"]
    sr_u8 = np.concatenate([c["sr_u8"] for c in chains])
    raw_u8 = np.concatenate([c["raw_u8"] for c in chains])
    planes = np.concatenate([c["planes"] for c in chains])
    kp = torch.cat([c["kernel_preds"] for c in chains])
    assert sr_u8.min() == 0 and sr_u8.max() == 255
    for b, name in enumerate(out["fnames"]):
        im = Image.open(tmp_path / "images" / name)
        assert im.mode == "RGB" and np.array_equal(np.array(im), sr_u8[b])
        for j, t in enumerate(th_dirs):
            im = Image.open(tmp_path / "masks" / t / name)
            assert im.mode == "L" and np.array_equal(np.array(im), planes[b, j]), (name, t)
        assert np.array_equal(np.array(Image.open(tmp_path / "masks" / "th_-1.00" / name)), raw_u8[b])
        for j in range(4):
            k = kp[b * 4 + j]
            stem = name.replace(".png", "")
            assert np.array_equal(np.array(Image.open(tmp_path / "kernels" / f"{stem}_{j}.png")), (k / torch.max(k)).mul(255).byte().numpy()[0])
            assert np.array_equal(np.array(Image.open(tmp_path / "kernels_origin" / f"{stem}_{j}_origin.png")),
                                  (k / torch.sum(k)).mul(255).byte().numpy()[0])
    assert len(os.listdir(tmp_path / "images")) == 5 and len(os.listdir(tmp_path / "kernels")) == 20
    rows = list(csv.reader(open(tmp_path / "iou_log.csv", newline="")))
    assert [r[0] for r in rows[1:]] == out["fnames"] and [float(c) for c in rows[0][1:]] == EC.THRESHOLDS
    assert np.array_equal(np.array([[np.float32(c) for c in r[1:]] for r in rows[1:]]), out["iou"])


def test_evaluate_dataset_surface_distance(stub_set):
    from csbsr_amd.inference import evaluate_dataset, summarize
    d, idx = stub_set, [0, 1, 3]                                            # (image 3 has the empty mask: degenerate cells, outliers)
    out = evaluate_dataset(EC.stub_model, _loader(d, idx), surface_distance=True)
    ref = _per_batch(EC.stub_model, _loader(d, idx), surface_distance=True)
    for k in ("hd", "msd"):
        want = np.concatenate([r[k] for r in ref])
        assert out[k].shape == (3, 99) and out[k].dtype == np.float64 and out[k].tobytes() == want.tobytes(), k
    assert out["hd_outliers"] == sum(r["hd_outliers"] for r in ref) and out["msd_outliers"] == sum(r["msd_outliers"] for r in ref)
    assert out["hd_outliers"] > 0
    assert out["iou"].tobytes() == np.concatenate([r["iou"] for r in ref]).tobytes()
    s = summarize(out["psnr"], out["ssim"], out["kernel_psnr"], out["iou"], out["hd"], out["msd"])
    assert out["summary"] == s and s["HD95_min"] == out["hd"].mean(0).min() and s["MSD_median"] == np.median(out["msd"])


def test_evaluate_dataset_with_the_real_model():
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.inference import evaluate_dataset
    from csbsr_amd.modeling.build_model import JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    m = JointModel(base_cfg.clone())
    deterministic_fill(m.state_dict())
    m.eval()
    hr, masks, lr, kernels, names = EC.make_testset(7, 3, 128, 128, 4)
    d = dict(hr=hr, masks=masks, lr=lr, kernels=kernels, names=names)
    a = evaluate_dataset(m, _loader(d, [0, 1, 2], image_size=64))
    b = evaluate_dataset(m, _loader(d, [0, 1, 2], image_size=64))
    ref = _per_batch(m, _loader(d, [0, 1, 2], image_size=64))
    assert [len(r["psnr"]) for r in ref] == [2, 1]
    for k, shape in (("psnr", (3,)), ("ssim", (3,)), ("kernel_psnr", (12,)), ("iou", (3, 99))):
        assert a[k].shape == shape and np.isfinite(a[k]).all()
        assert a[k].tobytes() == b[k].tobytes() == np.concatenate([r[k] for r in ref]).tobytes(), k
    assert a["summary"] == b["summary"] and all(np.isfinite(v) for v in a["summary"].values())
