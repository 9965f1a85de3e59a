"""csrc/skeleton.hip and its drivers on the device: every result is an integer and is asked for exactly, against the NumPy restatement of
tests/skeleton_cases.py (whose own properties tests/test_skeleton_cpu.py holds).

Through the C ABI every input sits inside an allocation filled with +inf (prediction planes) / 1 (masks) -- a read outside the image would
set pixels -- and every output and work plane inside a sentinel-filled allocation whose margins are checked; every call sequence runs
twice and the results must be identical."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import skeleton_cases as SC

pytestmark = pytest.mark.gpu

PAD = 64
ISENT, BSENT = 0x5A5A5A5A, 0x5A
DEV = torch.device("cuda", 0)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _inp(x, fill):
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).reshape(-1)
    buf = torch.full((x.numel() + 2 * PAD,), fill, dtype=torch.float32, device=DEV)
    buf[PAD:PAD + x.numel()] = x.to(DEV)
    return buf, buf[PAD:PAD + x.numel()]


def _out(n, dtype=torch.int32):
    buf = torch.full((n + 2 * PAD,), ISENT if dtype == torch.int32 else BSENT, dtype=dtype, device=DEV)
    return buf, buf[PAD:PAD + n]


def _margins_intact(*wholes):
    for w in wholes:
        sent = ISENT if w.dtype == torch.int32 else BSENT
        assert bool((w[:PAD] == sent).all()) and bool((w[-PAD:] == sent).all()), "a write outside an output"


def device_skeleton(planes, threshold, max_passes=0, fill=float("inf")):
    """(uint8 [N, H, W], launch groups) of init / passes / finish through the C ABI with the host loop of ``skeletonize``, run twice"""
    from csbsr_amd import _lib as L
    lib = L.load()
    K = int(lib.csbsr_skeleton_max_passes())
    assert K == SC.K
    N, H, W = planes.shape
    WW = (W + SC.WORD - 1) // SC.WORD
    _, x = _inp(planes, fill)
    runs = []
    for _ in range(2):
        (wa, a), (wb, b), (wc, cnt), (wo, out) = _out(N * H * WW), _out(N * H * WW), _out(1), _out(N * H * W, torch.uint8)
        cnt.zero_()
        L.call("csbsr_skeleton_init", _ptr(x), threshold, N, H, W, _ptr(a), _stream())
        done = total = groups = 0
        while max_passes == 0 or done < max_passes:
            p = K if max_passes == 0 else min(K, max_passes - done)
            L.call("csbsr_skeleton_passes", _ptr(a), _ptr(b), N, H, W, p, _ptr(cnt), _stream())
            a, b = b, a
            done, groups = done + p, groups + 1
            now = int(cnt.item())
            if now == total:
                break
            total = now
        L.call("csbsr_skeleton_finish", _ptr(a), N, H, W, _ptr(out), _stream())
        torch.cuda.synchronize()
        _margins_intact(wa, wb, wc, wo)
        s = out.cpu().numpy().reshape(N, H, W)
        assert total == int(SC.binarise(planes, threshold).sum()) - int(s.sum()), "every deleted pixel is counted exactly once"
        runs.append((s, groups))
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1], "two runs on the same input differ"
    return runs[0]


@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_skeleton_equals_the_restatement(name):
    planes = SC.cases()[name]
    got, groups = device_skeleton(planes, 0.5)
    want = SC.expected(name)
    assert got.dtype == np.uint8 and got.max() <= 1 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    passes = max(SC.skeleton(p > 0.5, return_passes=True)[1] for p in planes)
    assert groups <= -(-passes // SC.K) + 1                                         # at most one launch beyond the converging one
    if name in ("ones_33x129", "corner_blob", "batch4"):
        assert groups >= 3


@pytest.mark.parametrize("name", ["cracks", "batch4"])
def test_masks_with_ones_around_them(name):
    got, _ = device_skeleton(SC.cases()[name], 0.5, fill=1.0)
    assert np.array_equal(got, SC.expected(name))


@pytest.mark.parametrize("max_passes", [0, 1, 2, 3, SC.K - 1, SC.K, SC.K + 1, 2 * SC.K + 3])
def test_skeletonize_at_a_number_of_passes(max_passes):
    """a ``max_passes`` that is no multiple of the passes of a launch: the last group is shorter"""
    from csbsr_amd.utils.estimate_metrics import skeletonize
    for name in ("corner_blob", "batch4"):
        x = torch.from_numpy(SC.cases()[name]).to(DEV)
        out = skeletonize(x, max_passes=max_passes)
        assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == tuple(x.shape)
        want = SC.expected(name, max_passes)
        assert np.array_equal(out.cpu().numpy(), want), (name, np.argwhere(out.cpu().numpy() != want)[:5])
        got_abi, _ = device_skeleton(SC.cases()[name], 0.5, max_passes)
        assert np.array_equal(got_abi, want)
    assert not np.array_equal(SC.expected("corner_blob", SC.K + 1), SC.expected("corner_blob", SC.K))         # the extra pass matters
    assert not np.array_equal(SC.expected("corner_blob", SC.K + 1), SC.expected("corner_blob", 2 * SC.K))


def test_skeletonize_surface():
    from csbsr_amd.utils.estimate_metrics import skeletonize
    pred, mask, t = SC.pair()
    assert np.isnan(pred).any() and np.isinf(pred).any()
    want = SC.skeleton_of(pred, t)
    p = torch.from_numpy(pred).to(DEV)
    assert np.array_equal(skeletonize(p, t).cpu().numpy(), want)                    # NaN is not predicted
    assert np.array_equal(skeletonize(p[:, None], t).cpu().numpy(), want)           # [B, 1, H, W] -> [B, H, W]
    assert np.array_equal(skeletonize(torch.from_numpy(pred), np.float32(t)).cpu().numpy(), SC.skeleton_of(pred, np.float32(t)))
    assert np.array_equal(skeletonize(torch.from_numpy(mask).to(DEV)).cpu().numpy(), SC.skeleton_of(mask, 0.5))       # mask > 0.5
    got_abi, _ = device_skeleton(pred, t)
    assert np.array_equal(got_abi, want)
    with pytest.raises(ValueError):
        skeletonize(p, max_passes=-1)
    with pytest.raises(ValueError):
        skeletonize(p, threshold=float("nan"))


def device_centerline_counts(sp, pred, t, sl, mask):
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = pred.shape
    (_, p), (_, m) = _inp(pred, float("inf")), _inp(mask, 1.0)
    skels = []
    for s in (sp, sl):
        whole = torch.full((s.size + 2 * PAD,), 1, dtype=torch.uint8, device=DEV)   # ones around the skeletons
        whole[PAD:PAD + s.size] = torch.from_numpy(np.ascontiguousarray(s, np.uint8)).reshape(-1).to(DEV)
        skels.append((whole, whole[PAD:PAD + s.size]))
    runs = []
    for _ in range(2):
        whole, counts = _out(N * 4)
        L.call("csbsr_centerline_counts", _ptr(skels[0][1]), _ptr(p), t, _ptr(skels[1][1]), _ptr(m), N, H, W, _ptr(counts), _stream())
        torch.cuda.synchronize()
        _margins_intact(whole)
        runs.append(counts.cpu().numpy().reshape(N, 4).astype(np.int64))
    assert np.array_equal(runs[0], runs[1])
    return runs[0]


def test_centerline_counts():
    from csbsr_amd.utils.estimate_metrics import centerline_counts
    pred, mask, t = SC.pair()
    want = SC.counts(pred, mask, t)
    got = device_centerline_counts(SC.skeleton_of(pred, t), pred, t, SC.skeleton_of(mask, 0.5), mask)
    assert np.array_equal(got, want), (got, want)
    p, m = torch.from_numpy(pred).to(DEV)[:, None], torch.from_numpy(mask).to(DEV)[:, None]
    out = centerline_counts(p, m, t)
    assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (3, 4) and np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(out, centerline_counts(p, m, t))
    one = np.ones((1, 1, 1), np.float32)                                            # one pixel, every combination
    for pv, mv, w in ((1, 1, [1, 1, 1, 1]), (1, 0, [1, 0, 0, 0]), (0, 1, [0, 0, 1, 0]), (0, 0, [0, 0, 0, 0])):
        c = device_centerline_counts((one * pv).astype(np.uint8), one * pv, 0.5, (one * mv).astype(np.uint8), one * mv)
        assert c.tolist() == [w]


def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    L.load()
    x = torch.zeros(64, device=DEV)
    a, b = torch.zeros(64, dtype=torch.int32, device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV)
    cnt, out = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(64, dtype=torch.uint8, device=DEV)
    st = _stream()
    good = dict(N=1, H=8, W=8)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(N=65536)):
        d = {**good, **bad}
        dims = (d["N"], d["H"], d["W"])
        for call in (("csbsr_skeleton_init", _ptr(x), 0.5, *dims, _ptr(a), st), ("csbsr_skeleton_passes", _ptr(a), _ptr(b), *dims, 1, _ptr(cnt), st),
                     ("csbsr_skeleton_finish", _ptr(a), *dims, _ptr(out), st),
                     ("csbsr_centerline_counts", _ptr(out), _ptr(x), 0.5, _ptr(out), _ptr(x), *dims, _ptr(cnt), st)):
            with pytest.raises(L.CsbsrHipError):
                L.call(*call)
    for passes in (0, -1, SC.K + 1):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_skeleton_passes", _ptr(a), _ptr(b), 1, 8, 8, passes, _ptr(cnt), st)
    with pytest.raises(L.CsbsrHipError):                                             # in place
        L.call("csbsr_skeleton_passes", _ptr(a), _ptr(a), 1, 8, 8, 1, _ptr(cnt), st)
    for th in (float("nan"), float("inf")):
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_skeleton_init", _ptr(x), th, 1, 8, 8, _ptr(a), st)
    for call in (("csbsr_skeleton_init", None, 0.5, 1, 8, 8, _ptr(a), st), ("csbsr_skeleton_init", _ptr(x), 0.5, 1, 8, 8, None, st),
                 ("csbsr_skeleton_passes", None, _ptr(b), 1, 8, 8, 1, _ptr(cnt), st), ("csbsr_skeleton_passes", _ptr(a), None, 1, 8, 8, 1, _ptr(cnt), st),
                 ("csbsr_skeleton_passes", _ptr(a), _ptr(b), 1, 8, 8, 1, None, st), ("csbsr_skeleton_finish", None, 1, 8, 8, _ptr(out), st),
                 ("csbsr_skeleton_finish", _ptr(a), 1, 8, 8, None, st),
                 ("csbsr_centerline_counts", _ptr(out), _ptr(x), 0.5, _ptr(out), _ptr(x), 1, 8, 8, None, st),
                 ("csbsr_centerline_counts", None, _ptr(x), 0.5, _ptr(out), _ptr(x), 1, 8, 8, _ptr(cnt), st)):
        with pytest.raises(L.CsbsrHipError):
            L.call(*call)
    torch.cuda.synchronize()
    assert int(cnt.abs().sum()) == 0 and int(out.sum()) == 0                         # nothing ran


# ------------------------------------------------------------------------------------------------ the drivers
@pytest.fixture(scope="module")
def stub_set():
    import eval_io_cases as EC
    hr, masks, lr, kernels, names = EC.make_testset(11, 5, 64, 96, 4, zero_mask=3)
    items = [EC.reference_item_numpy(hr[i], masks[i], lr[i], kernels[i], (32, 48), 4, 2) for i in range(5)]
    return dict(hr=hr, masks=masks, lr=lr, kernels=kernels, names=names, items=items)


def _loader(d):
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    return DeviceTestLoader(ResidentTestSet(d["hr"], d["masks"], d["lr"], d["kernels"], d["names"], device=DEV), (32, 48), 4, 2)


def test_evaluate_dataset_with_cldice_threshold(stub_set, tmp_path):
    import eval_io_cases as EC
    from csbsr_amd.inference import cldice_scores, evaluate_batch, evaluate_dataset, summarize_cldice
    d, t = stub_set, 0.5
    out = evaluate_dataset(EC.stub_model, _loader(d), cldice_threshold=t, save_dir=str(tmp_path / "cl"))
    plain = evaluate_dataset(EC.stub_model, _loader(d), save_dir=str(tmp_path / "plain"))
    # the stub's own maps, on the CPU (bit-identical to the device's: tests/test_eval_io_gpu.py)
    chains = [EC.cpu_chain(d["items"][i0:i0 + 2], len(d["items"][i0:i0 + 2])) for i0 in (0, 2, 4)]
    seg = torch.cat([c["seg"] for c in chains])[:, 0].numpy()
    masks = np.stack([it[2][0] for it in d["items"]])
    want = SC.counts(seg, masks, t)
    assert out["cl_counts"].dtype == np.int64 and out["cl_counts"].shape == (5, 4) and np.array_equal(out["cl_counts"], want), (out["cl_counts"], want)
    assert (want[3, 2:] == 0).all() and (want[[0, 1, 2, 4], 2] > 0).all() and (want[:, 0] > 0).all() and (want[:, 1] < want[:, 0]).any()
    keys = ["clDice", "Tprec", "Tsens", "clDice_pooled"]
    assert {k: out["summary"][k] for k in keys} == summarize_cldice(want) and 0 < out["summary"]["clDice"] < 1
    rows = SC.read_csv(str(tmp_path / "cl" / "cldice_log.csv"))
    assert [r[0] for r in rows[1:]] == out["fnames"] and np.array_equal(np.array([[int(v) for v in r[1:5]] for r in rows[1:]]), want)
    for k, a in enumerate(cldice_scores(want)):
        assert [float(r[5 + k]) for r in rows[1:]] == a.tolist()
    # without the option: the parent commit's keys and files, and the same bits
    assert set(plain) == {"fnames", "psnr", "ssim", "kernel_psnr", "iou", "summary"}
    assert set(plain["summary"]) == {"PSNR_mean", "SSIM_mean", "PSNR(Kernel)_mean", "AIU_mean", "IoU_max"}
    assert set(out) == set(plain) | {"cl_counts"} and set(out["summary"]) == set(plain["summary"]) | set(keys)
    for k in ("psnr", "ssim", "kernel_psnr", "iou"):
        assert out[k].tobytes() == plain[k].tobytes(), k
    assert sorted(os.listdir(tmp_path / "plain")) == ["images", "iou_log.csv", "kernels", "kernels_origin", "masks"]
    assert sorted(os.listdir(tmp_path / "cl")) == ["cldice_log.csv", "images", "iou_log.csv", "kernels", "kernels_origin", "masks"]
    assert open(tmp_path / "cl" / "iou_log.csv").read() == open(tmp_path / "plain" / "iou_log.csv").read()
    # evaluate_batch, batch by batch
    rows = [evaluate_batch(EC.stub_model, imgs, s1, s2, sr_t, m, kt, ksize=21, cldice_threshold=t)["cl_counts"]
            for imgs, sr_t, m, kt, _, s1, s2 in _loader(d)]
    assert np.array_equal(np.concatenate(rows), want) and rows[0].dtype == np.int64
    imgs, sr_t, m, kt, _, s1, s2 = next(iter(_loader(d)))
    assert set(evaluate_batch(EC.stub_model, imgs, s1, s2, sr_t, m, kt, ksize=21)) == {"sr_preds", "segment_preds", "kernel_preds", "psnr",
                                                                                     "ssim", "kernel_psnr", "iou"}
    for bad in (0.0, 1.0, 2, float("nan")):
        with pytest.raises(ValueError):
            evaluate_dataset(lambda *a, **k: pytest.fail("the model ran"), _loader(d), cldice_threshold=bad)


def test_predict_dataset_with_measure_threshold(tmp_path):
    """Two images of 16 x 24 and 21 x 17 LR pixels, patch (8, 8), scale 4: both are several tiles of the loader, and the skeleton is taken on
    the stitched 64 x 96 and 84 x 68 maps."""
    from PIL import Image
    import eval_io_cases as EC
    import predict_cases as PC
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd.inference import predict_dataset
    images = PC.make_images(PC.PREDICT_SIZES[:2], seed=17)
    names = ["field_0.png", "field_1.png"]
    t = 0.4
    for batch_patches in (16, 4):                                                   # one unit for both images; one unit per image
        ld = DevicePredictLoader(ResidentImageSet(images, names, device=DEV), (8, 8), 4, halo=2, batch_patches=batch_patches)
        assert len(list(ld)) == (1 if batch_patches == 16 else 2)
        want = PC.host_chain(ld, images, EC.stub_model, torch.from_numpy, EC.thresholds32()[EC.SAVE_IDX])
        save = tmp_path / str(batch_patches)
        got = list(predict_dataset(EC.stub_model, ld, save_dir=str(save), measure_threshold=t))
        plain = list(predict_dataset(EC.stub_model, ld))
        stats = []
        for g, p, w in zip(got, plain, want):
            assert set(p) == {"name", "sr_u8", "map_u8", "map_f32", "kernels"} and set(g) == set(p) | {"crack_px", "skeleton_px", "mean_width_px"}
            assert np.array_equal(g["map_f32"].cpu().numpy().view(np.uint32), w["map_f32"].view(np.uint32))
            assert torch.equal(g["map_f32"], p["map_f32"]) and torch.equal(g["sr_u8"], p["sr_u8"]) and torch.equal(g["map_u8"], p["map_u8"])
            region = SC.binarise(w["map_f32"], t)
            skel = SC.skeleton(region)
            assert type(g["crack_px"]) is int and type(g["skeleton_px"]) is int and type(g["mean_width_px"]) is float
            assert (g["crack_px"], g["skeleton_px"]) == (int(region.sum()), int(skel.sum())) and 0 < g["skeleton_px"] < g["crack_px"]
            assert g["mean_width_px"] == int(region.sum()) / int(skel.sum())
            im = Image.open(save / "skeletons" / g["name"])
            assert im.mode == "L" and np.array_equal(np.array(im), skel.astype(np.uint8) * 255), g["name"]
            stats.append((g["name"], g["crack_px"], g["skeleton_px"], g["mean_width_px"]))
        assert sorted(os.listdir(save)) == ["crack_stats.csv", "images", "kernels", "kernels_origin", "masks", "skeletons"]
        assert sorted(os.listdir(save / "skeletons")) == names
        rows = SC.read_csv(str(save / "crack_stats.csv"))
        assert rows[0] == ["name", "crack_px", "skeleton_px", "mean_width_px"]
        assert [(r[0], int(r[1]), int(r[2]), float(r[3])) for r in rows[1:]] == stats
    # without the option and with save_dir: today's folders
    for _ in predict_dataset(EC.stub_model, ld, save_dir=str(tmp_path / "plain")):
        pass
    assert sorted(os.listdir(tmp_path / "plain")) == ["images", "kernels", "kernels_origin", "masks"]
    # an empty region: no skeleton, width 0.0
    g = next(predict_dataset(lambda imgs, dummy=None: tuple(torch.zeros_like(v) for v in EC.stub_model(imgs)), ld, measure_threshold=t))
    assert (g["crack_px"], g["skeleton_px"], g["mean_width_px"]) == (0, 0, 0.0)
    with pytest.raises(ValueError):
        next(predict_dataset(EC.stub_model, ld, measure_threshold=1.0))
