"""csbsr_pr_sweep (csrc/pr_sweep.hip) and its drivers on the device: every count is an integer and is asked for exactly, against the NumPy
restatement of tests/pr_sweep_cases.py (held equal to the per-threshold SciPy form by tests/test_pr_sweep_cpu.py).

Through the C ABI every input sits inside an allocation filled with +inf (pred) / 1 (mask) -- a read outside the image would add counts --
and every output inside a sentinel-filled allocation whose margins are checked; every call runs twice and the results must be identical."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pr_sweep_cases as PC

pytestmark = pytest.mark.gpu

PAD = 64
ISENT = 0x5A5A5A5A
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


def _out(n):
    buf = torch.full((n + 2 * PAD,), ISENT, dtype=torch.int32, device=DEV)
    return buf, buf[PAD:PAD + n]


def device_counts(pred, mask, thresholds, tol2):
    """int64 [N, 4, T] of csbsr_pr_sweep through the C ABI, called twice"""
    from csbsr_amd import _lib as L
    L.load()
    N, H, W = pred.shape
    T = len(thresholds)
    (_, p), (_, m) = _inp(pred, float("inf")), _inp(mask, 1.0)
    th = torch.from_numpy(PC.th32(thresholds)).to(DEV)
    runs = []
    for _ in range(2):
        hwhole, hist = _out(N * 3 * (T + 1))
        hist.zero_()
        cwhole, counts = _out(N * 4 * T)
        L.call("csbsr_pr_sweep", _ptr(p), _ptr(m), _ptr(th), N, H, W, T, tol2, _ptr(hist), _ptr(counts), _stream())
        torch.cuda.synchronize()
        for whole in (hwhole, cwhole):
            assert bool((whole[:PAD] == ISENT).all()) and bool((whole[-PAD:] == ISENT).all()), "a write outside the output"
        runs.append(counts.cpu().numpy().reshape(N, 4, T).astype(np.int64))
    assert np.array_equal(runs[0], runs[1]), "two calls on the same inputs differ"
    return runs[0]


@pytest.mark.parametrize("name", sorted(PC.cases()))
def test_counts_equal_the_restatement(name):
    pred, mask, th, tol2 = PC.cases()[name]
    got, want = device_counts(pred, mask, th, tol2), PC.counts_histogram(pred, mask, th, tol2)
    assert np.array_equal(got, want), (np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])


def test_realistic_size_against_the_per_threshold_form():
    pred, mask, th, tol2 = PC.realistic()
    assert tol2 == 4 and pred.shape == (2, 448, 448) and len(th) == 99
    assert np.array_equal(device_counts(pred, mask, th, tol2), PC.realistic_reference())


def test_python_surface():
    from csbsr_amd.utils.estimate_metrics import pr_sweep
    pred, mask, th, _ = PC.cases()["batch3"]
    p, m = torch.from_numpy(pred).to(DEV)[:, None], torch.from_numpy(mask).to(DEV)[:, None]
    for tolerance, tol2 in ((0, 0), (2.0, 4), (2.24, 5), (16, 256)):
        out = pr_sweep(p, m, th, tolerance)
        assert out.is_cuda and out.dtype == torch.int32 and tuple(out.shape) == (3, 4, 99)
        assert np.array_equal(out.cpu().numpy(), PC.counts_histogram(pred, mask, th, tol2)), tolerance
    assert torch.equal(pr_sweep(p, m, th), pr_sweep(p, m, th, 2.0))
    with pytest.raises(ValueError):
        pr_sweep(p, m, th, 16.5)


def test_bad_arguments_are_refused():
    from csbsr_amd import _lib as L
    L.load()
    p, m = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    th = torch.from_numpy(PC.th32(PC.TH255 + [0.999])).to(DEV)
    hist, counts = torch.zeros(3 * 257, dtype=torch.int32, device=DEV), torch.zeros(4 * 256, dtype=torch.int32, device=DEV)
    good = dict(N=1, H=8, W=8, T=99, tol2=4)
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(H=8193), dict(W=8193), dict(T=0), dict(T=256), dict(tol2=-1), dict(tol2=257)):
        a = {**good, **bad}
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_pr_sweep", _ptr(p), _ptr(m), _ptr(th), a["N"], a["H"], a["W"], a["T"], a["tol2"], _ptr(hist), _ptr(counts), _stream())
    for null in range(5):
        ptrs = [_ptr(p), _ptr(m), _ptr(th), _ptr(hist), _ptr(counts)]
        ptrs[null] = None
        with pytest.raises(L.CsbsrHipError):
            L.call("csbsr_pr_sweep", *ptrs[:3], 1, 8, 8, 99, 4, *ptrs[3:], _stream())


@pytest.mark.parametrize("name", ["37x70_tol2_0", "33x129_tol2_0", "batch3"])
def test_tolerance_zero_against_the_iou_sweep(name):
    """inter = tp, union = n_pred + n_gt - tp: the ``inter`` / ``uni`` outputs of csbsr_iou_sweep are integers below 2^24, exact in fp32"""
    from csbsr_amd import _lib as L
    pred, mask, th, _ = PC.cases()[name]
    N, H, W = pred.shape
    T = len(th)
    c = device_counts(pred, mask, th, 0)
    p, m = torch.from_numpy(pred).to(DEV).contiguous(), torch.from_numpy(mask).to(DEV).contiguous()
    t = torch.from_numpy(PC.th32(th)).to(DEV)
    hist = torch.zeros(N, 2, T + 1, dtype=torch.int32, device=DEV)
    iou, inter, uni = (torch.empty(N, T, dtype=torch.float32, device=DEV) for _ in range(3))
    L.call("csbsr_iou_sweep", _ptr(p), _ptr(m), _ptr(t), N, H * W, T, 1e-5, _ptr(hist), _ptr(iou), _ptr(inter), _ptr(uni), _stream())
    inter, uni = inter.cpu().numpy().astype(np.int64), uni.cpu().numpy().astype(np.int64)
    assert np.array_equal(c[:, 1], inter) and np.array_equal(c[:, 2], inter)
    assert np.array_equal(c[:, 0] + c[:, 3] - c[:, 1], uni) and inter.max() > 0


def test_tolerance_zero_against_the_classification_counts():
    from csbsr_amd.inference import CLASSIFICATION_IDX, classification_counts
    pred, mask, th, _ = PC.cases()["33x129_tol2_0"]
    hard = (mask > 0.5).astype(np.float32)                                  # a {0, 1} mask: both predicates agree on it
    c = device_counts(pred, hard, th, 0)
    p, m = torch.from_numpy(pred).to(DEV)[:, None], torch.from_numpy(hard).to(DEV)[:, None]
    t49 = torch.from_numpy(PC.th32(th))[CLASSIFICATION_IDX].to(DEV)
    tp, tn, ng, nn = classification_counts(p, m, t49).cpu().numpy()[0]
    j = CLASSIFICATION_IDX
    assert (c[0, 1, j], c[0, 3, j]) == (tp, ng) and c[0, 0, j] - c[0, 1, j] == nn - tn and tp > 0


# ------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope="module")
def stub_set():
    import eval_io_cases as EC
    hr, masks, lr, kernels, names = EC.make_testset(11, 5, 64, 96, 4, zero_mask=3)
    items = [EC.reference_item_numpy(hr[i], masks[i], lr[i], kernels[i], (32, 48), 4, 2) for i in range(5)]
    return dict(hr=hr, masks=masks, lr=lr, kernels=kernels, names=names, items=items)


def _loader(d):
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    return DeviceTestLoader(ResidentTestSet(d["hr"], d["masks"], d["lr"], d["kernels"], d["names"], device=DEV), (32, 48), 4, 2)


def test_evaluate_dataset_with_pr_tolerance(stub_set, tmp_path):
    import eval_io_cases as EC
    from csbsr_amd.inference import THRESHOLDS, evaluate_batch, evaluate_dataset, pr_scores, summarize_pr
    d = stub_set
    out = evaluate_dataset(EC.stub_model, _loader(d), pr_tolerance=2, save_dir=str(tmp_path / "pr"))
    plain = evaluate_dataset(EC.stub_model, _loader(d), save_dir=str(tmp_path / "plain"))
    # the stub's own maps, on the CPU (bit-identical to the device's: tests/test_eval_io_gpu.py)
    chains = [EC.cpu_chain(d["items"][i0:i0 + 2], len(d["items"][i0:i0 + 2])) for i0 in (0, 2, 4)]
    seg = torch.cat([c["seg"] for c in chains])[:, 0].numpy()
    masks = np.stack([it[2][0] for it in d["items"]])
    want = PC.counts_histogram(seg, masks, THRESHOLDS, 4)
    assert out["pr_counts"].dtype == np.int64 and out["pr_counts"].shape == (5, 4, 99) and np.array_equal(out["pr_counts"], want)
    assert (want[3, 3] == 0).all() and (want[[0, 1, 2, 4], 3] > 0).all() and (want[:, 1] < want[:, 0]).any() and (want[:, 2] > 0).any()
    pr_keys = ["ODS", "ODS_threshold", "OIS", "AP", "P_at_ODS", "R_at_ODS"]
    assert {k: out["summary"][k] for k in pr_keys} == summarize_pr(want, THRESHOLDS)
    assert 0 < out["summary"]["ODS"] <= 1 and 0 < out["summary"]["AP"] <= 1
    fn, th, p, r, f = PC.read_pr_log(str(tmp_path / "pr" / "pr_log.csv"))
    assert fn == out["fnames"] and th == THRESHOLDS and all(np.array_equal(a, b) for a, b in zip((p, r, f), pr_scores(want)))
    # without the option: the parent commit's keys and files, and the same bits
    assert set(plain) == {"fnames", "psnr", "ssim", "kernel_psnr", "iou", "summary"}
    assert set(plain["summary"]) == {"PSNR_mean", "SSIM_mean", "PSNR(Kernel)_mean", "AIU_mean", "IoU_max"}
    assert set(out) == set(plain) | {"pr_counts"} and set(out["summary"]) == set(plain["summary"]) | set(pr_keys)
    for k in ("psnr", "ssim", "kernel_psnr", "iou"):
        assert out[k].tobytes() == plain[k].tobytes(), k
    assert sorted(os.listdir(tmp_path / "plain")) == ["images", "iou_log.csv", "kernels", "kernels_origin", "masks"]
    assert sorted(os.listdir(tmp_path / "pr")) == ["images", "iou_log.csv", "kernels", "kernels_origin", "masks", "pr_log.csv"]
    assert open(tmp_path / "pr" / "iou_log.csv").read() == open(tmp_path / "plain" / "iou_log.csv").read()
    # evaluate_batch, batch by batch
    rows = [evaluate_batch(EC.stub_model, imgs, s1, s2, sr_t, m, kt, ksize=21, pr_tolerance=2)["pr_counts"]
            for imgs, sr_t, m, kt, _, s1, s2 in _loader(d)]
    assert np.array_equal(np.concatenate(rows), want) and rows[0].dtype == np.int64
    imgs, sr_t, m, kt, _, s1, s2 = next(iter(_loader(d)))
    assert set(evaluate_batch(EC.stub_model, imgs, s1, s2, sr_t, m, kt, ksize=21)) == {"sr_preds", "segment_preds", "kernel_preds", "psnr",
                                                                                     "ssim", "kernel_psnr", "iou"}
