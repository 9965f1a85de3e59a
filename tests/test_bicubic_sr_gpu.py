"""MODEL.SR="bicubic" on the device: csbsr_aa_bicubic_up against the fp64 restatement (tests/bicubic_cases.py) through the C ABI, the model
against the REFERENCE's bicubic fixture (tests/golden/bicubic_pspnet*.npz), bit-equality with the joint model's detector half fed the same
up-scaled image, two steps of do_train with an exact resume, and one evaluate_dataset / predict_dataset pass."""
import os

import numpy as np
import pytest
import torch

import bicubic_cases as BC
import eval_io_cases as EC
import predict_cases as PC
from golden_utils import load_golden, max_rel_to_scale, fill_style

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256


def _ptr(t):
    import ctypes as C
    return C.c_void_p(t.data_ptr())


def _up(x, scale, antialias, clip, out=None):
    from csbsr_amd import _lib as L
    planes, H, W = x.shape
    y = torch.empty(planes, H * scale, W * scale, dtype=torch.float32, device=x.device) if out is None else out
    with torch.cuda.device(x.device):
        L.call("csbsr_aa_bicubic_up", _ptr(x), _ptr(y), planes, H, W, scale, int(antialias), int(clip), L.stream(x.device))
    return y


def _bicubic_cfg(detector="PSPNet", scale=4):
    from csbsr_amd.config import cfg as base_cfg
    cfg = base_cfg.clone()
    cfg.MODEL.SR, cfg.MODEL.DETECTOR_TYPE, cfg.MODEL.SCALE_FACTOR = "bicubic", detector, scale
    return cfg


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("antialias", [1, 0])
@pytest.mark.parametrize("case", BC.KERNEL_CASES)
def test_kernel_against_the_restatement(case, antialias):
    """1e-5 absolute: 16 products plus the weights' rounding, <= 32 roundings x 2^-24 x (sum|w| = 1.25^2) x (max|x| = 1.2) = 3.6e-6, times 3.
    Guard bands round the output, two runs bit-identical, clip=1 == clamp(clip=0) bit for bit."""
    planes, H, W, s = case
    x = torch.from_numpy(BC.case_input(*case)).to(DEV)
    want = BC.case_reference(planes, H, W, s, antialias)
    nb = planes * H * s * W * s * 4
    outs = {}
    for clip in (0, 1):
        whole = torch.full((GUARD + nb + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        y = whole[GUARD:GUARD + nb].view(torch.float32).view(planes, H * s, W * s)
        _up(x, s, antialias, clip, out=y)
        again = _up(x, s, antialias, clip)
        torch.cuda.synchronize()
        assert bool((whole[:GUARD] == 0xA5).all()) and bool((whole[-GUARD:] == 0xA5).all())
        assert torch.equal(y.view(torch.int32), again.view(torch.int32))
        ref = np.clip(want, 0.0, 1.0) if clip else want
        err = float(np.abs(y.cpu().double().numpy() - ref).max())
        print(f"{case} antialias={antialias} clip={clip}: max |diff| {err:.2e}")
        assert err <= 1e-5
        outs[clip] = y.clone()
    assert float(outs[0].min()) < 0 and float(outs[0].max()) > 1          # the clip bites
    assert torch.equal(outs[1].view(torch.int32), outs[0].clamp(0, 1).view(torch.int32))


def test_kernel_refuses_what_it_does_not_build():
    from csbsr_amd import _lib as L
    x = torch.zeros(1, 4, 4, device=DEV)
    with pytest.raises(L.CsbsrHipError):
        _up(x, 2, 1, 0)                                                   # a scale that is no multiple of 4
    with pytest.raises(L.CsbsrHipError):
        _up(x, 4, 1, 0, out=torch.zeros(1 + 256, device=DEV)[1:].view(1, 16, 16))      # an output off the 16-byte grid


# ------------------------------------------------------------------------------------------------------------------ the reference
def _fixture_inputs(g):
    """x and the blur kernel are stored; the mask (exact integer arithmetic on seeded draws) and the HR target (unused by this model) are
    regenerated: the first sample of wc_pspnet_it40000's batch."""
    from csbsr_amd.data.synthetic import make_batch
    B = int(g["B"])
    _, hr, mask, k = (t[:B].contiguous() for t in make_batch(2, int(g["lr"]), scale=int(g["scale"]), ksize=21, seed=int(g["seed"])))
    assert float(mask.double().sum()) == float(g["mask_sum"]) and np.allclose(k.numpy(), g["kernel"], atol=1e-7)
    return torch.from_numpy(g["x"]), hr, mask, torch.from_numpy(g["kernel"])


def test_parity_with_the_reference_fixture():
    """The bounds of test_detector_on_reference_sr[split]: sr_preds 1e-5 absolute, map / loss / BatchNorm buffers < 1e-3, every detector
    gradient tensor 3e-2 by the sampled-element method; sr_loss is None, kernel_preds all zeros; JointModel in eval mode (contractive
    fill): map < 1e-3, clipped sr_preds 1e-5."""
    from csbsr_amd.modeling.build_model import JointModelWithLoss, JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    from test_wc_parity_gpu import _grad_errors, _assert_grads
    g = BC.fixture()
    x, hr, mask, k = _fixture_inputs(g)
    m = JointModelWithLoss(_bicubic_cfg(), 1000, 0, None)
    deterministic_fill(m.state_dict(), fill_style(g))
    m.ss_loss_fn.alpha = float(g["alpha"])
    m.detector_precision = "split"
    m.train()
    m.dropout_masks = {}                                                  # the fixture ran without dropout
    seg_l, sr_l, seg, sr, kp = m(int(g["it"]), x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
    assert sr_l is None and kp.shape == k.shape and float(kp.abs().max()) == 0.0
    from csbsr_amd.trainer import calc_loss
    calc_loss(seg_l, sr_l, int(g["it"]), m.cfg).backward()
    torch.cuda.synchronize()
    e_sr = float((sr.cpu() - torch.from_numpy(g["sr_preds"])).abs().max())
    e_seg = max_rel_to_scale(seg.cpu(), g["segment_preds"])
    e_segl = max_rel_to_scale(seg_l.detach().cpu(), g["segment_loss"])
    sd = m.state_dict()
    e_bn = max(max_rel_to_scale(sd[kk[4:]].cpu(), v) for kk, v in g.items() if kk.startswith("buf."))
    print(f"bicubic_pspnet [split]: sr_preds {e_sr:.2e} (abs) seg {e_seg:.2e} seg_loss {e_segl:.2e} BN buffers {e_bn:.2e}")
    assert e_sr <= 1e-5
    assert e_seg < 1e-3 and e_segl < 1e-3 and e_bn < 1e-3, (e_seg, e_segl, e_bn)
    grads = {kk: v.grad for kk, v in m._named_full() if isinstance(v, torch.nn.Parameter)}
    errs = _grad_errors(g, grads, "segmentation_model")
    assert len(errs) > 100
    _assert_grads(errs, 3e-2, "bicubic_pspnet detector gradients [split]")
    assert m.last_dsr is None and m.last_dkvec is None
    del m, grads
    # eval mode: the contractive fill (why: tests/golden/make_bicubic_golden.py -- under the random fill the reference's own eval-mode map
    # is saturated and moves by 3.1e-2 for 1e-4 on the input; recorded as eval_cond_*)
    assert float(g["eval_cond_contractive_0.0001"]) < 1e-3 < float(g["eval_cond_random_0.0001"])
    ev = JointModel(_bicubic_cfg())
    deterministic_fill(ev.state_dict(), str(g["eval_fill"]))
    ev.detector_precision = "split"
    ev.eval()
    e_sr32, e_seg32, e_k = ev(x, torch.zeros(x.shape[0], 1, 21, 21), sr_targets=hr)
    assert tuple(e_k.shape) == tuple(g["eval_kernel_preds_shape"]) and float(e_k.abs().max()) == 0.0
    assert bool(g["eval_sr_is_clamped_sr"])
    e1 = float((e_sr32.cpu() - torch.from_numpy(g["sr_preds"]).clamp(0, 1)).abs().max())
    e2 = max_rel_to_scale(e_seg32.cpu(), g["eval_segment_preds"])
    print(f"bicubic_pspnet eval: clipped sr_preds {e1:.2e} (abs) seg {e2:.2e}")
    assert e1 <= 1e-5 and e2 < 1e-3 and float(e_sr32.min()) >= 0 and float(e_sr32.max()) <= 1


# ------------------------------------------------------------------------------------------------------------------ inside this build
@pytest.mark.parametrize("case", ["wc_pspnet_it40000", "wc_hrnet_ocr_it40000"])
def test_equals_the_joint_models_detector_half(case):
    """The same kernels on the same bytes: map, segmentation loss, BatchNorm buffers and every detector gradient of the bicubic model are
    BIT-identical to the KBPN model's ``forward_from_sr`` fed csbsr_aa_bicubic_up(x), backward of the segmentation mean only."""
    from test_wc_parity_gpu import _inputs, _model
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    g = load_golden(case)
    x, hr, mask, k = _inputs(g)
    B, _, h, w = x.shape
    s, it = int(g["scale"]), int(g["it"])
    up = _up(x.to(DEV).reshape(B * 3, h, w).contiguous(), s, 1, 0).view(B, 3, h * s, w * s)

    joint = _model(g, "split")
    seg_l, _, seg, _, _ = joint.forward_from_sr(it, up, torch.from_numpy(g["kernel_preds"]).reshape(B, -1), x, hr, mask, k)
    seg_l.mean().backward()
    torch.cuda.synchronize()
    want = {"seg": seg.clone(), "seg_l": seg_l.detach().clone()}
    want_sd = {n: t.clone() for n, t in joint.state_dict().items() if n.startswith("segmentation_model.")}
    want_g = {n: (None if v.grad is None else v.grad.clone()) for n, v in joint._named_full() if n.startswith("segmentation_model.")
              and isinstance(v, torch.nn.Parameter)}
    assert joint.last_dsr is not None
    del joint

    m = JointModelWithLoss(_bicubic_cfg(str(g["detector"]), s), 1000, 0, None)
    deterministic_fill(m.state_dict(), fill_style(g))
    m.ss_loss_fn.alpha = float(g["alpha"])
    m.detector_precision = "split"
    m.train()
    m.dropout_masks = {kk.split(".", 1)[1]: torch.from_numpy(v) for kk, v in g.items() if kk.startswith("dropmask.")}
    seg_l2, sr_l2, seg2, sr2, kp2 = m(it, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
    assert sr_l2 is None and float(kp2.abs().max()) == 0.0
    seg_l2.mean().backward()
    torch.cuda.synchronize()
    assert torch.equal(sr2, up) and torch.equal(seg2, want["seg"]) and torch.equal(seg_l2.detach(), want["seg_l"])
    sd = m.state_dict()
    assert list(sd.keys()) == list(want_sd.keys())
    for n, t in sd.items():
        assert torch.equal(t, want_sd[n]), n
    n_grad = 0
    for n, v in m._named_full():
        if isinstance(v, torch.nn.Parameter):
            a, b = v.grad, want_g[n]
            assert (a is None) == (b is None), n
            if a is not None:
                assert torch.equal(a, b), n
                n_grad += 1
    assert n_grad > 100 and m.last_dsr is None and m.last_dkvec is None


# ------------------------------------------------------------------------------------------------------------------ the trainer
def test_two_steps_of_do_train_and_an_exact_resume(tmp_path):
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    from test_trainer_gpu import _pool
    cfg = _bicubic_cfg()
    cfg.SOLVER.BATCH_SIZE = 2
    ds = _pool()
    loader = lambda n, seed: DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=n, seed=seed, drop_last=True)
    it0 = 40000

    def build(resume_iter):
        m = JointModelWithLoss(cfg, 5, resume_iter, None, device=DEV)
        deterministic_fill(m.state_dict(), "contractive")
        return m, T.build_optimizer(cfg, m)

    def run(model, opt, ld, resume_iter, out=None):
        logs = []
        T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt, resume_iter), ld, resume_iter=resume_iter, log_step=1, save_step=1,
                   output_dir=out, log=logs.append)
        return [(r["iteration"], r["segment_loss"], r["sr_loss"], r["boundary_alpha"]) for r in logs if "segment_loss" in r]
    torch.manual_seed(5)
    full, opt_full = build(it0)
    logs_full = run(full, opt_full, loader(2, 31), it0)
    assert [r[0] for r in logs_full] == [40001, 40002]
    assert all(np.isfinite(r[1]) and r[1] > 0 and r[2] == 0.0 for r in logs_full)
    assert sum(p.grad is not None for p in full.parameters()) > 100 and full.last_dsr is None

    torch.manual_seed(5)
    first, opt_first = build(it0)
    logs_a = run(first, opt_first, loader(1, 31), it0, str(tmp_path))
    for kind in ("model", "optimizer", "trainer"):
        assert (tmp_path / kind / "iteration_40001.pth").is_file()
    assert not any(k.startswith("sr_model") for k in torch.load(tmp_path / "model" / "iteration_40001.pth", map_location="cpu"))
    del first, opt_first
    torch.manual_seed(777)
    torch.rand(3, device=DEV)
    second, opt_second = build(0)
    ld = loader(2, 999)
    it = T.resume(cfg, str(tmp_path), 40001, second, opt_second, ld)
    assert it == 40001
    logs_b = run(second, opt_second, ld, it)
    assert logs_a + logs_b == logs_full
    sd, sd_full = second.state_dict(), full.state_dict()
    for name, t in sd.items():
        assert torch.equal(t, sd_full[name]), name
    for p, q in zip(opt_second.param_groups[0]["params"], opt_full.param_groups[0]["params"]):
        for key, v in opt_second.state[p].items():
            assert torch.equal(v.cpu(), opt_full.state[q][key].cpu()), key

    view = ds.subset([3, 1, 4, 0, 2])
    res = T.validate(second, DeviceTrainLoader(view, 64, 4, batch_size=2, seed=3, shuffle=False), 40002, seed=7)
    assert set(res) == {"eval_segment_loss", "eval_sr_loss", "psnr", "ssim", "kernel_psnr", "iou", "batches", "images"}
    assert res["eval_sr_loss"] == 0.0 and (res["batches"], res["images"]) == (3, 5)
    assert all(np.isfinite(v) for v in res.values()) and res["psnr"] > 5 and 0 <= res["iou"] <= 1


# ------------------------------------------------------------------------------------------------------------------ inference
def _eval_model():
    from csbsr_amd.modeling.build_model import JointModel
    from csbsr_amd.utils.detfill import deterministic_fill
    m = JointModel(_bicubic_cfg())
    deterministic_fill(m.state_dict())
    m.eval()
    return m


def _zero_kernel_psnr(kernel_targets):
    k = kernel_targets.detach().cpu().double().numpy().reshape(-1, kernel_targets.shape[-2] * kernel_targets.shape[-1])
    return 10.0 * np.log10(1.0 / (k ** 2).mean(1))


def test_evaluate_dataset_with_the_bicubic_model(tmp_path):
    from PIL import Image
    from csbsr_amd.data.resident_test import DeviceTestLoader, ResidentTestSet
    from csbsr_amd.inference import evaluate_dataset
    m = _eval_model()
    hr, masks, lr, kernels, names = EC.make_testset(7, 3, 128, 128, 4)
    mk = lambda: DeviceTestLoader(ResidentTestSet(hr, masks, lr, kernels, names, device=DEV), 64, 4, 2)
    out = evaluate_dataset(m, mk(), save_dir=str(tmp_path))
    for k, shape in (("psnr", (3,)), ("ssim", (3,)), ("kernel_psnr", (12,)), ("iou", (3, 99))):
        assert out[k].shape == shape and out[k].dtype == np.float32 and np.isfinite(out[k]).all(), k
    assert all(np.isfinite(v) for v in out["summary"].values())
    want = np.concatenate([_zero_kernel_psnr(b[3]) for b in mk()])
    assert want.shape == (12,) and np.allclose(out["kernel_psnr"], want, rtol=1e-5, atol=0)
    # the saved SR image is the clipped restatement of the LR image (patches of 16 x 16 LR: restated per patch), to one level
    sr = np.zeros((128, 128, 3))
    x = lr[0].astype(np.float32) / np.float32(255)
    for py in range(2):
        for px in range(2):
            t = BC.bicubic_up_ref(x[16 * py:16 * py + 16, 16 * px:16 * px + 16].transpose(2, 0, 1), 4, True, clip=True)
            sr[64 * py:64 * py + 64, 64 * px:64 * px + 64] = t.transpose(1, 2, 0)
    got = np.array(Image.open(tmp_path / "images" / out["fnames"][0])).astype(np.int64)
    assert np.abs(got - np.floor(sr * 255.0)).max() <= 1
    kfiles = sorted(os.listdir(tmp_path / "kernels"))
    assert len(kfiles) == 12 and all(np.array(Image.open(tmp_path / "kernels" / f)).max() == 0 for f in kfiles)      # black


def test_predict_dataset_with_the_bicubic_model():
    from csbsr_amd.data.resident_predict import DevicePredictLoader, ResidentImageSet
    from csbsr_amd.inference import predict_dataset
    m = _eval_model()
    images = PC.make_images([(40, 24), (16, 16)], seed=23)
    ld = DevicePredictLoader(ResidentImageSet(images, ["field_0.png", "field_1.png"], device=DEV), 16, 4, halo=8, batch_patches=4)

    def restated(win, dummy):          # the clipped restatement on the tiles; the map and the kernels are not compared through it
        sr = torch.from_numpy(BC.bicubic_up_ref(win.numpy(), 4, True, clip=True).astype(np.float32))
        return sr, torch.zeros(sr.shape[0], 1, *sr.shape[2:]), torch.zeros_like(dummy)
    want = PC.host_chain(ld, images, restated, torch.from_numpy, EC.thresholds32()[EC.SAVE_IDX])
    got = list(predict_dataset(m, ld))
    assert [g["name"] for g in got] == ["field_0.png", "field_1.png"]
    for g, w, (h, w_) in zip(got, want, ((40, 24), (16, 16))):
        assert g["sr_u8"].dtype == torch.uint8 and g["map_u8"].dtype == torch.uint8 and g["map_f32"].dtype == torch.float32
        assert tuple(g["sr_u8"].shape) == (4 * h, 4 * w_, 3) and tuple(g["map_f32"].shape) == (4 * h, 4 * w_) == tuple(g["map_u8"].shape)
        assert g["kernels"].dtype == torch.float32 and g["kernels"].shape[1:] == (1, 21, 21) and float(g["kernels"].abs().max()) == 0.0
        assert torch.isfinite(g["map_f32"]).all() and g["sr_u8"].float().std() > 1
        assert np.abs(g["sr_u8"].cpu().numpy().astype(np.int64) - w["sr_u8"].astype(np.int64)).max() <= 1
    assert [g["kernels"].shape[0] for g in got] == [6, 1]
