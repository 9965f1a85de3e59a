"""SR-only pretraining on the device, at the fixtures' size (LR 16 -> HR 64): SRModelWithLoss against the reference's golden vectors and,
bit for bit, against JointModelWithLoss inside SR_PRETRAIN_ITER; the image-only loader against the loader with masks; do_pretrain_sr's
exact resume; validate_sr against validate; the exported weights through MODEL.SR_SCRATCH = False."""
import numpy as np
import pytest
import torch

from golden_utils import load_golden, max_rel_to_scale

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IT = 20001          # inside SR_PRETRAIN_ITER [1, 30001) and past both KBPN module-pretraining windows: every KBPN tensor trains


def _cfg(**kw):
    """keys as SECTION__KEY"""
    from csbsr_amd.config import cfg
    c = cfg.clone()
    for k, v in kw.items():
        sec, key = k.split("__")
        c[sec][key] = v
    return c


def _sr_model(cfg, style="random", **kw):
    from csbsr_amd.modeling.build_model import SRModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    m = SRModelWithLoss(cfg, device=DEV, **kw)
    deterministic_fill(m.state_dict(), style)
    return m


def _joint_model(cfg, style="random", **kw):
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    m = JointModelWithLoss(cfg, 1000, 0, None, device=DEV, **kw)
    deterministic_fill(m.state_dict(), style)
    return m


# ----------------------------------------------------------------------------------------------------------------- 1. the reference's vectors
@pytest.mark.parametrize("case", ["e2e_pspnet_it1", "e2e_pspnet_konly_it10001", "e2e_pspnet_it20001"])
def test_forward_matches_golden(case):
    """The three fixtures lie inside SR_PRETRAIN_ITER, so the reference's scalar loss is its sr_loss mean.  Bounds: those
    tests/test_joint_gpu.py::test_forward_matches_golden applies to the same fixtures (none of the three carries one of its widened
    variants: no pixel shuffle, residual learning on, error summed at HR, no oriented weight), restated: 1e-3 of the tensor's maximum."""
    g = load_golden(case)
    assert not bool(g.get("pixel_shuffle", False)) and bool(g.get("residual_learning", True)) and not bool(g.get("lr_error", False))
    assert float(g.get("sfo_sr_amp", 0.0)) == 0
    cfg = _cfg(MODEL__SCALE_FACTOR=int(g["scale"]))
    if "residual_learning" in g:
        cfg.SOLVER.ONLY_KERNEL_LOSS_FOR_PRETRAIN = bool(g["only_kernel_loss"])
    if "kernel_sft" in g:
        cfg.MODEL.KBPN_KERNEL_SFT = bool(g["kernel_sft"])
    if "zero_pad_kernel" in g:
        cfg.MODEL.ZERO_PAD_KERNEL = bool(g["zero_pad_kernel"])
    it = int(g["it"])
    assert cfg.SOLVER.SR_PRETRAIN_ITER[0] <= it < cfg.SOLVER.SR_PRETRAIN_ITER[1]
    m = _sr_model(cfg, antialias=bool(g["antialias"]))
    m.micro_batch, m.max_resident = 8, 8
    m.dropout_masks = {}
    m.train()
    t = lambda k: torch.from_numpy(g[k])
    sr_l, sr, kp = m(it, t("x"), sr_targets=t("hr"), kernel_targets=t("kernel"))
    outs = {"sr_loss": sr_l.detach().cpu(), "sr_preds": sr.cpu(), "kernel_preds": kp.cpu()}
    worst = {k: max_rel_to_scale(v, g[k]) for k, v in outs.items()}
    # the scalar: |mean(a) - mean(b)| <= max |a - b|, so it is held to the same 1e-3 of the loss vector's maximum
    e_loss = abs(float(sr_l.detach().mean()) - float(g["loss"])) / float(np.abs(g["sr_loss"]).max())
    print(case, {k: f"{v:.1e}" for k, v in worst.items()}, f"loss {e_loss:.1e}")
    assert tuple(sr.shape) == tuple(g["sr_preds"].shape) and tuple(kp.shape) == tuple(g["kernel_preds"].shape) and sr_l.shape == (sr.shape[0],)
    for k, v in worst.items():
        assert v < 1e-3, (k, v)
    assert e_loss < 1e-3


# ----------------------------------------------------------------------------------------------------------------- 2. the joint model's bits
def _step(m, batch, joint):
    x, hr, mask, k = batch
    m.zero_grad()
    if joint:
        _, sr_l, _, sr, kp = m(IT, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
    else:
        sr_l, sr, kp = m(IT, x, sr_targets=hr, kernel_targets=k)
    sr_l.mean().backward()
    torch.cuda.synchronize()
    grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in m._named_full()
             if isinstance(p, torch.nn.Parameter) and n.startswith("sr_model.")}
    return sr_l.detach().clone(), sr.clone(), kp.clone(), grads, sr_l


@pytest.mark.parametrize("zero_pad", [False, True])
def test_bit_equal_to_the_joint_model_in_the_sr_window(zero_pad):
    """B = 3 in micro-batches of 2 with one resident: one resident micro-batch and one ragged micro-batch whose forward is recomputed in
    the backward, full saves, on both models."""
    from csbsr_amd.data.synthetic import make_batch
    cfg = _cfg(MODEL__ZERO_PAD_KERNEL=zero_pad)
    batch = make_batch(3, 16, scale=4, ksize=21, seed=17)
    res = []
    for joint in (False, True):
        m = (_joint_model if joint else _sr_model)(cfg)
        m.micro_batch, m.max_resident, m.lean_saves, m.dropout_enabled = 2, 1, False, False
        m.train()
        res.append(_step(m, batch, joint))
        assert (m._n_res, m._mb_used, m._lean) == (1, 2, False) and not m.last_step_overflowed
        if not joint:
            rt = m._runtime()
            assert rt["psp"] is None and set(rt["flat"]) == {f"kbpn.{s}" for s in range(5)}
        del m
    (l0, sr0, k0, g0, _), (l1, sr1, k1, g1, _) = res
    assert torch.equal(l0, l1) and torch.equal(sr0, sr1) and torch.equal(k0, k1)
    assert list(g0) == list(g1) and len(g0) >= 154
    trained = 0
    for n in g0:
        assert (g0[n] is None) == (g1[n] is None), n
        if g0[n] is not None:
            assert torch.equal(g0[n], g1[n]), n
            trained += int(float(g0[n].abs().max()) > 0)
    assert trained > 100          # (both did compute gradients: the equality is not that of two idle models)


def test_runs_repeat_no_detector_runtime_and_one_backward_per_forward():
    from csbsr_amd.data.synthetic import make_batch
    cfg = _cfg()
    batch = make_batch(3, 16, scale=4, ksize=21, seed=23)
    m = _sr_model(cfg)
    m.micro_batch, m.max_resident, m.dropout_enabled = 2, 1, False
    m.train()
    a = _step(m, batch, False)
    b = _step(m, batch, False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for n in a[3]:
        assert (a[3][n] is None) == (b[3][n] is None) and (a[3][n] is None or torch.equal(a[3][n], b[3][n])), n
    assert sum(v is not None for v in a[3].values()) > 100
    rt = m._runtime()
    assert rt["psp"] is None and rt["kbpn"] is not None and m.segmentation_model is None
    assert all(k.startswith("sr_model.") for k in rt["P"]) and "seg" not in rt["flat"]
    # the loss scale follows the PSPNet rule: 2^round(log2(B H W)), minus the back-off
    assert rt["eng"].grad_scale == float(2 ** round(np.log2(3 * 64 * 64)))
    m.scale_backoff = 4
    _step(m, batch, False)
    assert rt["eng"].grad_scale == float(2 ** (round(np.log2(3 * 64 * 64)) - 4))
    with pytest.raises(RuntimeError, match="backward called twice"):
        b[4].mean().backward()
    # eval / no_grad: nothing is kept and the outputs carry no graph
    m.eval()
    with torch.no_grad():
        sr_l, sr, kp = m(IT, batch[0], sr_targets=batch[1], kernel_targets=batch[3])
    assert not sr_l.requires_grad and sr_l.grad_fn is None and torch.isfinite(sr_l).all()


# ----------------------------------------------------------------------------------------------------------------- 3. loader
def test_image_only_loader_yields_the_bytes_of_the_loader_with_masks():
    from csbsr_amd.data.resident import DeviceTrainLoader, ResidentDataset
    import resident_cases as RC
    sizes = [(40, 52), (36, 45), (33, 38), (50, 33), (37, 64), (44, 41)]
    images, masks = RC.random_pairs(np.random.default_rng(0), sizes)
    only, both = ResidentDataset(images, device=DEV), ResidentDataset(images, masks, device=DEV)
    for kw in ({}, {"resized_crop": {"scale": (0.4, 1.0), "ratio": (0.75, 1.33)}, "vflip_p": 0.3}, {"blur": False}):
        mk = lambda ds: DeviceTrainLoader(ds, 32, 4, batch_size=4, seed=5, num_iterations=3, **kw)
        n = 0
        for a, b in zip(mk(only), mk(both)):
            assert len(a) == 3 and len(b) == 5
            x, hr, k = a
            assert tuple(x.shape[1:]) == (3, 8, 8) and tuple(hr.shape[1:]) == (3, 32, 32) and tuple(k.shape[1:]) == (1, 21, 21)
            assert torch.equal(x, b[0]) and torch.equal(hr, b[1]) and torch.equal(k, b[3])
            n += 1
        assert n == 3


# ----------------------------------------------------------------------------------------------------------------- 4. the loop
def _images():
    """five smooth uint8 images of 64 .. 80 px"""
    rng = np.random.default_rng(7)
    images = []
    for H, W in ((64, 80), (72, 64), (80, 80), (66, 71), (75, 68)):
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 60 * np.sin(xx / rng.uniform(4, 9) + rng.uniform(0, 3)) * np.cos(yy / rng.uniform(4, 9))
        images.append(np.clip(base[:, :, None] + rng.normal(0, 12, size=(H, W, 3)), 0, 255).astype(np.uint8))
    return images


def test_resumed_pretraining_is_the_uninterrupted_run(tmp_path):
    """Six iterations at B = 2 in one go against three, a checkpoint, NEW model / optimiser / loader objects, ``resume`` and three more:
    weights, Adam state and log records are bit-identical."""
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader, ResidentDataset
    cfg = _cfg(SOLVER__BATCH_SIZE=2, SOLVER__SCHEDULER=True)
    ds = ResidentDataset(_images(), device=DEV)
    loader = lambda n, seed: DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=n, seed=seed, drop_last=True)

    def run(model, opt, ld, resume_iter, out=None):
        logs = []
        T.do_pretrain_sr(cfg, model, opt, T.build_scheduler(cfg, opt, resume_iter, scheduler_flag=False), ld, resume_iter=resume_iter,
                         log_step=2, save_step=3, output_dir=out, log=logs.append)
        return [(r["iteration"], r["sr_loss"], r["lr"], r["overflow_steps"]) for r in logs if "sr_loss" in r]
    full = _sr_model(cfg)
    opt_full = T.build_optimizer(cfg, full)
    logs_full = run(full, opt_full, loader(6, 31), 0)
    assert [r[0] for r in logs_full] == [2, 4, 6] and all(r[2] == cfg.SOLVER.LR and r[3] == 0 for r in logs_full)
    assert all(np.isfinite(r[1]) and r[1] > 0 for r in logs_full)

    first = _sr_model(cfg)
    logs_a = run(first, T.build_optimizer(cfg, first), loader(3, 31), 0, str(tmp_path))
    for kind in ("model", "optimizer", "trainer"):
        assert (tmp_path / kind / "iteration_3.pth").is_file()
    assert all(k.startswith("sr_model.") for k in torch.load(tmp_path / "model" / "iteration_3.pth"))
    del first
    second = _sr_model(cfg, style="contractive")
    with torch.no_grad():
        for p in second.parameters():
            p.mul_(0.5)                                      # not the weights the run stopped with
    opt_second = T.build_optimizer(cfg, second)
    ld = loader(6, 999)
    it = T.resume(cfg, str(tmp_path), 3, second, opt_second, ld)
    assert it == 3
    logs_b = run(second, opt_second, ld, it)
    assert logs_a + logs_b == logs_full                      # (the window 3 .. 4 straddles the checkpoint: its sum came from the file)
    sd, sd_full = second.state_dict(), full.state_dict()
    moved = 0
    fresh = _sr_model(cfg).state_dict()
    for name, t in sd.items():
        assert torch.equal(t, sd_full[name]), name
        moved += int(not torch.equal(t.cpu(), fresh[name].cpu()))
    assert moved > 100
    n_state = 0
    for p, q in zip(opt_second.param_groups[0]["params"], opt_full.param_groups[0]["params"]):
        assert set(opt_second.state[p]) == set(opt_full.state[q])
        for key, v in opt_second.state[p].items():
            assert torch.equal(torch.as_tensor(v).cpu(), torch.as_tensor(opt_full.state[q][key]).cpu()), key
            n_state += 1
    assert n_state > 300 and {float(s["step"]) for s in opt_second.state.values() if "step" in s} == {6.0}


def test_validate_sr_equals_the_sr_fields_of_validate():
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader, ResidentDataset
    cfg = _cfg(SOLVER__BATCH_SIZE=2)
    images = _images()
    masks = [(255 * (np.hypot(*np.mgrid[0:a.shape[0], 0:a.shape[1]]) % 23 < 3)).astype(np.uint8) for a in images]
    only, both = ResidentDataset(images, device=DEV), ResidentDataset(images, masks, device=DEV)
    mk = lambda ds: DeviceTrainLoader(ds, 64, 4, batch_size=2, seed=1, shuffle=False)
    sr_only, joint = _sr_model(cfg, "contractive"), _joint_model(cfg, "contractive")
    for k, v in sr_only.state_dict().items():
        assert torch.equal(v, joint.state_dict()[k]), k
    sr_only.train()
    got = T.validate_sr(sr_only, mk(only), IT, seed=7)
    assert sr_only.training and (got["batches"], got["images"]) == (3, 5)
    assert got == T.validate_sr(sr_only, mk(only), IT, seed=7)
    want = T.validate(joint, mk(both), IT, seed=7)
    print("validate_sr:", got, "validate:", want)
    for key, ref in (("eval_sr_loss", "eval_sr_loss"), ("psnr", "psnr"), ("ssim", "ssim"), ("kernel_psnr", "kernel_psnr")):
        assert got[key] == want[ref], key
    assert np.isfinite(list(got.values())).all() and got["psnr"] > 5


def test_exported_weights_through_sr_scratch_false(tmp_path):
    from csbsr_amd import trainer as T
    from csbsr_amd.data.synthetic import make_batch
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    cfg = _cfg()
    x, hr, mask, k = make_batch(2, 16, scale=4, ksize=21, seed=29)
    src = _sr_model(cfg)
    path = T.export_pretrained_sr(src, cfg, root=str(tmp_path))
    assert path.endswith("KBPN_pretrain_x4_stage4_bicubic7.pth")
    joint = JointModelWithLoss(_cfg(MODEL__SR_SCRATCH=False), 1000, 0, None, device=DEV, pretrained_root=str(tmp_path))
    src.eval()
    joint.eval()
    with torch.no_grad():
        sr_l, sr, kp = src(IT, x, sr_targets=hr, kernel_targets=k)
        _, sr_lj, _, srj, kpj = joint(IT, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
    assert torch.equal(sr, srj) and torch.equal(kp, kpj) and torch.equal(sr_l, sr_lj)
    assert float(sr.abs().max()) > 0 and torch.isfinite(sr).all()
