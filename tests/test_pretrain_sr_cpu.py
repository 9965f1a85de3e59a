"""Host side of SR-only pretraining: SRModelWithLoss's state and refusals, MODEL.SR_SCRATCH = False, the image-only resident loader's
decisions and do_pretrain_sr / validate_sr over a stub model.  No GPU."""
import os

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import LambdaLR

import resident_cases as RC

# the reference's format strings (model/engine/trainer.py:300, :393), quoted
REF_TRAIN_LINE = "===> Iter: {:07d}, LR: {:.5f}, Cost: {:.2f}s, Eta: {}, SR_Loss({}): {:.6f}"
REF_EVAL_LINE = "=====> SR_Loss({}): {:.6f} PSNR:{:.4f} SSIM:{:.4f} PSNR(Kernel):{:.4f}"


def _cfg(**kw):
    """keys as SECTION__KEY"""
    from csbsr_amd.config import cfg
    c = cfg.clone()
    for k, v in kw.items():
        sec, key = k.split("__")
        c[sec][key] = v
    return c


@pytest.fixture(scope="module")
def T():
    from csbsr_amd import trainer
    return trainer


# ----------------------------------------------------------------------------------------------------------------- 1. construction
def test_state_is_the_sr_model_part_of_the_joint_model_in_order():
    from csbsr_amd.modeling.build_model import JointModelWithLoss, SRModelWithLoss
    for kw in ({}, {"MODEL__SR_PIXEL_SHUFFLE": True}, {"MODEL__ZERO_PAD_KERNEL": True, "MODEL__SCALE_FACTOR": 2, "MODEL__NUM_STAGES": 3}):
        m = SRModelWithLoss(_cfg(**kw))
        j = JointModelWithLoss(_cfg(**kw), 1000, 0, None)
        want = [(k, tuple(v.shape)) for k, v in j.state_dict().items() if k.startswith("sr_model.")]
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want and len(want) > 100
        assert not any("segmentation_model" in k for k in m.state_dict())
        assert m.segmentation_model is None and not any("segmentation_model" in n for n, _ in m.named_parameters())
        jp = [tuple(p.shape) for n, p in j.named_parameters() if n.startswith("sr_model.")]
        assert [tuple(p.shape) for p in m.parameters()] == jp
        assert {m._bucket_of(k) for k in m.state_dict()} == {f"kbpn.{s}" for s in range(m.pc.num_stages + 1)}


def test_reference_positional_arguments():
    from csbsr_amd.modeling.build_model import SRModelWithLoss
    m = SRModelWithLoss(_cfg(), None, 123, 7)          # (cfg, sr_transforms, num_train_ds, resume_iter), build_model.py:536
    assert m.sr_loss_fn == "KBPNLoss" and m.scale_backoff == 0 and m.reducer is None


@pytest.mark.parametrize("kw", [{"MODEL__SR": "bicubic"}, {"MODEL__SR": "DBPN"}, {"SOLVER__SR_LOSS_FUNC": "L1"}, {"MODEL__SCALE_FACTOR": 1},
                                {"SOLVER__ORIENTED_WEIGHT_ITER": 100, "SOLVER__SEG_FAIL_ORIENTED_WEIGHT4SR_AMP": 1.0},
                                {"SOLVER__ORIENTED_WEIGHT_ITER": 100, "SOLVER__CRACK_ORIENTED_WEIGHT4SR_AMP": 0.5}])
def test_refusals(kw):
    from csbsr_amd.modeling.build_model import SRModelWithLoss
    with pytest.raises(NotImplementedError):
        SRModelWithLoss(_cfg(**kw))


def test_oriented_amplitudes_without_a_start_iteration_are_accepted():
    from csbsr_amd.modeling.build_model import SRModelWithLoss
    SRModelWithLoss(_cfg(SOLVER__ORIENTED_WEIGHT_ITER=-1, SOLVER__SEG_FAIL_ORIENTED_WEIGHT4SR_AMP=1.0))
    SRModelWithLoss(_cfg(SOLVER__ORIENTED_WEIGHT_ITER=100))


# ----------------------------------------------------------------------------------------------------------------- 2. SR_SCRATCH = False
def _pretrain_file(tmp_path, cfg, name, extra=None):
    from csbsr_amd.modeling.build_model import SRModelWithLoss
    src = SRModelWithLoss(cfg, seed=77)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    sd.update(extra or {})
    os.makedirs(tmp_path / "pretrain", exist_ok=True)
    torch.save(sd, tmp_path / "pretrain" / name)
    return sd


def test_sr_scratch_false_loads_the_pretrained_file(tmp_path):
    from csbsr_amd.modeling.build_model import JointModelWithLoss, JointModel, SRModelWithLoss, pretrained_sr_path
    scratch = _cfg()
    assert scratch.MODEL.SR_SCRATCH is True                                  # the project's default
    assert (scratch.BLUR.KERNEL_SIZE, scratch.BLUR.KERNEL_SIZE_OUTPUT) == (7, 21)
    assert pretrained_sr_path(scratch, "weights") == os.path.join("weights", "pretrain", "KBPN_pretrain_x4_stage4_bicubic7.pth")
    same = _cfg(BLUR__KERNEL_SIZE=21, MODEL__SCALE_FACTOR=2, MODEL__NUM_STAGES=3)
    assert pretrained_sr_path(same, "w") == os.path.join("w", "pretrain", "KBPN_pretrain_x2_stage3.pth")
    sd = _pretrain_file(tmp_path, scratch, "KBPN_pretrain_x4_stage4_bicubic7.pth")
    cfg = _cfg(MODEL__SR_SCRATCH=False)
    root = str(tmp_path)
    ref_joint = JointModelWithLoss(scratch, 1000, 0, None).state_dict()
    built = (JointModelWithLoss(cfg, 1000, 0, None, pretrained_root=root), JointModel(cfg, pretrained_root=root),
             SRModelWithLoss(cfg, pretrained_root=root))
    for m in built:
        got = m.state_dict()
        for k, v in sd.items():
            assert torch.equal(got[k], v), k
        assert not torch.equal(got["sr_model.feat.0.weight"], ref_joint["sr_model.feat.0.weight"])
        for k, v in got.items():
            if k.startswith("segmentation_model."):
                assert torch.equal(v, ref_joint[k]), k                       # the detector keeps its seeded init
    assert sum(k.startswith("segmentation_model.") for k in built[0].state_dict()) > 100
    assert built[2].pretrained_sr_path == os.path.join(root, "pretrain", "KBPN_pretrain_x4_stage4_bicubic7.pth")
    # the plain name when the two kernel sizes are equal
    _pretrain_file(tmp_path, same, "KBPN_pretrain_x2_stage3.pth")
    same.MODEL.SR_SCRATCH = False
    assert SRModelWithLoss(same, pretrained_root=root).pretrained_sr_path.endswith("KBPN_pretrain_x2_stage3.pth")


def test_sr_scratch_false_is_non_strict_and_refuses_unexpected_keys(tmp_path):
    from csbsr_amd.modeling.build_model import JointModelWithLoss, SRModelWithLoss
    cfg = _cfg(MODEL__SR_SCRATCH=False)
    with pytest.raises(FileNotFoundError):
        SRModelWithLoss(cfg, pretrained_root=str(tmp_path))
    with pytest.raises(FileNotFoundError):
        JointModelWithLoss(cfg, 1000, 0, None, pretrained_root=str(tmp_path))
    # a file that lacks a tensor: that tensor keeps its init (strict=False)
    name = "KBPN_pretrain_x4_stage4_bicubic7.pth"
    sd = _pretrain_file(tmp_path, _cfg(), name)
    first = next(iter(sd))
    torch.save({k: v for k, v in sd.items() if k != first}, tmp_path / "pretrain" / name)
    m = SRModelWithLoss(cfg, pretrained_root=str(tmp_path))
    assert torch.equal(m.state_dict()[first], SRModelWithLoss(_cfg()).state_dict()[first])
    # an unexpected key -- a detector tensor of a whole joint checkpoint is one, cut by len("sr_model.") like every key
    for extra in ({"sr_model.not_a_layer.weight": torch.zeros(1)}, {"segmentation_model.final.0.weight": torch.zeros(1)}):
        _pretrain_file(tmp_path, _cfg(), name, extra)
        with pytest.raises(RuntimeError):
            SRModelWithLoss(cfg, pretrained_root=str(tmp_path))


def test_export_pretrained_sr_round_trip(tmp_path, T):
    from csbsr_amd.modeling.build_model import JointModelWithLoss, SRModelWithLoss
    cfg = _cfg()
    src = SRModelWithLoss(cfg, seed=5)
    path = T.export_pretrained_sr(src, cfg, root=str(tmp_path / "a"))
    assert path == os.path.join(str(tmp_path / "a"), "pretrain", "KBPN_pretrain_x4_stage4_bicubic7.pth") and os.path.isfile(path)
    loaded = JointModelWithLoss(_cfg(MODEL__SR_SCRATCH=False), 1000, 0, None, pretrained_root=str(tmp_path / "a"))
    for k, v in src.state_dict().items():
        assert torch.equal(loaded.state_dict()[k], v), k
    # from a joint model, and from a DataParallel-style state_dict of one: only sr_model.* is written
    joint = JointModelWithLoss(cfg, 1000, 0, None, seed=9)
    for i, obj in enumerate((joint, {"module." + k: v for k, v in joint.state_dict().items()})):
        p = T.export_pretrained_sr(obj, cfg, root=str(tmp_path / f"j{i}"))
        assert list(torch.load(p)) == list(src.state_dict())
        m = SRModelWithLoss(_cfg(MODEL__SR_SCRATCH=False), pretrained_root=str(tmp_path / f"j{i}"))
        for k, v in m.state_dict().items():
            assert torch.equal(v, joint.state_dict()[k]), k
    with pytest.raises(ValueError):
        T.export_pretrained_sr({"segmentation_model.x": torch.zeros(1)}, cfg, root=str(tmp_path))


# ----------------------------------------------------------------------------------------------------------------- 3. loader
SIZES = [(40, 52), (36, 45), (33, 38), (50, 33), (37, 64), (44, 41)]


def _datasets():
    from csbsr_amd.data import resident as R
    images, masks = RC.random_pairs(np.random.default_rng(0), SIZES)
    return R, R.ResidentDataset(images, masks, device="cpu"), R.ResidentDataset(images, device="cpu"), images


def _same(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and len(a) > 0 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))


def test_image_only_dataset_views():
    R, with_masks, only, images = _datasets()
    assert only.mask is None and only.mask_pool is None and with_masks.mask is not None
    assert only.nbytes == sum(a.size for a in images) and with_masks.nbytes == only.nbytes + sum(H * W for H, W in SIZES)
    img, m = only.sample(2)
    assert m is None and np.array_equal(img, images[2])
    a, b = only.split(0.7, seed=3)
    a2, b2 = with_masks.split(0.7, seed=3)
    assert (len(a), len(b)) == (4, 2) and a.indices.tolist() == a2.indices.tolist() and b.indices.tolist() == b2.indices.tolist()
    assert a.mask is None and np.array_equal(a.sample(1)[0], images[int(a.indices[1])])
    sub = only.subset([5, 0])
    assert sub.indices.tolist() == [5, 0] and sub.nbytes == only.nbytes
    only.check_selection(np.array([[0, 8, 20, 1, 0]], dtype=np.int32), 32, 32)
    with pytest.raises(ValueError):
        only.check_selection(np.array([[0, 9, 20, 1, 0]], dtype=np.int32), 32, 32)          # 9 + 32 > 40
    only.check_windows(np.array([[2, 0, 0, 0, 1, 33, 38]], dtype=np.int32), 32, 32)
    with pytest.raises(ValueError):
        only.check_windows(np.array([[2, 1, 0, 0, 1, 33, 38]], dtype=np.int32), 32, 32)
    with pytest.raises(ValueError):
        R.ResidentDataset([], None, device="cpu")
    with pytest.raises(ValueError):
        R.ResidentDataset(images, [np.zeros((4, 4), np.uint8)], device="cpu")


def test_from_image_dir_globs_png(tmp_path):
    from PIL import Image
    from csbsr_amd.data.resident import ResidentDataset
    rng = np.random.default_rng(1)
    arrays = {f"{n}.png": rng.integers(0, 256, size=(9 + i, 11, 3), dtype=np.uint8) for i, n in enumerate(("b", "a", "c"))}
    for n, a in arrays.items():
        Image.fromarray(a).save(tmp_path / n)
    Image.fromarray(arrays["a.png"]).save(tmp_path / "ignored.bmp")
    ds = ResidentDataset.from_image_dir(str(tmp_path), device="cpu")
    assert ds.names == ["a.png", "b.png", "c.png"] and ds.mask is None and len(ds) == 3
    for i, n in enumerate(ds.names):
        assert np.array_equal(ds.sample(i)[0], arrays[n])
    with pytest.raises(FileNotFoundError):
        ResidentDataset.from_image_dir(str(tmp_path), pattern="*.jpg", device="cpu")


@pytest.mark.parametrize("kw", [{}, {"vflip_p": 0.4}, {"resized_crop": {"scale": (0.3, 1.0), "ratio": (0.75, 1.33)}, "vflip_p": 0.4},
                                {"shuffle": False}, {"drop_last": True, "isotropic": True}, {"blur": False}])
def test_image_only_loader_takes_the_decisions_of_the_loader_with_masks(kw):
    R, with_masks, only, _ = _datasets()
    mk = lambda ds: R.DeviceTrainLoader(ds, 32, 4, batch_size=4, seed=11, num_iterations=None if kw.get("shuffle") is False else 5, **kw)
    a, b = mk(only), mk(with_masks)
    assert a.image_only and not b.image_only and len(a) == len(b)
    da = list(a.iter_decisions())
    assert _same(da, b.iter_decisions())
    assert da[0][0].shape[1] == (7 if "resized_crop" in kw else 5)
    if "vflip_p" in kw:
        assert 0 < sum(int(s[:, 4].sum()) for s, _ in da) < sum(len(s) for s, _ in da)
    # views too: a split of the image-only dataset draws what the same split of the dataset with masks draws
    assert _same(mk(only.split(0.7, 3)[0]).iter_decisions(), mk(with_masks.split(0.7, 3)[0]).iter_decisions())


def test_image_only_loader_state_round_trip_and_shard_refusal():
    R, with_masks, only, _ = _datasets()
    mk = lambda ds, seed=9: R.DeviceTrainLoader(ds, 32, 4, batch_size=4, seed=seed, num_iterations=6, vflip_p=0.2)
    whole = list(mk(with_masks).iter_decisions())
    a = mk(only)
    it = a.iter_decisions()
    head = [next(it) for _ in range(2)]
    b = mk(only, seed=4242)
    b.load_state_dict(a.state_dict())
    assert _same(head + list(b.iter_decisions()), whole) and b.produced == 6
    c = mk(with_masks, seed=1)                    # the state is interchangeable: the decisions do not depend on the mask pool
    c.load_state_dict(a.state_dict())
    assert _same(head + list(c.iter_decisions()), whole)
    with pytest.raises(NotImplementedError):
        R.DeviceTrainLoader(only, 32, 4, batch_size=2, shard=(0, 2))
    R.DeviceTrainLoader(with_masks, 32, 4, batch_size=2, shard=(0, 2))
    from csbsr_amd import _lib as L
    with pytest.raises(L.CsbsrHipError):          # batches exist on a GPU only
        next(iter(mk(only)))


# ----------------------------------------------------------------------------------------------------------------- 4. trainer over a stub
class _Stub(torch.nn.Module):
    """the surface do_pretrain_sr / validate_sr touch: SRModelWithLoss.forward's signature and three outputs, last_step_overflowed"""

    def __init__(self, calls=None):
        super().__init__()
        self.calls = [] if calls is None else calls
        self.w = torch.nn.Parameter(torch.tensor([0.5, -0.25]))
        self.last_step_overflowed = False
        self.seen = []

    def train(self, mode=True):
        self.calls.append("train" if mode else "eval")
        return super().train(mode)

    def forward(self, iter, x, sr_targets=None, kernel_targets=None):
        self.calls.append("forward")
        self.seen.append((iter, self.training, torch.is_grad_enabled(), kernel_targets.requires_grad))
        sr_loss = (sr_targets.mean((1, 2, 3)) - self.w[1]) ** 2 + (x.mean((1, 2, 3)) * self.w[0]) ** 2
        return sr_loss, sr_targets + 0.25 * x.mean(), kernel_targets * 2


class _Opt(torch.optim.Adam):
    def __init__(self, calls, *a, **kw):
        super().__init__(*a, **kw)
        self.calls = calls

    def zero_grad(self, *a, **kw):
        self.calls.append("zero_grad")
        return super().zero_grad(*a, **kw)

    def step(self, *a, **kw):
        self.calls.append("step")
        return super().step(*a, **kw)


def _batches(n, sizes=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        B = 2 if sizes is None else sizes[i]
        out.append((torch.rand(B, 3, 4, 4, generator=g), torch.rand(B, 3, 8, 8, generator=g), torch.rand(B, 1, 5, 5, generator=g)))
    return out


def _run(T, cfg, n, tmp_path=None, resume_iter=0, model=None, eval_batches=None, batches=None, **kw):
    m = _Stub() if model is None else model
    calls = m.calls
    opt = _Opt(calls, m.parameters(), lr=cfg.SOLVER.LR)
    sched = T.build_scheduler(cfg, opt, resume_iter, scheduler_flag=False)
    step = sched.step
    sched.step = lambda *a, **k: (calls.append("sched"), step(*a, **k))[1]
    logs = []
    T.do_pretrain_sr(cfg, m, opt, sched, _batches(n) if batches is None else batches, eval_batches, resume_iter=resume_iter, log=logs.append,
                     output_dir=None if tmp_path is None else str(tmp_path), **kw)
    return m, opt, logs, calls


def test_iteration_order_and_hooks(T):
    cfg = _cfg()
    marks = []
    m = _Stub()
    m.w.register_hook(lambda g: m.calls.append("backward"))
    hooks = {"before_step": lambda it, model: model.calls.append(f"before{it}"),
             "after_step": lambda it, model, record: marks.append((it, None if record is None else record["iteration"]))}
    _, _, logs, calls = _run(T, cfg, 3, model=m, log_step=2, hooks=hooks, resume_iter=10)
    per_iter = ["train", "zero_grad", "forward", "backward", "step", "sched"]          # trainer.py:275-290
    assert calls == ["before11"] + per_iter + ["before12"] + per_iter + ["before13"] + per_iter
    assert [s[0] for s in m.seen] == [11, 12, 13] and all(s[1] and s[2] and not s[3] for s in m.seen)
    assert marks == [(11, None), (12, 12), (13, None)] and [r["iteration"] for r in logs] == [12]


def test_record_keys_window_mean_and_checkpoint_files(T, tmp_path):
    cfg = _cfg()
    m, opt, logs, _ = _run(T, cfg, 6, tmp_path, log_step=2, save_step=3)
    train_logs = [r for r in logs if "sr_loss" in r]
    assert [r["iteration"] for r in train_logs] == [2, 4, 6]
    for r in train_logs:
        assert set(r) == {"iteration", "lr", "sr_loss", "overflow_steps", "cost_s", "eta", "sr_loss_func"}
        assert r["sr_loss_func"] == "KBPN" and r["overflow_steps"] == 0 and r["lr"] == cfg.SOLVER.LR
    # the window mean: Python-float sums of the batch means (trainer.py:285, :298)
    ref = _Stub()
    ropt = torch.optim.Adam(ref.parameters(), lr=cfg.SOLVER.LR)
    want, acc = [], 0.0
    for it, (x, hr, k) in enumerate(_batches(6), 1):
        ropt.zero_grad()
        loss = ref(it, x, hr, k)[0].mean()
        acc += loss.item()
        loss.backward()
        ropt.step()
        if it % 2 == 0:
            want.append(acc / 2)
            acc = 0.0
    assert [r["sr_loss"] for r in train_logs] == want and torch.equal(m.w, ref.w)
    assert [r["iteration"] for r in logs if "checkpoint" in r] == [3, 6]
    for it in (3, 6):
        for kind in ("model", "optimizer", "trainer"):
            assert (tmp_path / kind / f"iteration_{it}.pth").is_file()
    assert sorted(os.listdir(tmp_path)) == ["model", "optimizer", "trainer"] and len(os.listdir(tmp_path / "model")) == 2
    assert list(torch.load(tmp_path / "model" / "iteration_6.pth")) == ["w"]
    st = torch.load(tmp_path / "trainer" / "iteration_3.pth")
    assert st["iteration"] == 3 and st["ss_loss_fn"] is None and float(st["logging"]["sums"].sum()) > 0          # mid-window
    assert float(torch.load(tmp_path / "trainer" / "iteration_6.pth")["logging"]["sums"].abs().sum()) == 0
    # overflowed steps are counted from the host flag
    m2 = _Stub()
    m2.last_step_overflowed = True
    assert [r["overflow_steps"] for r in _run(T, cfg, 4, model=m2, log_step=2)[2]] == [2, 4]


def test_resume_continues_the_stub_run_exactly(T, tmp_path):
    cfg = _cfg()
    full, _, logs_full, _ = _run(T, cfg, 6, log_step=4)
    _run(T, cfg, 3, tmp_path, log_step=4, save_step=3)
    m = _Stub()
    opt = _Opt(m.calls, m.parameters(), lr=cfg.SOLVER.LR)
    it = T.resume(cfg, str(tmp_path), 3, m, opt, None)
    logs = []
    T.do_pretrain_sr(cfg, m, opt, T.build_scheduler(cfg, opt, it, scheduler_flag=False), _batches(6)[3:], resume_iter=it, log_step=4,
                     log=logs.append)
    assert torch.equal(m.w, full.w)
    assert [(r["iteration"], r["sr_loss"]) for r in logs] == [(r["iteration"], r["sr_loss"]) for r in logs_full] and len(logs) == 1


def test_the_rate_is_constant_whatever_the_config_says(T):
    from csbsr_amd.utils.lr_scheduler import UpDownScheduler, BOOST_WINDOW, BOOST_FACTOR
    pre = 5 - BOOST_WINDOW[0]          # the boost window would open at iteration 5
    cfg = _cfg(SOLVER__SCHEDULER=True, SOLVER__SR_PRETRAIN_ITER=[pre - 5, pre])
    w = torch.nn.Parameter(torch.zeros(1))
    s = T.build_scheduler(cfg, torch.optim.SGD([w], lr=1.0), 3, scheduler_flag=False)
    f = s.lr_lambdas[0]
    assert isinstance(s, LambdaLR) and isinstance(f, UpDownScheduler) and (f.pretrain_iter, f.resume_iter, f.scheduler_flag) == (pre, 3, False)
    # the keyword's default keeps SOLVER.SCHEDULER
    assert T.build_scheduler(cfg, torch.optim.SGD([w], lr=1.0), 3).lr_lambdas[0].scheduler_flag is True
    assert T.build_scheduler(_cfg(), torch.optim.SGD([w], lr=1.0)).lr_lambdas[0].scheduler_flag is False
    _, _, logs, _ = _run(T, cfg, 8, log_step=1)
    assert [r["lr"] for r in logs] == [cfg.SOLVER.LR] * 8
    boosted = LambdaLR(torch.optim.SGD([w], lr=1.0), lr_lambda=UpDownScheduler(pre, 0, True))
    assert BOOST_FACTOR in [boosted.lr_lambdas[0](i) for i in range(8)]          # (with the flag on the same run would have been boosted)


@pytest.fixture
def host_metrics(monkeypatch):
    """validate_sr computes its metrics with the device kernels; over the CPU stub a plain torch stand-in replaces them"""
    from csbsr_amd.utils import estimate_metrics as EM

    def psnr_ssim(a, b):
        return 10 * torch.log10(1 / ((a - b) ** 2).mean((1, 2, 3))), ((a - b).abs().mean((1, 2, 3)))
    monkeypatch.setattr(EM, "psnr_ssim", psnr_ssim)
    return psnr_ssim


def test_validate_sr_averages_losses_over_batches_and_metrics_over_images(T, host_metrics):
    m = _Stub()
    m.train()
    ev = _batches(3, sizes=[2, 2, 1], seed=5)
    m.calls.clear()
    got = T.validate_sr(m, ev, 17)
    assert m.calls == ["eval", "forward", "forward", "forward", "train"] and m.training
    assert [s[:3] for s in m.seen] == [(17, False, False)] * 3
    # the reference's bookkeeping (trainer.py:331-353, :390-393)
    eval_sr_loss, psnr_scores, ssim_scores, kernel_psnr_scores = 0, np.array([]), np.array([]), np.array([])
    with torch.no_grad():
        for x, hr, k in ev:
            sr_loss, sr, kp = m(17, x, hr, k)
            sr, kp = sr.clone(), kp.clone()
            assert (kp > 1).any() and (sr > 1).any()                          # (the clamps below do something)
            sr[sr > 1] = 1
            sr[sr < 0] = 0
            kp[kp > 1] = 1
            kp[kp < 0] = 0
            ps, ss = host_metrics(sr, hr)
            psnr_scores, ssim_scores = np.append(psnr_scores, ps), np.append(ssim_scores, ss)
            kernel_psnr_scores = np.append(kernel_psnr_scores, host_metrics(kp, k)[0])
            eval_sr_loss += sr_loss.mean().item()
    eval_sr_loss /= len(ev)
    assert got == {"eval_sr_loss": eval_sr_loss, "psnr": sum(psnr_scores) / len(psnr_scores), "ssim": sum(ssim_scores) / len(ssim_scores),
                   "kernel_psnr": sum(kernel_psnr_scores) / len(kernel_psnr_scores), "batches": 3, "images": 5}
    # the short batch is a third of the loss and a fifth of the metrics
    per_image = torch.cat([m(17, x, hr, k)[0].detach() for x, hr, k in ev])
    assert got["eval_sr_loss"] != pytest.approx(float(per_image.mean()), rel=1e-4)
    with pytest.raises(ValueError):
        T.validate_sr(m, [], 17)
    m.eval()
    T.validate_sr(m, ev, 17)
    assert not m.training


def test_printed_lines_are_the_references(T, capsys, tmp_path, host_metrics):
    cfg = _cfg()
    records = []

    def log(r):
        records.append(r)
        T.print_pretrain_line(r)
    m = _Stub()
    opt = torch.optim.Adam(m.parameters(), lr=cfg.SOLVER.LR)
    T.do_pretrain_sr(cfg, m, opt, T.build_scheduler(cfg, opt, 0, scheduler_flag=False), _batches(2), _batches(2, seed=3), log_step=2, save_step=2,
                     eval_step=2, output_dir=str(tmp_path), log=log)
    out = capsys.readouterr().out
    tr, ck, ev = records
    want = REF_TRAIN_LINE.format(tr["iteration"], tr["lr"], tr["cost_s"], tr["eta"], cfg.SOLVER.SR_LOSS_FUNC, tr["sr_loss"]) + "\n"
    want += "=====> Save Checkpoint to {}".format(os.path.join(str(tmp_path), "model", "iteration_2.pth")) + "\n"
    want += "\nestimation result (iter=2):\n"
    want += REF_EVAL_LINE.format(cfg.SOLVER.SR_LOSS_FUNC, ev["eval_sr_loss"], ev["psnr"], ev["ssim"], ev["kernel_psnr"]) + "\n"
    assert out == want
    assert tr["iteration"] == 2 and ev["iteration"] == 2 and ev["sr_loss_func"] == "KBPN" and ck["checkpoint"].endswith("iteration_2.pth")
    assert out.startswith("===> Iter: 0000002, LR: 0.00002, Cost: ") and ", Eta: 0:00:00, SR_Loss(KBPN): " in out
    import inspect
    assert inspect.signature(T.do_pretrain_sr).parameters["log"].default is T.print_pretrain_line


def test_data_parallel_pretraining_is_refused(T, monkeypatch):
    monkeypatch.setenv("CSBSR_FORCE_DIST", "1")
    m = _Stub()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    class _Untouchable:
        def __iter__(self):
            raise AssertionError("the refusal comes before the first batch")
    with pytest.raises(NotImplementedError):
        T.do_pretrain_sr(_cfg(), m, opt, T.build_scheduler(_cfg(), opt, 0, scheduler_flag=False), _Untouchable())
    assert m.calls == []
