"""The training driver on the device: csbsr_sgd_step against torch.optim.SGD, the reference trajectory driven through do_train, exact
resume from the three checkpoint files, and validate() against a restatement from per-batch model calls."""
import copy

import numpy as np
import pytest
import torch

from golden_utils import load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------------------------- 7. SGD
def _close(a, b, what):
    """<= 2e-6 of the tensor's largest magnitude: three fp32 roundings per quantity and step (fused or unfused multiply-add in each of the
    three updates), six steps: 18 * 2^-24 = 1.1e-6 -- the form and constant of test_adam_step_matches_torch."""
    err, top = float((a - b).abs().max()), float(b.abs().max())
    print(f"  {what}: max |diff| {err:.3e}, bound {2e-6 * top:.3e}")
    assert err <= 2e-6 * top + 1e-30, (what, err, top)


def test_sgd_step_matches_torch():
    from csbsr_amd.optim import SGD
    torch.manual_seed(22)
    shapes = [(1,), (7,), (3, 3, 3, 3), (64, 33, 3, 3), (20000,), (8192,), (128, 128, 8, 8)]
    shapes2 = [(5,), (9001,), (16, 8, 3, 3)]                   # the second group: momentum 0, weight decay 0 (no buffer at all)
    P0 = [torch.randn(s) * 0.1 for s in shapes + shapes2]
    pa = [torch.nn.Parameter(t.clone().cuda()) for t in P0]
    pb = [torch.nn.Parameter(t.clone().cuda()) for t in P0]
    # one tensor that does not start on a 16-byte boundary (a view one element into its allocation): the scalar path, two chunks
    odd = torch.randn(9002) * 0.1
    hold_a, hold_b = odd.clone().cuda(), odd.clone().cuda()
    pa.insert(7, torch.nn.Parameter(hold_a[1:]))
    pb.insert(7, torch.nn.Parameter(hold_b[1:]))
    assert pa[7].data_ptr() % 16 == 4 and pa[7].is_contiguous()
    n1 = 8
    start = [a.detach().clone() for a in pa]
    groups = lambda ps: [{"params": ps[:n1]}, {"params": ps[n1:], "momentum": 0.0, "weight_decay": 0.0}]
    oa = SGD(groups(pa), lr=1e-2, momentum=0.9, weight_decay=5e-4)
    ob = torch.optim.SGD(groups(pb), lr=1e-2, momentum=0.9, weight_decay=5e-4)

    def set_grads(it, A, B):
        for k, (a, b) in enumerate(zip(A, B)):
            if k == 3 and it in (1, 4):
                a.grad = b.grad = None
                continue
            g = torch.randn_like(a) * (10.0 ** (-(k % 4)))
            a.grad, b.grad = g.clone(), g.clone()
    for it in range(6):
        set_grads(it, pa, pb)
        if it == 3:
            for o in (oa, ob):
                for grp in o.param_groups:
                    grp["lr"] = 5e-2
        frozen = (pa[3].detach().clone(), oa.state[pa[3]]["momentum_buffer"].clone()) if it in (1, 4) else None
        oa.step(); ob.step()
        if frozen is not None:          # torch's skip rule: neither the value nor the buffer of a parameter without a gradient moves
            assert torch.equal(pa[3].detach(), frozen[0]) and torch.equal(oa.state[pa[3]]["momentum_buffer"], frozen[1])
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(pa, pb)):
        if k < n1:
            assert set(oa.state[a]) == set(ob.state[b]) == {"momentum_buffer"}
            _close(oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"], f"buffer {k}")
        else:
            assert len(oa.state[a]) == 0 or oa.state[a].get("momentum_buffer") is None
        _close(a.detach(), b.detach(), f"parameter {k}")
        assert not torch.equal(a.detach(), start[k])                    # (and it moved at all)
    assert torch.equal(hold_a[:1].cpu(), odd[:1])                  # the element in front of the view is not ours
    # state_dict interchange, both ways, one more step each (deep copies: load_state_dict shares tensors that are already in place)
    qa = [torch.nn.Parameter(b.detach().clone()) for b in pb]
    o_hip = SGD(groups(qa), lr=1.0)
    o_hip.load_state_dict(copy.deepcopy(ob.state_dict()))        # torch -> HIP
    qb = [torch.nn.Parameter(a.detach().clone()) for a in pa]
    o_torch = torch.optim.SGD(groups(qb), lr=1.0)
    o_torch.load_state_dict(copy.deepcopy(oa.state_dict()))      # HIP -> torch
    assert o_hip.param_groups[0]["lr"] == 5e-2 and o_torch.param_groups[1]["momentum"] == 0.0
    for k, four in enumerate(zip(qa, pb, qb, pa)):
        g = torch.randn_like(four[0]) * (10.0 ** (-(k % 4)))
        for t in four:
            t.grad = g.clone()
    o_hip.step(); ob.step(); o_torch.step(); oa.step()
    torch.cuda.synchronize()
    for k in range(len(pa)):
        _close(qa[k].detach(), pb[k].detach(), f"torch -> HIP, parameter {k}")
        _close(pa[k].detach(), qb[k].detach(), f"HIP -> torch, parameter {k}")
        if k < n1:
            _close(o_hip.state[qa[k]]["momentum_buffer"], ob.state[pb[k]]["momentum_buffer"], f"torch -> HIP, buffer {k}")
            _close(oa.state[pa[k]]["momentum_buffer"], o_torch.state[qb[k]]["momentum_buffer"], f"HIP -> torch, buffer {k}")


# ----------------------------------------------------------------------------------------------------------------- 8. trajectory
def test_trajectory_through_the_trainer():
    """do_train over the first four steps of the reference trajectory (tests/test_trajectory_gpu.py: same fixture, same batches, same
    recorded dropout masks, split precision, HIP Adam) stays within LOSS_EARLY = 2e-3 of the reference's scalar loss, reproduces alpha
    exactly, and leaves parameters BIT-identical to those of that test's hand-written loop run here beside it: the trainer adds logic, not
    arithmetic."""
    from csbsr_amd import trainer as T
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.data.synthetic import make_batch
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.optim import Adam as HipAdam
    from csbsr_amd.utils.detfill import deterministic_fill
    g = load_golden("traj_pspnet_it40000")
    it0, B, lr, scale, seed0 = (int(g[k]) for k in ("it0", "B", "lr", "scale", "seed0"))
    steps, beta = 4, float(g["beta"])
    cfg = base_cfg.clone()
    cfg.MODEL.SCALE_FACTOR, cfg.MODEL.DETECTOR_TYPE = scale, str(g["detector"])
    cfg.SOLVER.TASK_LOSS_WEIGHT, cfg.SOLVER.BATCH_SIZE, cfg.SOLVER.LR = beta, 6, float(g["lr_rate"])

    def build():
        m = JointModelWithLoss(cfg, 1000, 0, None)
        deterministic_fill(m.state_dict(), str(g["fill"]))
        m.detector_precision = "split"
        m.micro_batch, m.max_resident = 8, 8
        m.train()
        params = [p for p in m.parameters() if p.requires_grad]
        m._runtime()
        return m, HipAdam(params, lr=float(g["lr_rate"]), betas=(0.9, 0.999), eps=1e-8)

    def masks(step):
        return {kk.split(".", 2)[2]: torch.from_numpy(v) for kk, v in g.items() if kk.startswith(f"dropmask.{step}.")}
    batches = [make_batch(B, lr, scale=scale, ksize=21, seed=seed0 + step) for step in range(steps)]
    # the hand-written loop
    ref, opt = build()
    for step in range(steps):
        ref.ss_loss_fn.fix_alpha = False
        ref.ss_loss_fn.update_alpha()
        x, hr, mask, k = batches[step]
        ref.dropout_masks = masks(step)
        opt.zero_grad()
        seg_l, sr_l = ref(it0 + step, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)[:2]
        ((1 - beta) * sr_l.mean() + beta * seg_l.mean()).backward()
        assert not ref.last_step_overflowed
        opt.step()
    # the trainer
    m, opt2 = build()
    logs, alphas = [], []

    def before_step(iteration, model):
        model.dropout_masks = masks(iteration - it0)
        assert len(model.dropout_masks) == 5
    T.do_train(cfg, m, opt2, T.build_scheduler(cfg, opt2, it0 - 1), batches, resume_iter=it0 - 1, log_step=1, log=logs.append,
               hooks={"before_step": before_step, "after_step": lambda it, model, rec: alphas.append(model.ss_loss_fn.alpha)})
    assert [r["iteration"] for r in logs] == list(range(it0, it0 + steps))
    for step, r in enumerate(logs):
        loss = (1 - beta) * r["sr_loss"] + beta * r["segment_loss"]
        e = abs(loss - float(g["loss"][step])) / abs(float(g["loss"][step]))
        print(f"step {step}: loss {loss:.6f} (ref {float(g['loss'][step]):.6f}, rel {e:.1e})  alpha {r['boundary_alpha']}")
        assert e < 2e-3, (step, e)
        assert abs(r["boundary_alpha"] - float(g["alpha"][step])) < 1e-12 and alphas[step] == r["boundary_alpha"]
        assert r["overflow_steps"] == 0 and r["lr"] == float(g["lr_rate"])
        assert r["total"] == r["sr_loss"] + beta * r["segment_loss"]
    sd, sd_ref = m.state_dict(), ref.state_dict()
    for name, t in sd.items():
        assert torch.equal(t, sd_ref[name]), name
    trained = 0
    for p, q in zip(opt2.param_groups[0]["params"], opt.param_groups[0]["params"]):
        assert float(opt2.state[p]["step"]) == float(opt.state[q]["step"]) == steps and torch.equal(opt2.state[p]["exp_avg"], opt.state[q]["exp_avg"])
        trained += int(float(opt2.state[p]["exp_avg_sq"].max()) > 0)
    assert trained > 250                                       # (both did train: the equality above is not that of two idle models)


# ----------------------------------------------------------------------------------------------------------------- 9 / 10: a small run
def _pool():
    """five uint8 image / mask pairs of 64 .. 80 px: smooth images with a crack-like stroke each"""
    from csbsr_amd.data.resident import ResidentDataset
    rng = np.random.default_rng(7)
    images, masks = [], []
    for H, W in ((64, 80), (72, 64), (80, 80), (66, 71), (75, 68)):
        yy, xx = np.mgrid[0:H, 0:W]
        base = 128 + 60 * np.sin(xx / rng.uniform(4, 9) + rng.uniform(0, 3)) * np.cos(yy / rng.uniform(4, 9))
        img = np.clip(base[:, :, None] + rng.normal(0, 12, size=(H, W, 3)), 0, 255).astype(np.uint8)
        m = np.zeros((H, W), np.uint8)
        c = (xx * rng.uniform(0.3, 0.9) + rng.uniform(5, 25)).astype(int)
        m[np.abs(yy - c) < 2] = 255
        img[m > 0] //= 3
        images.append(img)
        masks.append(m)
    return ResidentDataset(images, masks, device=DEV)


def _small_cfg(optimizer="Adam"):
    from csbsr_amd.config import cfg as base_cfg
    cfg = base_cfg.clone()
    cfg.MODEL.SCALE_FACTOR, cfg.MODEL.DETECTOR_TYPE, cfg.MODEL.OPTIMIZER = 4, "PSPNet", optimizer
    cfg.SOLVER.BATCH_SIZE = 2
    cfg.SOLVER.SR_PRETRAIN_ITER = [1, 39999]          # the run below (40001 ..) is in the joint phase, two iterations after it began
    return cfg


def _small_model(cfg, resume_iter):
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    m = JointModelWithLoss(cfg, 5, resume_iter, None, device=DEV)
    deterministic_fill(m.state_dict(), "contractive")
    assert m.dropout_enabled and m.dropout_masks is None
    return m


@pytest.mark.parametrize("optimizer", ["Adam", "SGD"])
def test_resumed_run_is_the_uninterrupted_run(optimizer, tmp_path):
    """Four iterations in one go against two iterations, a checkpoint, NEW model / optimiser / loader objects, ``resume`` and two more:
    parameters, BatchNorm buffers, optimiser state and the four logged loss pairs are bit-identical.  Dropout draws from the device's
    generator and the loader from its own: both are scrambled before the resume, so equality means they came back from the file."""
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader
    cfg = _small_cfg(optimizer)
    ds = _pool()
    # drop_last: every training batch holds two images (train-mode BatchNorm over the 1 x 1 pyramid bin needs more than one value per
    # channel), so an epoch is two batches of the five images and the third iteration opens a new permutation -- after the resume
    loader = lambda n, seed: DeviceTrainLoader(ds, 64, 4, batch_size=2, num_iterations=n, seed=seed, drop_last=True)
    it0 = 40000

    def run(model, opt, ld, resume_iter, out=None):
        logs = []
        T.do_train(cfg, model, opt, T.build_scheduler(cfg, opt, resume_iter), ld, resume_iter=resume_iter, log_step=1, save_step=2,
                   output_dir=out, log=logs.append)
        return [(r["iteration"], r["segment_loss"], r["sr_loss"], r["boundary_alpha"]) for r in logs if "segment_loss" in r]
    torch.manual_seed(5)
    full = _small_model(cfg, it0)
    opt_full = T.build_optimizer(cfg, full)
    logs_full = run(full, opt_full, loader(4, 31), it0)
    assert [r[0] for r in logs_full] == [40001, 40002, 40003, 40004] and len({r[3] for r in logs_full}) == 2      # alpha stepped inside the run

    torch.manual_seed(5)
    first = _small_model(cfg, it0)
    logs_a = run(first, T.build_optimizer(cfg, first), loader(2, 31), it0, str(tmp_path))
    for kind in ("model", "optimizer", "trainer"):
        assert (tmp_path / kind / "iteration_40002.pth").is_file()
    del first
    torch.manual_seed(777)                                     # not the state the run stopped in
    torch.rand(3, device=DEV)
    second = _small_model(cfg, 0)                              # (alpha and its counter come from the file, not from this constructor)
    opt_second = T.build_optimizer(cfg, second)
    ld = loader(4, 999)
    it = T.resume(cfg, str(tmp_path), 40002, second, opt_second, ld)
    assert it == 40002
    logs_b = run(second, opt_second, ld, it)
    assert logs_a + logs_b == logs_full
    sd, sd_full = second.state_dict(), full.state_dict()
    assert any(k.endswith("running_mean") for k in sd)
    for name, t in sd.items():
        assert torch.equal(t, sd_full[name]), name
    n_state = 0
    for p, q in zip(opt_second.param_groups[0]["params"], opt_full.param_groups[0]["params"]):
        assert set(opt_second.state[p]) == set(opt_full.state[q])
        for key, v in opt_second.state[p].items():
            assert torch.equal(v.cpu(), opt_full.state[q][key].cpu()), key
            n_state += 1
    assert n_state >= 290
    if optimizer == "Adam":
        assert {float(s["step"]) for s in opt_second.state.values()} == {4.0}


def test_validate_equals_a_restatement_and_leaves_the_model_alone():
    from csbsr_amd import trainer as T
    from csbsr_amd.data.resident import DeviceTrainLoader
    from csbsr_amd.utils.estimate_metrics import PSNR, SSIM, IoU
    cfg = _small_cfg()
    ds = _pool()
    view = ds.subset([3, 1, 4, 0, 2])
    mk = lambda seed: DeviceTrainLoader(view, 64, 4, batch_size=2, seed=seed, shuffle=False)
    torch.manual_seed(5)
    m = _small_model(cfg, 40000)
    m.train()
    x, hr, mask, k, sdf = next(iter(mk(1)))
    seg_l, sr_l = m(40001, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, segment_sdf=sdf)[:2]
    T.calc_loss(seg_l, sr_l, 40001, cfg).backward()           # gradients and BatchNorm statistics exist before the validation
    before = {n: t.clone() for n, t in m.state_dict().items()}
    grads = [None if p.grad is None else p.grad.clone() for p in m.parameters()]
    assert sum(g is not None for g in grads) == 290
    m.iter_cnt = True
    loader = mk(123)
    got = T.validate(m, loader, 40001, seed=7)
    again = T.validate(m, loader, 40001, seed=7)
    assert got == again and (got["batches"], got["images"]) == (3, 5)
    assert m.training and m.iter_cnt is True
    for n, t in m.state_dict().items():
        assert torch.equal(t, before[n]), n
    for p, g0 in zip(m.parameters(), grads):
        assert (p.grad is None and g0 is None) or torch.equal(p.grad, g0)
    free_a, free_b = T.validate(m, loader, 40001), T.validate(m, loader, 40001)        # the reference's behaviour: fresh draws every pass
    assert free_a != free_b and free_a != got
    # the restatement: per-batch model calls, the metric classes, the reference's host bookkeeping
    psnr, ssim, iou = PSNR(), SSIM(), IoU()
    eval_seg = eval_sr = 0
    scores = {key: np.array([]) for key in ("psnr", "kernel_psnr", "ssim", "iou")}
    sizes = []
    m.eval()
    with torch.no_grad():
        for x, hr, mask, k, sdf in mk(7):
            seg_l, sr_l, seg, sr, kp = m(40001, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, segment_sdf=sdf)
            eval_seg += seg_l.mean().item()
            eval_sr += sr_l.mean().item()
            sr[sr > 1] = 1
            sr[sr < 0] = 0
            kp = kp.clone()
            kp[kp > 1] = 1
            kp[kp < 0] = 0
            scores["psnr"] = np.append(scores["psnr"], psnr(sr, hr))
            scores["kernel_psnr"] = np.append(scores["kernel_psnr"], psnr(kp, k))
            scores["ssim"] = np.append(scores["ssim"], ssim(sr, hr))
            scores["iou"] = np.append(scores["iou"], iou((seg >= 0.5).float(), mask))
            sizes.append(x.shape[0])
    m.train()
    assert sizes == [2, 2, 1]
    want = {"eval_segment_loss": eval_seg / 3, "eval_sr_loss": eval_sr / 3, **{key: sum(v) / len(v) for key, v in scores.items()}}
    print("validate:", got, "restated:", want)
    for key, v in want.items():
        assert got[key] == v, key
    assert np.isfinite(list(want.values())).all() and 0 <= want["iou"] <= 1 and want["psnr"] > 5
