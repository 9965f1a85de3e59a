"""Host side of the training driver (csbsr_amd/trainer.py), of the loader's sequential order and resumable state
(csbsr_amd/data/resident.py) and of csbsr_amd.optim.SGD.  No GPU: the loop runs over a stub nn.Module that has the model's surface."""
import os

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import LambdaLR

from golden_utils import load_golden
import resident_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    from csbsr_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import subprocess
        subprocess.run(["make", "-C", os.path.join(ROOT, "csbsr_amd", "csrc"), "-j8"], check=True)
    from csbsr_amd import trainer
    return trainer


def _cfg(**solver):
    from csbsr_amd.config import cfg
    c = cfg.clone()
    for k, v in solver.items():
        c.SOLVER[k] = v
    return c


# ----------------------------------------------------------------------------------------------------------------- 1. calc_loss
def test_calc_loss_fixed_weight_equals_the_oracle(T):
    from oracle import csbsr_oracle as O
    g = torch.Generator().manual_seed(3)
    seg, sr = torch.rand(6, generator=g) * 2, torch.rand(6, generator=g)
    cfg = _cfg()
    assert cfg.SOLVER.INCRESE_TASK_W_ITER == [30000, 170000]
    pc = O.PathCfg()
    assert pc.beta == cfg.SOLVER.TASK_LOSS_WEIGHT and list(pc.joint_pretrain) == cfg.SOLVER.SR_PRETRAIN_ITER
    for it in (1, 17, 30000, 30001, 40000, 299999):
        assert torch.equal(T.calc_loss(seg, sr, it, cfg), O.calc_loss(seg, sr, it, pc)), it
    assert torch.equal(T.calc_loss(seg, sr, 30000, cfg), sr.mean()) and not torch.equal(T.calc_loss(seg, sr, 30001, cfg), sr.mean())


def test_calc_loss_ramp_is_capped_at_one_and_not_floored(T):
    cfg = _cfg(TASK_LOSS_WEIGHT=-1, SR_PRETRAIN_ITER=[0, 0])
    a, b = cfg.SOLVER.INCRESE_TASK_W_ITER
    seg, sr = torch.tensor([3.0, 5.0]), torch.tensor([0.5, 1.5])
    assert T.increase_w_task(cfg, a) == 0 and T.increase_w_task(cfg, (a + b) // 2) == 0.5
    assert T.increase_w_task(cfg, b) == 1 and T.increase_w_task(cfg, b + 12345) == 1
    assert T.increase_w_task(cfg, a - 7000) == pytest.approx(-0.05, abs=1e-15)          # the quirk: no floor at 0
    for it in (a, (a + b) // 2, b + 12345, a - 7000):
        w = min((1 - 0) / (b - a) * (it - a), 1)
        assert torch.equal(T.calc_loss(seg, sr, it, cfg), (1 - w) * sr.mean() + w * seg.mean()), it
    assert torch.equal(T.calc_loss(seg, sr, b + 1, cfg), seg.mean())
    assert float(T.calc_loss(seg, sr, a - 7000, cfg)) == pytest.approx(1.05 * 1.0 - 0.05 * 4.0)


def test_seg_pretrain_window_wins_over_the_sr_window(T):
    cfg = _cfg(SR_PRETRAIN_ITER=[1, 101], SEG_PRETRAIN_ITER=[50, 151])
    seg, sr = torch.tensor([3.0, 5.0]), torch.tensor([0.5, 1.5])
    assert torch.equal(T.calc_loss(seg, sr, 49, cfg), sr.mean())
    assert torch.equal(T.calc_loss(seg, sr, 50, cfg), seg.mean()) and torch.equal(T.calc_loss(seg, sr, 100, cfg), seg.mean())
    assert torch.equal(T.calc_loss(seg, sr, 150, cfg), seg.mean())
    assert torch.equal(T.calc_loss(seg, sr, 151, cfg), 0.7 * sr.mean() + 0.3 * seg.mean())
    assert torch.equal(T.calc_pretrain_loss(torch.tensor(9.0), seg.mean(), sr.mean(), 75, cfg), seg.mean())


def test_calc_loss_keeps_the_graph_and_reads_nothing_back(T):
    """the scalar is a function of the loss vectors on their device; the half a pretraining window drops gets no gradient"""
    cfg = _cfg()
    seg, sr = torch.ones(4, requires_grad=True), torch.ones(4, requires_grad=True)
    T.calc_loss(seg, sr, 5, cfg).backward()
    assert seg.grad is None and torch.equal(sr.grad, torch.full((4,), 0.25))
    seg2, sr2 = torch.ones(4, device="meta"), torch.ones(4, device="meta")          # any read-back of a meta tensor raises
    assert T.calc_loss(seg2, sr2, 40000, cfg).device.type == "meta"
    assert T.calc_loss(seg2, sr2, 40000, _cfg(TASK_LOSS_WEIGHT=-1)).device.type == "meta"


# ----------------------------------------------------------------------------------------------------------------- 2. alpha schedule
def test_alpha_schedule_reproduces_the_trajectory_fixture(T):
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    g = load_golden("traj_pspnet_it40000")
    cfg = _cfg(BATCH_SIZE=6)
    cfg.MODEL.SCALE_FACTOR, cfg.MODEL.DETECTOR_TYPE = int(g["scale"]), str(g["detector"])
    m = JointModelWithLoss(cfg, 1000, 0, None)
    it0, steps = int(g["it0"]), int(g["steps"])
    assert (it0, steps) == (40000, 12)
    got = []
    for it in range(it0, it0 + steps):
        T.set_alpha_phase(cfg, m, it)
        assert m.ss_loss_fn.fix_alpha is False
        got.append(m.ss_loss_fn.alpha)
    assert got == [float(a) for a in g["alpha"]]
    before = (m.ss_loss_fn.alpha, )
    for it in (1, 2, 30000):          # inside SR_PRETRAIN_ITER: frozen, counter held at 1
        m.ss_loss_fn.iter = 77
        T.set_alpha_phase(cfg, m, it)
        assert m.ss_loss_fn.fix_alpha is True and m.ss_loss_fn.iter == 1 and (m.ss_loss_fn.alpha, ) == before
    T.set_alpha_phase(cfg, m, 30001)
    assert m.ss_loss_fn.fix_alpha is False and m.ss_loss_fn.iter == 2


# ----------------------------------------------------------------------------------------------------------------- 3. loop mechanics
class _Alpha:
    def __init__(self, calls):
        self.alpha, self.iter, self.fix_alpha, self.calls = 1.0, 0, False, calls

    def update_alpha(self):
        self.calls.append("alpha")
        self.alpha -= 0.01


class _Stub(torch.nn.Module):
    """the surface do_train / validate touch: forward's signature and five outputs, ss_loss_fn, iter_cnt, last_step_overflowed"""

    def __init__(self, calls=None):
        super().__init__()
        self.calls = [] if calls is None else calls
        self.w = torch.nn.Parameter(torch.tensor([0.5, -0.25]))
        self.ss_loss_fn = _Alpha(self.calls)
        self.iter_cnt, self.last_step_overflowed = True, False
        self.seen = []

    def train(self, mode=True):
        self.calls.append("train" if mode else "eval")
        return super().train(mode)

    def forward(self, iter, x, sr_targets=None, segment_targets=None, kernel_targets=None, segment_sdf=None):
        self.calls.append("forward")
        self.seen.append((iter, self.training, self.iter_cnt, segment_sdf is not None, torch.is_grad_enabled()))
        seg_loss = (x.mean((1, 2, 3)) * self.w[0]) ** 2 + 1
        sr_loss = (sr_targets.mean((1, 2, 3)) - self.w[1]) ** 2
        return seg_loss, sr_loss, segment_targets * 0 + 0.5, sr_targets + 0.25, kernel_targets * 2


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


class _Sched(LambdaLR):
    def step(self, *a, **kw):
        if getattr(self, "calls", None) is not None:
            self.calls.append("sched")
        return super().step(*a, **kw)


def _batches(n, B=2, sdf=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        b = (torch.rand(B, 3, 4, 4, generator=g), torch.rand(B, 3, 8, 8, generator=g), (torch.rand(B, 1, 8, 8, generator=g) > 0.5).float(),
             torch.rand(B, 1, 5, 5, generator=g))
        out.append(b + (torch.rand(B, 1, 8, 8, generator=g), ) if sdf else b)
    return out


def _run(T, cfg, n, tmp_path=None, resume_iter=0, model=None, eval_batches=None, **kw):
    calls = []
    m = _Stub(calls) if model is None else model
    calls = m.calls
    opt = _Opt(calls, m.parameters(), lr=cfg.SOLVER.LR)
    from csbsr_amd.utils.lr_scheduler import UpDownScheduler
    sched = _Sched(opt, lr_lambda=UpDownScheduler(cfg.SOLVER.SR_PRETRAIN_ITER[1], resume_iter, cfg.SOLVER.SCHEDULER))
    sched.calls = calls
    logs = []
    T.do_train(cfg, m, opt, sched, _batches(n, sdf=kw.pop("sdf", False)), eval_batches, resume_iter=resume_iter, log=logs.append,
               output_dir=None if tmp_path is None else str(tmp_path), **kw)
    return m, opt, logs, calls


def test_loop_order_within_an_iteration(T):
    cfg = _cfg(SR_PRETRAIN_ITER=[0, 0])
    marks = []
    hooks = {"before_step": lambda it, model: model.calls.append(f"before{it}"),
             "after_step": lambda it, model, record: marks.append((it, None if record is None else record["iteration"]))}
    m, opt, logs, calls = _run(T, cfg, 3, log_step=2, hooks=hooks, resume_iter=10)
    per_iter = ["alpha", "train", "zero_grad", "forward", "step", "sched"]
    assert calls == ["before11"] + per_iter + ["before12"] + per_iter + ["before13"] + per_iter
    assert [s[0] for s in m.seen] == [11, 12, 13] and all(s[1] and s[4] for s in m.seen)
    assert marks == [(11, None), (12, 12), (13, None)]
    assert [r["iteration"] for r in logs] == [12]


def test_backward_runs_between_forward_and_step(T):
    cfg = _cfg(SR_PRETRAIN_ITER=[0, 0])
    m = _Stub()
    m.w.register_hook(lambda g: m.calls.append("backward"))
    _run(T, cfg, 1, model=m, log_step=1)
    assert m.calls == ["alpha", "train", "zero_grad", "forward", "backward", "step", "sched"]


def test_fifth_batch_element_is_the_sdf(T):
    cfg = _cfg()
    m, *_ = _run(T, cfg, 2, sdf=True)
    assert [s[3] for s in m.seen] == [True, True]
    m, *_ = _run(T, cfg, 2, sdf=False)
    assert [s[3] for s in m.seen] == [False, False]


@pytest.fixture
def host_metrics(monkeypatch):
    """validate() computes its metrics with the device kernels; over the CPU stub they are replaced by plain torch stand-ins (what is
    tested here is the loop, the kernels have their own tests)"""
    from csbsr_amd.utils import estimate_metrics as EM

    def psnr_ssim(a, b):
        return 10 * torch.log10(1 / ((a - b) ** 2).mean((1, 2, 3))), torch.zeros(a.shape[0])

    def iou_sweep(p, m, thresholds, smooth=1e-5):
        o, t = p - thresholds[0] > 0, m > 0.5
        return ((o & t).sum((1, 2, 3)) + smooth) / ((o | t).sum((1, 2, 3)) + smooth).reshape(-1, 1)
    monkeypatch.setattr(EM, "psnr_ssim", psnr_ssim)
    monkeypatch.setattr(EM, "iou_sweep", iou_sweep)


def test_cadence_files_and_record_keys(T, tmp_path, host_metrics):
    cfg = _cfg(SR_PRETRAIN_ITER=[0, 0])
    ev = _batches(3, seed=5)
    m, opt, logs, calls = _run(T, cfg, 12, tmp_path, eval_batches=ev, log_step=2, save_step=3, eval_step=4)
    train_logs = [r for r in logs if "segment_loss" in r]
    saves = [r for r in logs if "checkpoint" in r]
    evals = [r for r in logs if "eval_segment_loss" in r]
    assert [r["iteration"] for r in train_logs] == [2, 4, 6, 8, 10, 12]
    assert [r["iteration"] for r in saves] == [3, 6, 9, 12]
    assert [r["iteration"] for r in evals] == [4, 8, 12]
    for r in train_logs:
        assert {"iteration", "lr", "segment_loss", "sr_loss", "total", "boundary_alpha", "overflow_steps"} <= set(r)
        assert r["total"] == r["sr_loss"] + cfg.SOLVER.TASK_LOSS_WEIGHT * r["segment_loss"] and r["overflow_steps"] == 0
    assert train_logs[-1]["boundary_alpha"] == m.ss_loss_fn.alpha == pytest.approx(1 - 0.12)
    for it in (3, 6, 9, 12):
        for kind in ("model", "optimizer", "trainer"):
            assert (tmp_path / kind / f"iteration_{it}.pth").is_file()
    assert sorted(os.listdir(tmp_path)) == ["model", "optimizer", "trainer"] and len(os.listdir(tmp_path / "model")) == 4
    # the reference's two files are plain state_dicts
    fresh = _Stub()
    fresh.load_state_dict(torch.load(tmp_path / "model" / "iteration_12.pth"))
    assert torch.equal(fresh.w, m.w) and not torch.equal(fresh.w, _Stub().w)
    o2 = torch.optim.Adam(fresh.parameters(), lr=1.0)
    o2.load_state_dict(torch.load(tmp_path / "optimizer" / "iteration_12.pth"))
    assert float(o2.state[fresh.w]["step"]) == 12 and torch.equal(o2.state[fresh.w]["exp_avg"], opt.state[m.w]["exp_avg"])
    st = torch.load(tmp_path / "trainer" / "iteration_9.pth")
    assert st["iteration"] == 9 and st["ss_loss_fn"]["alpha"] == pytest.approx(1 - 0.09) and st["cuda_rng"] is None
    assert st["logging"]["sums"].dtype == torch.float64 and float(st["logging"]["sums"].abs().sum()) > 0       # iteration 9 is mid-window
    assert float(torch.load(tmp_path / "trainer" / "iteration_12.pth")["logging"]["sums"].abs().sum()) == 0
    # validation: eval mode, no_grad, iter_cnt off; everything back on afterwards
    val = [s for s in m.seen if not s[1]]
    assert len(val) == 9 and all(s[2] is False and s[4] is False for s in val) and {s[0] for s in val} == {4, 8, 12}
    assert all(s[2] is True for s in m.seen if s[1])
    assert m.iter_cnt is True and m.training is True
    i = calls.index("eval")
    assert calls[i:i + 5] == ["eval", "forward", "forward", "forward", "train"]
    assert evals[0]["batches"] == 3 and evals[0]["images"] == 6


def test_logged_losses_are_window_means_in_fp64(T):
    cfg = _cfg(SR_PRETRAIN_ITER=[0, 0])
    m, opt, logs, _ = _run(T, cfg, 4, log_step=2)
    ref, ropt = _Stub(), None
    ropt = torch.optim.Adam(ref.parameters(), lr=cfg.SOLVER.LR)
    want, acc = [], [0.0, 0.0]
    for it, (x, hr, mask, k) in enumerate(_batches(4), 1):
        ropt.zero_grad()
        seg_l, sr_l = ref(it, x, hr, mask, k)[:2]
        T.calc_loss(seg_l, sr_l, it, cfg).backward()
        ropt.step()
        acc[0] += seg_l.mean().item()
        acc[1] += sr_l.mean().item()
        if it % 2 == 0:
            want.append((acc[0] / 2, acc[1] / 2))
            acc = [0.0, 0.0]
    assert [(r["segment_loss"], r["sr_loss"]) for r in logs] == want
    assert torch.equal(m.w, ref.w)


def test_overflowed_steps_are_counted_from_the_host_flag(T):
    cfg = _cfg()
    m = _Stub()
    m.last_step_overflowed = True
    _, _, logs, _ = _run(T, cfg, 4, model=m, log_step=2)
    assert [r["overflow_steps"] for r in logs] == [2, 4]


@pytest.mark.parametrize("resume_iter", [0, 6])
def test_lr_follows_lambda_lr_of_the_updown_scheduler(T, resume_iter):
    from csbsr_amd.utils.lr_scheduler import UpDownScheduler, BOOST_WINDOW, BOOST_FACTOR
    # the joint phase begins so that the boost window (open interval, counted from there) opens inside both runs: the rate printed at
    # iteration 9 (LambdaLR has stepped: it is the rate of iteration 10) is the first boosted one
    pre = 9 - BOOST_WINDOW[0]
    cfg = _cfg(SCHEDULER=True, SR_PRETRAIN_ITER=[pre - 5, pre])
    _, _, logs, _ = _run(T, cfg, 12 - resume_iter, resume_iter=resume_iter, log_step=1)
    w = torch.nn.Parameter(torch.zeros(1))
    o = torch.optim.SGD([w], lr=cfg.SOLVER.LR)
    s = LambdaLR(o, lr_lambda=UpDownScheduler(cfg.SOLVER.SR_PRETRAIN_ITER[1], resume_iter, True))
    want = []
    for it in range(resume_iter + 1, 13):
        o.step()
        s.step()
        want.append(o.param_groups[0]["lr"])
    assert [r["lr"] for r in logs] == want
    assert [r["iteration"] for r in logs] == list(range(resume_iter + 1, 13))
    base = cfg.SOLVER.LR
    assert want[0] == base and want[-1] == BOOST_FACTOR * base and want.count(base) == 8 - resume_iter


def test_build_optimizer_and_scheduler(T):
    from csbsr_amd import optim
    from csbsr_amd.utils.lr_scheduler import UpDownScheduler
    m = _Stub()
    frozen = torch.nn.Parameter(torch.zeros(3), requires_grad=False)
    m.frozen = frozen
    cfg = _cfg(LR=3e-5)
    o = T.build_optimizer(cfg, m)
    assert type(o) is optim.Adam and o.defaults == {"lr": 3e-5, "betas": (0.9, 0.999), "eps": 1e-8}
    assert len(o.param_groups[0]["params"]) == 2
    cfg.MODEL.OPTIMIZER = "SGD"
    o = T.build_optimizer(cfg, m)
    assert type(o) is optim.SGD and (o.defaults["lr"], o.defaults["momentum"], o.defaults["weight_decay"]) == (3e-5, 0.9, 5e-4)
    assert [p is m.w for p in o.param_groups[0]["params"]] == [True]
    cfg.MODEL.OPTIMIZER = "RMSprop"
    with pytest.raises(NotImplementedError):
        T.build_optimizer(cfg, m)
    cfg = _cfg(SCHEDULER=True, SR_PRETRAIN_ITER=[1, 777])
    s = T.build_scheduler(cfg, torch.optim.SGD([m.w], lr=1.0), 41)
    f = s.lr_lambdas[0]
    assert isinstance(s, LambdaLR) and isinstance(f, UpDownScheduler) and (f.pretrain_iter, f.resume_iter, f.scheduler_flag) == (777, 41, True)


def test_resume_with_the_references_two_files_only(T, tmp_path):
    """weights through fix_model_state_dict (a DataParallel prefix is stripped) with strict=False; alpha stays the constructor's; the
    returned iteration is the offset"""
    cfg = _cfg()
    src = _Stub()
    with torch.no_grad():
        src.w.copy_(torch.tensor([7.0, 8.0]))
    os.makedirs(tmp_path / "model")
    torch.save({"module.w": src.w.detach(), "module.extra": torch.zeros(1)}, tmp_path / "model" / "iteration_5.pth")
    m = _Stub()
    m.ss_loss_fn.alpha = 0.42
    opt = torch.optim.Adam(m.parameters(), lr=1.0)
    assert T.resume(cfg, str(tmp_path), 5, m, opt, None) == 5
    assert torch.equal(m.w, src.w) and m.ss_loss_fn.alpha == 0.42 and len(opt.state) == 0


def test_resume_continues_the_stub_run_exactly(T, tmp_path):
    cfg = _cfg(SR_PRETRAIN_ITER=[0, 0])
    full, _, logs_full, _ = _run(T, cfg, 6, log_step=4)
    _run(T, cfg, 3, tmp_path, log_step=4, save_step=3)
    m = _Stub()
    opt = _Opt(m.calls, m.parameters(), lr=cfg.SOLVER.LR)
    it = T.resume(cfg, str(tmp_path), 3, m, opt, None)
    assert m.ss_loss_fn.alpha == pytest.approx(0.97)
    logs = []
    T.do_train(cfg, m, opt, T.build_scheduler(cfg, opt, it), _batches(6)[3:], resume_iter=it, log_step=4, log=logs.append)
    assert torch.equal(m.w, full.w)
    assert [(r["iteration"], r["segment_loss"], r["sr_loss"]) for r in logs] == [(r["iteration"], r["segment_loss"], r["sr_loss"]) for r in logs_full]


# ----------------------------------------------------------------------------------------------------------------- 4. accumulator
def test_validation_accumulator_against_a_numpy_restatement(T):
    rng = np.random.default_rng(4)
    sizes = (2, 2, 1)
    batches = [{k: rng.random(b).astype(np.float32) * s for k, s in (("seg", 2.0), ("sr", 0.3), ("psnr", 40.0), ("ssim", 1.0), ("kpsnr", 50.0))}
               | {"iou": rng.random((b, 1)).astype(np.float32)} for b in sizes]
    acc = T.ValidationAccumulator()
    # the reference's bookkeeping: Python-float sums of the batch means, np.append of the per-sample metrics, sum / len at the end
    eval_seg = eval_sr = 0
    scores = {k: np.array([]) for k in ("psnr", "kpsnr", "ssim", "iou")}
    for b in batches:
        acc.add(torch.from_numpy(b["seg"]), torch.from_numpy(b["sr"]), torch.from_numpy(b["psnr"]), torch.from_numpy(b["ssim"]),
                torch.from_numpy(b["kpsnr"]), torch.from_numpy(b["iou"]))
        eval_seg += torch.from_numpy(b["seg"]).mean().item()
        eval_sr += torch.from_numpy(b["sr"]).mean().item()
        for k in scores:
            scores[k] = np.append(scores[k], b[k])
    got = acc.result()
    assert got["eval_segment_loss"] == eval_seg / 3 and got["eval_sr_loss"] == eval_sr / 3
    for k, name in (("psnr", "psnr"), ("kpsnr", "kernel_psnr"), ("ssim", "ssim"), ("iou", "iou")):
        assert len(scores[k]) == 5 and got[name] == sum(scores[k]) / len(scores[k]), name
    assert (got["batches"], got["images"]) == (3, 5)
    # the short batch is a third of the losses and a fifth of the metrics
    short = batches[2]
    assert got["eval_segment_loss"] == pytest.approx((batches[0]["seg"].mean() + batches[1]["seg"].mean() + short["seg"][0]) / 3, rel=1e-6)
    assert got["psnr"] == pytest.approx(np.concatenate([b["psnr"] for b in batches]).astype(np.float64).mean(), rel=1e-12)
    assert got["eval_segment_loss"] != pytest.approx(np.concatenate([b["seg"] for b in batches]).mean(), rel=1e-3)
    with pytest.raises(ValueError):
        T.ValidationAccumulator().result()


# ----------------------------------------------------------------------------------------------------------------- 5. loader
SIZES = [(40, 52), (31, 45), (24, 32), (50, 33), (37, 64)]


def _dataset(sizes=SIZES):
    from csbsr_amd.data import resident as R
    images, masks = RC.random_pairs(np.random.default_rng(0), sizes)
    return R, R.ResidentDataset(images, masks, device="cpu")


def _indices(loader):
    return [sel[:, 0].tolist() for sel, _ in loader.iter_decisions()]


def test_sequential_loader_order_sizes_and_single_pass(T):
    R, ds = _dataset()
    view = ds.subset([4, 0, 3, 1, 2])
    ld = R.DeviceTrainLoader(view, 16, 4, batch_size=2, seed=1, shuffle=False)
    assert _indices(ld) == [[4, 0], [3, 1], [2]] and len(ld) == 3
    assert _indices(ld) == [[4, 0], [3, 1], [2]]                                   # a second pass starts over: one pass each
    assert _indices(R.DeviceTrainLoader(view, 16, 4, batch_size=2, seed=1, shuffle=False, drop_last=True)) == [[4, 0], [3, 1]]
    assert _indices(R.DeviceTrainLoader(view, 16, 4, batch_size=2, seed=1, shuffle=False, shard=(1, 2))) == [[0, 1]]      # positions 1 and 3
    assert _indices(R.DeviceTrainLoader(view, 16, 4, batch_size=2, seed=1, shuffle=False, num_iterations=4)) == [[4, 0], [3, 1], [2], [4, 0]]
    # the crop, mirror and blur draws stay: they depend on the seed, the order does not
    a, b, c = (list(R.DeviceTrainLoader(view, 16, 4, batch_size=2, seed=s, shuffle=False).iter_decisions()) for s in (1, 1, 2))
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, b))
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(a, c)) and any(not torch.equal(x[1], y[1]) for x, y in zip(a, c))
    assert all(x[0][:, 0].tolist() == y[0][:, 0].tolist() for x, y in zip(a, c))
    assert sorted(sum(_indices(R.DeviceTrainLoader(view, 16, 4, batch_size=2, seed=1)), [])) == [0, 1, 2, 3, 4]          # default: shuffled, as before


def test_loader_state_round_trip_continues_bit_for_bit(T):
    R, ds = _dataset()
    mk = lambda: R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=9, num_iterations=7)
    whole = list(mk().iter_decisions())
    assert len(whole) == 7
    a = mk()
    it = a.iter_decisions()
    head = [next(it) for _ in range(3)]
    state = a.state_dict()
    assert state["produced"] == 3 and state["cursor"] == 5 and sorted(state["perm"].tolist()) == [0, 1, 2, 3, 4]
    import io
    buf = io.BytesIO()
    torch.save(state, buf)
    buf.seek(0)
    b = R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=12345, num_iterations=7)      # another seed: everything comes from the state
    b.load_state_dict(torch.load(buf))
    tail = list(b.iter_decisions())
    assert len(tail) == 4 and b.produced == 7
    for (s0, p0), (s1, p1) in zip(whole, head + tail):
        assert torch.equal(s0, s1) and torch.equal(p0, p1)
    sizes = [s.shape[0] for s, _ in whole]
    assert sizes == [2, 2, 1, 2, 2, 1, 2]                                               # epoch boundaries after batches 3 and 6: one among the tail
    assert len(list(b.iter_decisions())) == 7                                           # only the first iteration after a load continues
    # the original goes on unharmed, and a fresh loader is what it was
    assert all(torch.equal(x[0], y[0]) for x, y in zip(list(it), tail))
    # mid-epoch state too (cursor inside the permutation)
    c = mk()
    it = c.iter_decisions()
    next(it)
    d = mk()
    d.load_state_dict(c.state_dict())
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(list(d.iter_decisions()), whole[1:]))


def test_loader_state_at_the_end_of_the_single_pass_and_mismatch(T):
    R, ds = _dataset()
    a = R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=3, shuffle=False)
    it = a.iter_decisions()
    for _ in range(3):
        next(it)
    b = R.DeviceTrainLoader(ds, 16, 4, batch_size=2, seed=3, shuffle=False)
    b.load_state_dict(a.state_dict())
    assert list(b.iter_decisions()) == [] and list(it) == []
    with pytest.raises(ValueError):
        R.DeviceTrainLoader(ds.subset([0, 1, 2]), 16, 4, batch_size=2, seed=3).load_state_dict(a.state_dict())


# ----------------------------------------------------------------------------------------------------------------- 6. SGD host side
def test_sgd_refusals_state_keys_and_no_fallback(T):
    from csbsr_amd import _lib as L
    from csbsr_amd.optim import SGD
    p = torch.nn.Parameter(torch.zeros(5))
    for kw in ({"nesterov": True, "momentum": 0.9}, {"dampening": 0.1, "momentum": 0.9}, {"maximize": True}, {"lr": -1.0}, {"momentum": -0.5},
               {"weight_decay": -1e-4}):
        with pytest.raises(ValueError):
            SGD([p], **{"lr": 0.1, **kw})
    o = SGD([p], lr=0.1, momentum=0.9, weight_decay=5e-4)
    ref = torch.optim.SGD([p], lr=0.1, momentum=0.9, weight_decay=5e-4)
    assert set(ref.state_dict()["param_groups"][0]) <= set(o.state_dict()["param_groups"][0])       # torch.optim.SGD can step from our groups
    for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        assert o.param_groups[0][k] == ref.param_groups[0][k], k
    # torch's state key, through a state_dict loaded from torch.optim.SGD
    p.grad = torch.ones(5)
    ref.step()
    o.load_state_dict(ref.state_dict())
    assert set(o.state[p]) == {"momentum_buffer"} and torch.equal(o.state[p]["momentum_buffer"], ref.state[p]["momentum_buffer"])
    # host tensors: an error, never a torch step
    before = p.detach().clone()
    with pytest.raises(L.CsbsrHipError):
        o.step()
    with pytest.raises(L.CsbsrHipError):
        SGD([p], lr=0.1).step()
    assert torch.equal(p.detach(), before)
    p.grad = None
    o.step()                                   # torch's skip rule: nothing to do, nothing raised
    # a refused value that arrives through a state_dict is refused at the step
    sd = ref.state_dict()
    sd["param_groups"][0]["nesterov"] = True
    o.load_state_dict(sd)
    p.grad = torch.ones(5)
    with pytest.raises(ValueError):
        o.step()
