"""The training loop on the HBM-resident path: the reference's ``model/engine/trainer.py`` for ``MODEL.JOINT_LEARNING=True`` (the only mode
the model classes build), restated so that it consumes ``DeviceTrainLoader`` batches and never makes the host wait for the device between
two log steps.

    model = JointModelWithLoss(cfg, len(train_view), resume_iter)
    optimizer = build_optimizer(cfg, model)
    resume_iter = resume(cfg, out, resume_iter, model, optimizer, train_loader)          # only when continuing a run
    scheduler = build_scheduler(cfg, optimizer, resume_iter)
    do_train(cfg, model, optimizer, scheduler, train_loader, eval_loader, resume_iter=resume_iter, output_dir=out)

What is kept from the reference, quirks included: the order of an iteration (trainer.py:57-72), the loss mixing and its pretraining windows
(:406-438; the SEG window is applied after the SR window and wins), the task-weight ramp that is capped at 1 and NOT floored at 0 (:455-464),
the alpha phase (:495-508), the logged total ``sr + TASK_LOSS_WEIGHT * seg`` (:84, not the mixed training loss), the two checkpoint files and
their names (:117-131), validation with ``iter_cnt`` off (:133-250), its losses averaged over BATCHES and its metrics over IMAGES.

What differs, on purpose: the running loss sums stay on the device (fp64, the reference's Python-float sums) and are read back once per
``log_step`` -- the reference's two ``.item()`` per step make the host wait for every step; no W&B; a third checkpoint file carries what an exact
continuation needs (``resume``); ``resume`` also loads the optimiser file, which the reference writes and never reads.

Out of scope: data-parallel wiring (``GradBucketReducer`` still works in a caller's own loop), the first-batch PNG dumps of trainer.py:186-227,
``do_pretrain_sr`` / ``SRModelWithLoss``, and every cfg value the model constructors refuse (they keep raising there).
"""
import datetime
import os
import time

import torch
from torch.optim.lr_scheduler import LambdaLR

from .utils.lr_scheduler import UpDownScheduler
from .utils.misc import fix_model_state_dict


# ------------------------------------------------------------------------------------------------------------------ loss mixing
def increase_w_task(cfg, iteration):
    """The segmentation weight under ``TASK_LOSS_WEIGHT == -1``: a line from 0 at INCRESE_TASK_W_ITER[0] to 1 at INCRESE_TASK_W_ITER[1], capped
    at 1 and (the reference's quirk) negative before the start."""
    start, end = cfg.SOLVER.INCRESE_TASK_W_ITER
    return min(1.0 / (end - start) * (iteration - start), 1)


def calc_pretrain_loss(loss, segment_loss, sr_loss, iteration, cfg):
    """The pretraining windows: SR loss alone inside SR_PRETRAIN_ITER, then -- applied second, so it wins where the two overlap -- the
    segmentation loss alone inside SEG_PRETRAIN_ITER."""
    if cfg.SOLVER.SR_PRETRAIN_ITER[0] <= iteration < cfg.SOLVER.SR_PRETRAIN_ITER[1]:
        loss = sr_loss
    if cfg.SOLVER.SEG_PRETRAIN_ITER[0] <= iteration < cfg.SOLVER.SEG_PRETRAIN_ITER[1]:
        loss = segment_loss
    return loss


def _mix(seg, sr, iteration, cfg):
    """the scalar training loss from the two batch means (device scalars; nothing here reads them)"""
    w = increase_w_task(cfg, iteration) if cfg.SOLVER.TASK_LOSS_WEIGHT == -1 else cfg.SOLVER.TASK_LOSS_WEIGHT
    return calc_pretrain_loss((1 - w) * sr + w * seg, seg, sr, iteration, cfg)


def calc_loss(segment_loss, sr_loss, iteration, cfg):
    """Per-sample loss vectors -> the scalar that is back-propagated.  A loss vector the scalar does not use gets no gradient, which is how
    the model's backward knows that a pretraining phase skips one half."""
    return _mix(segment_loss.mean(), sr_loss.mean(), iteration, cfg)


def set_alpha_phase(cfg, model, iteration):
    """The boundary-loss alpha of this iteration: frozen (and its epoch counter held at 1) inside SR_PRETRAIN_ITER, stepped outside."""
    if "Boundary" not in cfg.SOLVER.SEG_LOSS_FUNC:
        return
    fn = model.ss_loss_fn
    if cfg.SOLVER.SR_PRETRAIN_ITER[0] <= iteration < cfg.SOLVER.SR_PRETRAIN_ITER[1]:
        fn.fix_alpha, fn.iter = True, 1
    else:
        fn.fix_alpha = False
        fn.update_alpha()


# ------------------------------------------------------------------------------------------------------------------ optimiser, scheduler
def build_optimizer(cfg, model):
    """train.py:90-93 on the one-launch HIP optimisers."""
    from . import optim
    if cfg.MODEL.OPTIMIZER == "Adam":
        return optim.Adam(model.parameters(), lr=cfg.SOLVER.LR, betas=(0.9, 0.999), eps=1e-8)
    if cfg.MODEL.OPTIMIZER == "SGD":
        return optim.SGD([p for p in model.parameters() if p.requires_grad], lr=cfg.SOLVER.LR, momentum=0.9, weight_decay=5e-4)
    raise NotImplementedError(f"MODEL.OPTIMIZER={cfg.MODEL.OPTIMIZER!r}: 'Adam' or 'SGD'")


def build_scheduler(cfg, optimizer, resume_iter=0):
    """train.py:95-96.  Build it AFTER ``resume``: LambdaLR counts from 0 again and ``resume_iter`` is its offset."""
    return LambdaLR(optimizer, lr_lambda=UpDownScheduler(cfg.SOLVER.SR_PRETRAIN_ITER[1], resume_iter, cfg.SOLVER.SCHEDULER))


# ------------------------------------------------------------------------------------------------------------------ logging
def print_line(record):
    """The default ``log``: the reference's console lines (trainer.py:89, :131, :233-234)."""
    if "checkpoint" in record:
        print("=====> Save Checkpoint to {}".format(record["checkpoint"]))
    elif "eval_segment_loss" in record:
        print(f"\nestimation result (iter={record['iteration']}):")
        print(f"=====> Segment_Loss({record['seg_loss_func']}): {record['eval_segment_loss']:.6f}, SR_Loss({record['sr_loss_func']}): "
              f"{record['eval_sr_loss']:.6f} PSNR:{record['psnr']:.4f} SSIM:{record['ssim']:.4f}  PSNR(Kernel):{record['kernel_psnr']:.4f} "
              f"IoU:{record['iou']:.4f}")
    else:
        print("===> Iter: {:07d}, LR: {:.5f}, Cost: {:.2f}s, Eta: {}, Segment_Loss({}): {:.6f}, SR_Loss({}): {:.6f}".format(
            record["iteration"], record["lr"], record["cost_s"], record["eta"], record["seg_loss_func"], record["segment_loss"],
            record["sr_loss_func"], record["sr_loss"]))


def _hook(hooks, name):
    if hooks is None:
        return None
    return hooks.get(name) if isinstance(hooks, dict) else getattr(hooks, name, None)


def _device_of(model):
    dev = getattr(model, "_device", None)
    if dev is None:
        dev = next(model.parameters()).device
    return torch.device(dev)


# ------------------------------------------------------------------------------------------------------------------ validation
class ValidationAccumulator:
    """The bookkeeping of one validation pass (trainer.py:142-149, 160-183, 230-234).  ``add`` takes one batch: its two per-sample loss
    vectors and its four per-sample metric vectors, on any device, and keeps them there; ``result`` reads everything back at once.

    The losses are means over BATCHES of the batch means (a short last batch weighs as much as a full one); the metrics are means over
    IMAGES.  The host arithmetic is the reference's: fp64 running sums in order of arrival."""

    METRICS = ("psnr", "ssim", "kernel_psnr", "iou")

    def __init__(self):
        self.losses, self.metrics = [], {k: [] for k in self.METRICS}

    def add(self, segment_loss, sr_loss, psnr, ssim, kernel_psnr, iou):
        self.losses.append(torch.stack([torch.as_tensor(segment_loss).float().mean(), torch.as_tensor(sr_loss).float().mean()]))
        for k, v in zip(self.METRICS, (psnr, ssim, kernel_psnr, iou)):
            self.metrics[k].append(torch.as_tensor(v).float().reshape(-1))

    def result(self):
        if not self.losses:
            raise ValueError("validation saw no batch")
        nb = len(self.losses)
        n = int(sum(v.numel() for v in self.metrics["psnr"]))
        flat = torch.cat([torch.stack(self.losses).reshape(-1)] + [torch.cat(self.metrics[k]) for k in self.METRICS]).cpu().double().tolist()
        losses, rest = flat[:2 * nb], flat[2 * nb:]
        out = {"eval_segment_loss": sum(losses[0::2]) / nb, "eval_sr_loss": sum(losses[1::2]) / nb}
        for i, k in enumerate(self.METRICS):
            out[k] = sum(rest[i * n:(i + 1) * n]) / n
        out["batches"], out["images"] = nb, n
        return out


def validate(model, loader, iteration, *, seed=None):
    """One pass over ``loader`` (batches of ``(x, hr, mask, k[, sdf])``) with the model in ``eval()`` under ``no_grad``: validation
    segmentation and SR loss, PSNR, SSIM, kernel PSNR and IoU at 0.5 (trainer.py:140-235).  The SR image and the kernel are clamped to
    [0, 1] before their metrics; the segmentation map is binarised with ``>= 0.5`` first (``iou_sweep`` alone compares with ``>``).

    ``seed``: when not None the loader's generator is re-seeded with it first, so successive validations see the same crops and blurs and
    are comparable; None is the reference's behaviour, fresh draws in every pass.  The model's mode is restored; ``iter_cnt`` is not touched
    (``do_train`` switches it off around the call, as the reference does)."""
    from .utils.estimate_metrics import iou_sweep, psnr_ssim
    if seed is not None:
        loader.gen.manual_seed(int(seed))
    was_training = model.training
    acc = ValidationAccumulator()
    model.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                x, hr, mask, k = batch[:4]
                extra = {"segment_sdf": batch[4]} if len(batch) > 4 else {}
                seg_l, sr_l, seg, sr, kp = model(iteration, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, **extra)
                ps, ss = psnr_ssim(sr.clamp(0, 1), hr)
                kps, _ = psnr_ssim(kp.clamp(0, 1), k)
                iou = iou_sweep((seg >= 0.5).float(), mask, [0.5])
                acc.add(seg_l, sr_l, ps, ss, kps, iou)
    finally:
        model.train(was_training)
    return acc.result()


# ------------------------------------------------------------------------------------------------------------------ checkpoints
def _paths(output_dir, iteration):
    return {kind: os.path.join(output_dir, kind, f"iteration_{iteration}.pth") for kind in ("model", "optimizer", "trainer")}


def _trainer_state(model, train_loader, iteration, sums, overflowed):
    dev = _device_of(model)
    fn = getattr(model, "ss_loss_fn", None)
    return {
        "iteration": int(iteration),
        "ss_loss_fn": None if fn is None else {"alpha": fn.alpha, "iter": fn.iter, "fix_alpha": fn.fix_alpha},
        "loader": train_loader.state_dict() if hasattr(train_loader, "state_dict") else None,
        "cuda_rng": torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None,          # Dropout2d's masks are drawn from it
        "cpu_rng": torch.get_rng_state(),
        "loss_scale": {k: getattr(model, k) for k in ("grad_scale", "scale_backoff", "overflow_steps") if hasattr(model, k)},
        "logging": {"sums": sums.detach().cpu(), "overflowed": int(overflowed)},
    }


def save_checkpoint(output_dir, iteration, model, optimizer, train_loader=None, sums=None, overflowed=0):
    """``model/``, ``optimizer/`` (the reference's two files: plain state_dicts, loadable there and by torch.optim.Adam / SGD) and
    ``trainer/iteration_N.pth`` (everything else ``resume`` needs to continue exactly).  Returns the three paths."""
    paths = _paths(output_dir, iteration)
    for p in paths.values():
        os.makedirs(os.path.dirname(p), exist_ok=True)
    torch.save(model.state_dict(), paths["model"])
    torch.save(optimizer.state_dict(), paths["optimizer"])
    sums = torch.zeros(2, dtype=torch.float64) if sums is None else sums
    torch.save(_trainer_state(model, train_loader, iteration, sums, overflowed), paths["trainer"])
    return paths


def resume(cfg, output_dir, iteration, model, optimizer, train_loader):
    """Load the checkpoint of ``iteration`` into freshly built objects and return the ``resume_iter`` to hand to ``build_scheduler`` and
    ``do_train``.  Build the model with ``resume_iter=iteration`` (its alpha then starts where the reference's would).

    With ``trainer/iteration_N.pth`` present the continued run IS the uninterrupted run: alpha and its counter, the loader's generator,
    permutation and cursor, the device's and the host's generator state, the loss-scale back-off and the logging sums are restored.  With
    only the reference's files the reference's semantics hold: weights through ``fix_model_state_dict`` with ``strict=False``, alpha from
    the model's constructor, a loader that starts over.  The optimiser file is loaded when it exists (the reference writes it and never
    reads it back)."""
    paths = _paths(output_dir, iteration)
    sd = fix_model_state_dict(torch.load(paths["model"], map_location="cpu"))
    model.load_state_dict(sd, strict=False)
    if hasattr(model, "_runtime"):
        model._runtime()          # parameters move to the device here: the optimiser's state must follow them, not stay on the host
    if os.path.isfile(paths["optimizer"]):
        optimizer.load_state_dict(torch.load(paths["optimizer"], map_location="cpu"))
    if not os.path.isfile(paths["trainer"]):
        return int(iteration)
    st = torch.load(paths["trainer"], map_location="cpu")
    if int(st["iteration"]) != int(iteration):
        raise ValueError(f"{paths['trainer']} holds iteration {st['iteration']}, not {iteration}")
    if st["ss_loss_fn"] is not None:
        for k, v in st["ss_loss_fn"].items():
            setattr(model.ss_loss_fn, k, v)
    if st["loader"] is not None and hasattr(train_loader, "load_state_dict"):
        train_loader.load_state_dict(st["loader"])
    dev = _device_of(model)
    if st["cuda_rng"] is not None and dev.type == "cuda":
        torch.cuda.set_rng_state(st["cuda_rng"], dev)
    torch.set_rng_state(st["cpu_rng"])
    for k, v in st["loss_scale"].items():
        setattr(model, k, v)
    model._resume_logging = (int(iteration), st["logging"])          # picked up (once) by do_train(resume_iter=iteration)
    return int(iteration)


# ------------------------------------------------------------------------------------------------------------------ the loop
def do_train(cfg, model, optimizer, scheduler, train_loader, eval_loader=None, *, resume_iter=0, log_step=50, save_step=2000, eval_step=2000,
             output_dir=None, log=print_line, hooks=None):
    """Train over ``train_loader`` (any iterable of ``(x, hr, mask, k)`` or ``(x, hr, mask, k, sdf)``), iterations counted from
    ``resume_iter + 1``.  Per iteration: set_alpha_phase, model.train(), zero_grad, forward, calc_loss, backward, optimizer.step(),
    scheduler.step().  ``hooks`` (a dict or an object) may carry ``before_step(iteration, model)``, called first in an iteration, and
    ``after_step(iteration, model, record)``, called last with that iteration's log record or None.

    Every ``log_step`` iterations ``log`` receives {iteration, lr, segment_loss, sr_loss, total, boundary_alpha, overflow_steps, ...}: the
    losses are window means, ``total`` is ``sr + TASK_LOSS_WEIGHT * seg``, ``overflow_steps`` counts the steps skipped so far because the
    fp16 backward overflowed (``model.last_step_overflowed``, a host flag).  That is the loop's only read-back of device values.  Every
    ``save_step`` iterations the three checkpoint files are written under ``output_dir`` (None: no checkpoints); every ``eval_step``
    iterations, with an ``eval_loader``, ``validate`` runs with ``model.iter_cnt`` off and its result goes to ``log``."""
    before, after = _hook(hooks, "before_step"), _hook(hooks, "after_step")
    names = {"seg_loss_func": cfg.SOLVER.SEG_LOSS_FUNC, "sr_loss_func": cfg.SOLVER.SR_LOSS_FUNC}
    sums, overflowed = None, 0
    carried = model.__dict__.pop("_resume_logging", None)
    if carried is not None and carried[0] == resume_iter:
        sums, overflowed = carried[1]["sums"].to(torch.float64), int(carried[1]["overflowed"])
    try:
        max_iter = len(train_loader) + resume_iter - int(getattr(train_loader, "produced", 0))
    except TypeError:
        max_iter = None
    trained_time, tic, end = 0.0, time.time(), time.time()
    for iteration, batch in enumerate(train_loader, resume_iter + 1):
        if before is not None:
            before(iteration, model)
        set_alpha_phase(cfg, model, iteration)
        model.train()
        optimizer.zero_grad()
        x, hr, mask, k = batch[:4]
        extra = {"segment_sdf": batch[4]} if len(batch) > 4 else {}
        segment_loss, sr_loss = model(iteration, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, **extra)[:2]
        seg, sr = segment_loss.mean(), sr_loss.mean()
        loss = _mix(seg, sr, iteration, cfg)
        loss.backward()
        optimizer.step()
        scheduler.step()
        step_sums = torch.stack([seg.detach(), sr.detach()]).double()
        sums = step_sums if sums is None else sums.to(step_sums.device) + step_sums
        overflowed += bool(getattr(model, "last_step_overflowed", False))
        del loss, segment_loss, sr_loss, seg, sr, batch, x, hr, mask, k, extra
        trained_time += time.time() - end
        end = time.time()

        record = None
        if iteration % log_step == 0:
            seg_m, sr_m = (v / log_step for v in sums.tolist())          # the one read-back of the window
            eta = "?" if max_iter is None else str(datetime.timedelta(seconds=int(trained_time / (iteration - resume_iter)
                                                                                  * (max_iter - iteration))))
            fn = getattr(model, "ss_loss_fn", None)
            record = {"iteration": iteration, "lr": optimizer.param_groups[0]["lr"], "segment_loss": seg_m, "sr_loss": sr_m,
                      "total": sr_m + cfg.SOLVER.TASK_LOSS_WEIGHT * seg_m,
                      "boundary_alpha": fn.alpha if fn is not None and "Boundary" in cfg.SOLVER.SEG_LOSS_FUNC else None,
                      "overflow_steps": overflowed, "cost_s": time.time() - tic, "eta": eta, **names}
            log(record)
            sums = None
            tic = time.time()

        if output_dir is not None and iteration % save_step == 0:
            paths = save_checkpoint(output_dir, iteration, model, optimizer, train_loader, sums, overflowed)
            log({"iteration": iteration, "checkpoint": paths["model"], **paths})

        if eval_loader is not None and iteration % eval_step == 0:
            model.iter_cnt = False
            try:
                result = validate(model, eval_loader, iteration)
            finally:
                model.iter_cnt = True
            log({"iteration": iteration, **result, **names})

        if after is not None:
            after(iteration, model, record)
