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

Data-parallel (one process per GPU, ``torch.distributed`` initialised with world > 1, or CSBSR_FORCE_DIST=1): ``do_train`` attaches the
``GradBucketReducer``, broadcasts rank 0's weights and checks with ``csbsr_amd.parallel.agree`` (a device fingerprint per tensor and a few KB
of all-reduce) that the replicas hold the same bits -- at the start and again before every checkpoint, which rank 0 alone writes.  Logged
losses and validation results are those of the GLOBAL batch.  With ``DeviceTrainLoader(shard_mode="batch")`` the run is the single-GPU run
with the same global batch, and its checkpoints continue on another number of GPUs (``resume``).

SR-only pretraining (the reference's ``DATASET.ONLY_IMAGES`` regime, train.py:70-74, 114-115 and trainer.py:252-402): ``do_pretrain_sr``
and ``validate_sr`` drive an ``SRModelWithLoss`` over an image-only ``DeviceTrainLoader`` (batches of ``(x, hr, k)``) with the same rules --
device-side fp64 window sum, one read-back per ``log_step``, the three checkpoint files, exact ``resume`` -- and ``export_pretrained_sr``
writes the file every ``MODEL.SR_SCRATCH = False`` model starts from.

    model = SRModelWithLoss(cfg)
    optimizer = build_optimizer(cfg, model)
    scheduler = build_scheduler(cfg, optimizer, resume_iter, scheduler_flag=False)       # train.py:74: constant rate in this regime
    do_pretrain_sr(cfg, model, optimizer, scheduler, train_loader, eval_loader, resume_iter=resume_iter, output_dir=out)
    export_pretrained_sr(model, cfg)

Out of scope: the first-batch PNG dumps of trainer.py:186-227 and :355-386, data-parallel SR pretraining (``do_pretrain_sr`` refuses it), and
every cfg value the model constructors refuse (they keep raising there).
"""
import collections
import datetime
import os
import time
import warnings

import torch
import torch.distributed as dist
from torch.optim.lr_scheduler import LambdaLR

from .parallel import agree
from .parallel.reducer import GradBucketReducer, broadcast_parameters, _forced
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


def _detector_only(cfg):
    """MODEL.SR == "bicubic" (trainer.py:414): the loss is the segmentation mean -- no pretraining window, no task weight, no SR loss"""
    return cfg.MODEL.SR == "bicubic"


def calc_loss(segment_loss, sr_loss, iteration, cfg):
    """Per-sample loss vectors -> the scalar that is back-propagated.  A loss vector the scalar does not use gets no gradient, which is how
    the model's backward knows that a pretraining phase skips one half.  With MODEL.SR == "bicubic" ``sr_loss`` may be None and the scalar
    is the segmentation mean at every iteration."""
    return _scalar(segment_loss.mean(), None if sr_loss is None else sr_loss.mean(), iteration, cfg)


def _scalar(seg, sr, iteration, cfg):
    """the rule of ``calc_loss`` on the two batch means (``sr`` may be None with MODEL.SR == "bicubic")"""
    return seg if _detector_only(cfg) else _mix(seg, sr, iteration, cfg)


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


def build_scheduler(cfg, optimizer, resume_iter=0, scheduler_flag=None):
    """train.py:95-96.  Build it AFTER ``resume``: LambdaLR counts from 0 again and ``resume_iter`` is its offset.  ``scheduler_flag``
    None takes ``SOLVER.SCHEDULER``; the SR-only regime passes False whatever the config says (train.py:74)."""
    flag = cfg.SOLVER.SCHEDULER if scheduler_flag is None else bool(scheduler_flag)
    return LambdaLR(optimizer, lr_lambda=UpDownScheduler(cfg.SOLVER.SR_PRETRAIN_ITER[1], resume_iter, flag))


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


# ------------------------------------------------------------------------------------------------------------------ data-parallel
def _dist(process_group=None):
    """(group, rank, world) when the data-parallel path is on -- torch.distributed initialised with more than one rank, or
    CSBSR_FORCE_DIST=1, the switch GradBucketReducer honours, which puts the real backend under the calls of a one-rank group -- else
    (None, 0, 1)."""
    if not (dist.is_available() and dist.is_initialized()):
        return None, 0, 1
    world = dist.get_world_size(process_group)
    if world == 1 and not _forced():
        return None, 0, 1
    return (dist.group.WORLD if process_group is None else process_group), dist.get_rank(process_group), world


def replica_tensors(model, optimizer=None, running_stats=True):
    """[(name, tensor)] of everything that must be the same on every replica: parameters and buffers (``state_dict()`` names) and, with an
    optimiser, its state tensors on the model's device (``optimizer.<group>.<index>.<key>``; host-side scalars such as Adam's ``step``
    follow from the common skip decision and are left out).  ``running_stats=False`` leaves out BatchNorm's ``running_mean`` /
    ``running_var``: once training has begun they are per replica BY DESIGN -- each replica normalises with, and averages, the statistics
    of its own shard, as the replicas of the reference's nn.DataParallel do, and rank 0's are the ones that are saved, as there."""
    dev = _device_of(model)
    out = [(k, v.detach()) for k, v in model.state_dict().items()
           if torch.is_tensor(v) and (running_stats or not k.endswith((".running_mean", ".running_var")))]
    if optimizer is not None:
        for gi, group in enumerate(optimizer.param_groups):
            for pi, p in enumerate(group["params"]):
                for key, v in optimizer.state.get(p, {}).items():
                    if torch.is_tensor(v) and v.device.type == dev.type and v.dim() > 0:
                        out.append((f"optimizer.{gi}.{pi}.{key}", v.detach()))
    return out


def _device_rng(dev):
    return torch.cuda.get_rng_state(dev) if dev.type == "cuda" else None


# ------------------------------------------------------------------------------------------------------------------ validation
class ValidationAccumulator:
    """The bookkeeping of one validation pass (trainer.py:142-149, 160-183, 230-234).  ``add`` takes one batch: its two per-sample loss
    vectors and its four per-sample metric vectors, on any device, and keeps them there; ``result`` reads everything back at once.

    The losses are means over BATCHES of the batch means (a short last batch weighs as much as a full one); the metrics are means over
    IMAGES.  The host arithmetic is the reference's: fp64 running sums in order of arrival.

    With a ``process_group`` every rank adds ITS rows of each global batch (``add_empty`` where it holds none: the short last batch of a
    ``shard_mode="batch"`` loader) and keeps, in fp64 on the device, ``[sum seg, sum sr, count]`` per global batch plus the four metric
    sums and the image count; ``result`` makes ONE SUM all-reduce of that table and aggregates as above over the GLOBAL batches:
    per-batch loss = sum / count, then the mean over batches; metrics are sums / images.  Every rank gets the same numbers, those of a
    one-rank pass over the same global batches (up to the rounding of the per-batch means, fp64 here where a one-rank pass takes an fp32
    mean).  Every rank must add the same number of batches.  ``device``: where the table lives when the rank saw nothing but empty slices.

    ``losses`` / ``metrics`` name what a single-rank pass of another regime carries (``validate_sr``: one loss, three metrics, fed through
    ``add_rows``); the rule and the one read-back are the same."""

    LOSSES = ("eval_segment_loss", "eval_sr_loss")
    METRICS = ("psnr", "ssim", "kernel_psnr", "iou")

    def __init__(self, process_group=None, device=None, losses=LOSSES, metrics=METRICS):
        self.loss_keys, self.metric_keys = tuple(losses), tuple(metrics)
        self.losses, self.metrics = [], {k: [] for k in self.metric_keys}
        self.pg, self.device = process_group, device
        self.rows, self.totals = [], None          # with a process group: fp64 [3] per global batch (None: a zero row), fp64 [5] metric sums + images

    def add_empty(self):
        """a global batch of which this rank holds nothing"""
        if self.pg is None:
            raise ValueError("an empty slice exists only in a data-parallel validation pass")
        self.rows.append(None)

    def add(self, segment_loss, sr_loss, psnr, ssim, kernel_psnr, iou):
        """``sr_loss`` None (a model without an SR loss: MODEL.SR == "bicubic") adds nothing to the SR sum (trainer.py:160-163)."""
        if sr_loss is None:
            sr_loss = torch.zeros_like(torch.as_tensor(segment_loss))
        if self.pg is not None:
            seg, sr = torch.as_tensor(segment_loss).double().reshape(-1), torch.as_tensor(sr_loss).double().reshape(-1)
            self.rows.append(torch.stack([seg.sum(), sr.sum(), seg.new_tensor(float(seg.numel()))]))
            ms = [torch.as_tensor(v).float().reshape(-1).double() for v in (psnr, ssim, kernel_psnr, iou)]
            tot = torch.stack([m.sum() for m in ms] + [seg.new_tensor(float(ms[0].numel()))])
            self.totals = tot if self.totals is None else self.totals + tot
            return
        self.add_rows((segment_loss, sr_loss), (psnr, ssim, kernel_psnr, iou))

    def add_rows(self, losses, metrics):
        """one batch of a single-rank pass: its per-sample loss vectors in the order of ``losses``, its per-sample metric vectors in the
        order of ``metrics``"""
        self.losses.append(torch.stack([torch.as_tensor(v).float().mean() for v in losses]))
        for k, v in zip(self.metric_keys, metrics):
            self.metrics[k].append(torch.as_tensor(v).float().reshape(-1))

    def _result_reduced(self):
        if not self.rows:
            raise ValueError("validation saw no batch")
        dev = next((r.device for r in self.rows if r is not None), torch.device("cpu") if self.device is None else torch.device(self.device))
        zero = torch.zeros(3, dtype=torch.float64, device=dev)
        table = torch.cat([zero if r is None else r for r in self.rows] + [torch.zeros(5, dtype=torch.float64, device=dev) if self.totals is None
                                                                          else self.totals])
        dist.all_reduce(table, op=dist.ReduceOp.SUM, group=self.pg)
        flat = table.cpu().tolist()
        nb = len(self.rows)
        rows, totals = [flat[3 * i:3 * i + 3] for i in range(nb)], flat[3 * nb:]
        n = int(round(totals[4]))
        out = {"eval_segment_loss": sum(r[0] / r[2] for r in rows) / nb, "eval_sr_loss": sum(r[1] / r[2] for r in rows) / nb}
        for i, k in enumerate(self.METRICS):
            out[k] = totals[i] / n
        out["batches"], out["images"] = nb, n
        return out

    def result(self):
        if self.pg is not None:
            return self._result_reduced()
        if not self.losses:
            raise ValueError("validation saw no batch")
        nb, nl = len(self.losses), len(self.loss_keys)
        n = int(sum(v.numel() for v in self.metrics[self.metric_keys[0]]))
        flat = torch.cat([torch.stack(self.losses).reshape(-1)] + [torch.cat(self.metrics[k]) for k in self.metric_keys]).cpu().double().tolist()
        losses, rest = flat[:nl * nb], flat[nl * nb:]
        out = {k: sum(losses[i::nl]) / nb for i, k in enumerate(self.loss_keys)}
        for i, k in enumerate(self.metric_keys):
            out[k] = sum(rest[i * n:(i + 1) * n]) / n
        out["batches"], out["images"] = nb, n
        return out


def check_downscale_agrees(model, *loaders):
    """SOLVER.DOWNSCALE_INTERPOLATION names ONE resize in the reference (train.py:43), used by the datasets and by KBPNLoss's pseudo-LR
    alike.  Here the loader (``.interpolation``) and the model (``.downscale``) each carry it: a loss that models another degradation
    than the data was made with trains silently wrong, so a disagreement is a ValueError before the first step.  A loader (or a model)
    that does not carry the attribute -- any plain iterable of batches -- is not checked."""
    want = getattr(model, "downscale", None)
    for loader in loaders:
        have = getattr(loader, "interpolation", None)
        if want is not None and have is not None and have != want:
            raise ValueError(f"the loader down-scales with {have!r} but the model's SR loss with {want!r} (SOLVER.DOWNSCALE_INTERPOLATION): "
                             "build both from the same cfg")


def _validation_pass(model, loader, seed, acc, add_batch):
    """The skeleton ``validate`` and ``validate_sr`` share: the loader's down-scale checked against the model's (check_downscale_agrees),
    re-seed the loader's generator (``seed`` not None), the model in ``eval()`` under
    ``no_grad``, ``add_batch(batch)`` for every batch the rank holds rows of, the mode restored, ``acc.result()``."""
    check_downscale_agrees(model, loader)
    if seed is not None:
        loader.gen.manual_seed(int(seed))
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for batch in loader:
                if batch is None:
                    acc.add_empty()
                else:
                    add_batch(batch)
    finally:
        model.train(was_training)
    return acc.result()


def validate(model, loader, iteration, *, seed=None, process_group=None):
    """One pass over ``loader`` (batches of ``(x, hr, mask, k[, sdf])``) with the model in ``eval()`` under ``no_grad``: validation
    segmentation and SR loss, PSNR, SSIM, kernel PSNR and IoU at 0.5 (trainer.py:140-235).  The SR image and the kernel are clamped to
    [0, 1] before their metrics; the segmentation map is binarised with ``>= 0.5`` first (``iou_sweep`` alone compares with ``>``).

    ``seed``: when not None the loader's generator is re-seeded with it first, so successive validations see the same crops and blurs and
    are comparable; None is the reference's behaviour, fresh draws in every pass.  The model's mode is restored; ``iter_cnt`` is not touched
    (``do_train`` switches it off around the call, as the reference does).

    Data-parallel (see ``_dist``; ``process_group`` None is the default group): ``loader`` is this rank's
    ``DeviceTrainLoader(shuffle=False, shard=(rank, world), shard_mode="batch")``, every rank walks the same global batches (a None
    batch is one of which the rank holds nothing: no forward) and gets the result over all of them (ValidationAccumulator)."""
    from .utils.estimate_metrics import iou_sweep, psnr_ssim
    pg = _dist(process_group)[0]
    acc = ValidationAccumulator() if pg is None else ValidationAccumulator(pg, _device_of(model))

    def add_batch(batch):
        x, hr, mask, k = batch[:4]
        extra = {"segment_sdf": batch[4]} if len(batch) > 4 else {}
        seg_l, sr_l, seg, sr, kp = model(iteration, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, **extra)
        ps, ss = psnr_ssim(sr.clamp(0, 1), hr)
        kps, _ = psnr_ssim(kp.clamp(0, 1), k)
        iou = iou_sweep((seg >= 0.5).float(), mask, [0.5])
        acc.add(seg_l, sr_l, ps, ss, kps, iou)
    return _validation_pass(model, loader, seed, acc, add_batch)


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
        "cuda_rng": _device_rng(dev),          # Dropout2d's masks are drawn from it
        "cpu_rng": torch.get_rng_state(),
        "loss_scale": {k: getattr(model, k) for k in ("grad_scale", "scale_backoff", "overflow_steps") if hasattr(model, k)},
        "logging": {"sums": sums.detach().cpu(), "overflowed": int(overflowed)},
    }


def save_checkpoint(output_dir, iteration, model, optimizer, train_loader=None, sums=None, overflowed=0, process_group=None):
    """``model/``, ``optimizer/`` (the reference's two files: plain state_dicts, loadable there and by torch.optim.Adam / SGD) and
    ``trainer/iteration_N.pth`` (everything else ``resume`` needs to continue exactly).  Returns the three paths.

    Data-parallel (see ``_dist``) this is a collective every rank calls: first ``assert_replicas_agree`` over parameters, buffers and the
    optimiser's state tensors (all but BatchNorm's running statistics, see ``replica_tensors``) -- ReplicaMismatch on every rank, and no
    file of this iteration, when a replica has drifted --, then rank 0
    writes the three files and a barrier follows.  The trainer file gains ``"world"`` and ``"ranks"``: per rank the device's and the
    host's generator state and, for a loader that is not in ``shard_mode="batch"`` (whose state is common), the rank's loader state.
    ``"logging"`` then holds the window sums of the GLOBAL batch (one more SUM all-reduce of two numbers)."""
    pg, rank, world = _dist(process_group)
    if pg is not None:
        return _save_checkpoint_dp(output_dir, iteration, model, optimizer, train_loader, sums, overflowed, pg, rank, world)
    paths = _paths(output_dir, iteration)
    for p in paths.values():
        os.makedirs(os.path.dirname(p), exist_ok=True)
    torch.save(model.state_dict(), paths["model"])
    torch.save(optimizer.state_dict(), paths["optimizer"])
    sums = torch.zeros(2, dtype=torch.float64) if sums is None else sums
    torch.save(_trainer_state(model, train_loader, iteration, sums, overflowed), paths["trainer"])
    return paths


def _save_checkpoint_dp(output_dir, iteration, model, optimizer, train_loader, sums, overflowed, pg, rank, world):
    agree.assert_replicas_agree(replica_tensors(model, optimizer, running_stats=False), pg, what=f"replicas at the checkpoint of iteration {iteration}")
    dev = _device_of(model)
    sums = torch.zeros(2, dtype=torch.float64, device=dev) if sums is None else sums.detach().clone()
    dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=pg)
    sums = sums / world
    per_rank = getattr(train_loader, "shard_mode", None) != "batch" and hasattr(train_loader, "state_dict")
    mine = {"cuda_rng": _device_rng(dev), "cpu_rng": torch.get_rng_state(), "loader": train_loader.state_dict() if per_rank else None}
    ranks = [None] * world if rank == 0 else None
    dist.gather_object(mine, ranks, dst=dist.get_global_rank(pg, 0), group=pg)
    paths = _paths(output_dir, iteration)
    if rank == 0:
        for p in paths.values():
            os.makedirs(os.path.dirname(p), exist_ok=True)
        torch.save(model.state_dict(), paths["model"])
        torch.save(optimizer.state_dict(), paths["optimizer"])
        state = _trainer_state(model, train_loader, iteration, sums, overflowed)
        state["world"], state["ranks"] = world, ranks
        torch.save(state, paths["trainer"])
    dist.barrier(group=pg)
    return paths


def resume(cfg, output_dir, iteration, model, optimizer, train_loader, process_group=None):
    """Load the checkpoint of ``iteration`` into freshly built objects and return the ``resume_iter`` to hand to ``build_scheduler`` and
    ``do_train``.  Build the model with ``resume_iter=iteration`` (its alpha then starts where the reference's would).

    With ``trainer/iteration_N.pth`` present the continued run IS the uninterrupted run: alpha and its counter, the loader's generator,
    permutation and cursor, the device's and the host's generator state, the loss-scale back-off and the logging sums are restored.  With
    only the reference's files the reference's semantics hold: weights through ``fix_model_state_dict`` with ``strict=False``, alpha from
    the model's constructor, a loader that starts over.  The optimiser file is loaded when it exists (the reference writes it and never
    reads it back).

    Data-parallel every rank calls it and loads the files.  At the world size the checkpoint was written at each rank restores ITS device
    and host generator state (and, outside ``shard_mode="batch"``, its loader state): the continued run is the uninterrupted run.  At
    another world size a ``shard_mode="batch"`` loader of the same global batch continues the same sample sequence and everything is
    restored but the generator states (Dropout2d's masks differ from here on), which a warning says; any other change of the world
    size is a ValueError."""
    world, rank = _dist(process_group)[2], _dist(process_group)[1]
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
    saved_world = int(st.get("world", 1))
    mine = st["ranks"][rank] if saved_world == world and st.get("ranks") is not None else st
    if saved_world != world:
        if getattr(train_loader, "shard_mode", None) != "batch" or st["loader"] is None or "global_batch" not in st["loader"]:
            raise ValueError(f"{paths['trainer']} was written by {saved_world} rank(s) and this run has {world}: only a run whose loaders are "
                             "in shard_mode='batch' with the same global batch continues on another world size")
        warnings.warn(f"resuming a checkpoint of {saved_world} rank(s) on {world}: the sample sequence, weights, optimiser state, alpha and "
                      "loss scale continue; the device and host generator states (Dropout2d masks) are not restored")
    loader_state = st["loader"] if mine.get("loader") is None else mine["loader"]
    if loader_state is not None and hasattr(train_loader, "load_state_dict"):
        train_loader.load_state_dict(loader_state)          # (a global batch other than the saved one raises here)
    dev = _device_of(model)
    if saved_world == world:
        if mine["cuda_rng"] is not None and dev.type == "cuda":
            torch.cuda.set_rng_state(mine["cuda_rng"], dev)
        torch.set_rng_state(mine["cpu_rng"])
    for k, v in st["loss_scale"].items():
        setattr(model, k, v)
    model._resume_logging = (int(iteration), st["logging"])          # picked up (once) by do_train(resume_iter=iteration)
    return int(iteration)


# ------------------------------------------------------------------------------------------------------------------ the loop
# What differs between the training regimes, for ``_loop``: ``names`` (the constant fields of every record), ``n_sums`` (how many batch means
# the window sums carry), ``begin(iteration)`` (called first in an iteration, before ``model.train()``; may be None), ``losses(iteration,
# batch) -> (the scalar to back-propagate, its n_sums batch means)``, ``record(window means) -> the loss fields of a log record`` and
# ``evaluate(iteration) -> a validation result``.
_Regime = collections.namedtuple("_Regime", "names n_sums begin losses record evaluate")


def _loop(regime, model, optimizer, scheduler, train_loader, eval_loader, resume_iter, log_step, save_step, eval_step, output_dir, log, hooks,
          process_group=None, pg=None, world=1):
    """The loop of ``do_train`` and ``do_pretrain_sr``: hooks, the step, the fp64 window sums on the device and their single read-back per
    ``log_step``, the overflow count, timing and ETA, and the checkpoint / eval / log cadence.  ``pg`` / ``world``: the data-parallel group
    (None: single process) the window sums are averaged over."""
    before, after = _hook(hooks, "before_step"), _hook(hooks, "after_step")
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
        if regime.begin is not None:
            regime.begin(iteration)
        model.train()
        optimizer.zero_grad()
        loss, means = regime.losses(iteration, batch)
        loss.backward()
        optimizer.step()
        scheduler.step()
        step_sums = torch.stack([v.detach() for v in means]).double()
        sums = step_sums if sums is None else sums.to(step_sums.device) + step_sums
        overflowed += bool(getattr(model, "last_step_overflowed", False))
        del loss, means, batch
        trained_time += time.time() - end
        end = time.time()

        record = None
        if iteration % log_step == 0:
            if pg is not None:          # equal shards: the mean over the ranks is the mean over the global batch
                dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=pg)
                sums = sums / world
            window = [v / log_step for v in sums.tolist()]          # the one read-back of the window
            eta = "?" if max_iter is None else str(datetime.timedelta(seconds=int(trained_time / (iteration - resume_iter)
                                                                                  * (max_iter - iteration))))
            record = {"iteration": iteration, "lr": optimizer.param_groups[0]["lr"], **regime.record(window),
                      "overflow_steps": overflowed, "cost_s": time.time() - tic, "eta": eta, **regime.names}
            log(record)
            sums = None
            tic = time.time()

        if output_dir is not None and iteration % save_step == 0:
            paths = save_checkpoint(output_dir, iteration, model, optimizer, train_loader,
                                    torch.zeros(regime.n_sums, dtype=torch.float64, device=_device_of(model)) if sums is None else sums,
                                    overflowed, process_group=process_group)
            log({"iteration": iteration, "checkpoint": paths["model"], **paths})

        if eval_loader is not None and iteration % eval_step == 0:
            log({"iteration": iteration, **regime.evaluate(iteration), **regime.names})

        if after is not None:
            after(iteration, model, record)


def do_train(cfg, model, optimizer, scheduler, train_loader, eval_loader=None, *, resume_iter=0, log_step=50, save_step=2000, eval_step=2000,
             output_dir=None, log=print_line, hooks=None, process_group=None):
    """Train over ``train_loader`` (any iterable of ``(x, hr, mask, k)`` or ``(x, hr, mask, k, sdf)``), iterations counted from
    ``resume_iter + 1``.  A loader that carries ``.interpolation`` (DeviceTrainLoader) must down-scale as the model's loss does
    (``model.downscale``, SOLVER.DOWNSCALE_INTERPOLATION): ValueError before the first step otherwise.  Per iteration: set_alpha_phase, model.train(), zero_grad, forward, calc_loss, backward, optimizer.step(),
    scheduler.step().  ``hooks`` (a dict or an object) may carry ``before_step(iteration, model)``, called first in an iteration, and
    ``after_step(iteration, model, record)``, called last with that iteration's log record or None.

    Every ``log_step`` iterations ``log`` receives {iteration, lr, segment_loss, sr_loss, total, boundary_alpha, overflow_steps, ...}: the
    losses are window means, ``total`` is ``sr + TASK_LOSS_WEIGHT * seg``, ``overflow_steps`` counts the steps skipped so far because the
    fp16 backward overflowed (``model.last_step_overflowed``, a host flag).  That is the loop's only read-back of device values.  Every
    ``save_step`` iterations the three checkpoint files are written under ``output_dir`` (None: no checkpoints); every ``eval_step``
    iterations, with an ``eval_loader``, ``validate`` runs with ``model.iter_cnt`` off and its result goes to ``log``.

    Data-parallel (``torch.distributed`` initialised with world > 1, or CSBSR_FORCE_DIST=1; ``process_group`` None is the default group),
    every rank calls this with its own model, optimiser and loaders.  At the start a ``GradBucketReducer`` is attached where
    ``model.reducer`` is None, rank 0's parameters and buffers are broadcast and ``assert_replicas_agree`` checks them.  A step is
    unchanged (the model's backward drives the reducer; no collective is added).  At a log step the two window sums are SUM-all-reduced
    and divided by the world size -- with equal shards the mean over the global batch --, ``log`` is called on rank 0 only and
    ``after_step`` receives the record on every rank; ``overflow_steps`` is common already (the ranks agree on the skip).  Validation and
    checkpoints: see ``validate`` and ``save_checkpoint``; both are collectives, and a drifted replica raises ReplicaMismatch on every
    rank before a file is written."""
    check_downscale_agrees(model, train_loader, eval_loader)
    pg, rank, world = _dist(process_group)
    if pg is not None:
        dev = _device_of(model)
        if getattr(model, "reducer", None) is None:
            model.reducer = GradBucketReducer(pg, side_stream=torch.cuda.Stream(dev) if dev.type == "cuda" else None)
        if hasattr(model, "_runtime"):
            model._runtime()          # the parameters move to the device here: broadcast and fingerprint them where they will be trained
        broadcast_parameters(model, process_group=pg)
        agree.assert_replicas_agree(replica_tensors(model), pg, what="parameters and buffers after the broadcast")
        if rank != 0:
            log = lambda record: None          # noqa: E731  (rank 0 speaks for the run)

    def losses(iteration, batch):
        x, hr, mask, k = batch[:4]
        extra = {"segment_sdf": batch[4]} if len(batch) > 4 else {}
        segment_loss, sr_loss = model(iteration, x, sr_targets=hr, segment_targets=mask, kernel_targets=k, **extra)[:2]
        # (no SR loss -- MODEL.SR == "bicubic" -- : its window sum stays 0 and the scalar is the segmentation mean, see calc_loss)
        seg, sr = segment_loss.mean(), (segment_loss.new_zeros(()) if sr_loss is None else sr_loss.mean())
        return _scalar(seg, sr, iteration, cfg), (seg, sr)

    def record(window):
        seg_m, sr_m = window
        fn = getattr(model, "ss_loss_fn", None)
        return {"segment_loss": seg_m, "sr_loss": sr_m, "total": sr_m + cfg.SOLVER.TASK_LOSS_WEIGHT * seg_m,
                "boundary_alpha": fn.alpha if fn is not None and "Boundary" in cfg.SOLVER.SEG_LOSS_FUNC else None}

    def evaluate(iteration):
        model.iter_cnt = False
        try:
            return validate(model, eval_loader, iteration, process_group=process_group)
        finally:
            model.iter_cnt = True
    regime = _Regime({"seg_loss_func": cfg.SOLVER.SEG_LOSS_FUNC, "sr_loss_func": cfg.SOLVER.SR_LOSS_FUNC}, 2,
                     lambda iteration: set_alpha_phase(cfg, model, iteration), losses, record, evaluate)
    _loop(regime, model, optimizer, scheduler, train_loader, eval_loader, resume_iter, log_step, save_step, eval_step, output_dir, log, hooks,
          process_group, pg, world)


# ------------------------------------------------------------------------------------------------------------------ SR-only pretraining
def print_pretrain_line(record):
    """The default ``log`` of ``do_pretrain_sr``: the reference's console lines (trainer.py:300, :326, :392-393)."""
    if "checkpoint" in record:
        print("=====> Save Checkpoint to {}".format(record["checkpoint"]))
    elif "eval_sr_loss" in record:
        print(f"\nestimation result (iter={record['iteration']}):")
        print(f"=====> SR_Loss({record['sr_loss_func']}): {record['eval_sr_loss']:.6f} PSNR:{record['psnr']:.4f} SSIM:{record['ssim']:.4f} "
              f"PSNR(Kernel):{record['kernel_psnr']:.4f}")
    else:
        print("===> Iter: {:07d}, LR: {:.5f}, Cost: {:.2f}s, Eta: {}, SR_Loss({}): {:.6f}".format(
            record["iteration"], record["lr"], record["cost_s"], record["eta"], record["sr_loss_func"], record["sr_loss"]))


def validate_sr(model, loader, iteration, *, seed=None):
    """One pass over ``loader`` (batches of ``(x, hr, k)``) with an SR-only model in ``eval()`` under ``no_grad`` (trainer.py:328-393):
    the SR loss averaged over BATCHES, PSNR, SSIM and kernel PSNR averaged over IMAGES with the SR image and the kernel clamped to [0, 1].
    ``seed`` as in ``validate``; the model's mode is restored."""
    from .utils.estimate_metrics import psnr_ssim
    acc = ValidationAccumulator(losses=("eval_sr_loss",), metrics=("psnr", "ssim", "kernel_psnr"))

    def add_batch(batch):
        x, hr, k = batch
        sr_l, sr, kp = model(iteration, x, sr_targets=hr, kernel_targets=k)
        ps, ss = psnr_ssim(sr.clamp(0, 1), hr)
        kps, _ = psnr_ssim(kp.clamp(0, 1), k)
        acc.add_rows((sr_l,), (ps, ss, kps))
    return _validation_pass(model, loader, seed, acc, add_batch)


def export_pretrained_sr(model_or_state_dict, cfg, root="weights"):
    """Write ``<root>/pretrain/KBPN_pretrain_x{SCALE}_stage{S}[_bicubic{K}].pth`` -- the ``sr_model.*`` tensors of an SR-only or joint
    model (or of a state_dict of one, ``module.`` prefixes dropped), which is what ``MODEL.SR_SCRATCH = False`` loads -- and return its path."""
    from .modeling.build_model import pretrained_sr_path
    sd = model_or_state_dict.state_dict() if hasattr(model_or_state_dict, "state_dict") else model_or_state_dict
    sd = {k: v.detach().cpu().clone() for k, v in fix_model_state_dict(sd).items() if k.startswith("sr_model.")}
    if not sd:
        raise ValueError("no sr_model.* tensor to export")
    path = pretrained_sr_path(cfg, root)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(sd, path)
    return path


def do_pretrain_sr(cfg, model, optimizer, scheduler, train_loader, eval_loader=None, *, resume_iter=0, log_step=50, save_step=2000, eval_step=2000,
                   output_dir=None, log=print_pretrain_line, hooks=None):
    """Train an SR-only model over ``train_loader`` (any iterable of ``(x, hr, k)``), iterations counted from ``resume_iter + 1``.  Per
    iteration (trainer.py:275-290): model.train(), zero_grad, forward, ``sr_loss.mean()``, backward, optimizer.step(), scheduler.step().
    Build the scheduler with ``build_scheduler(..., scheduler_flag=False)``.  ``hooks`` as in ``do_train``.

    Every ``log_step`` iterations ``log`` receives {iteration, lr, sr_loss, overflow_steps, cost_s, eta, sr_loss_func}; ``sr_loss`` is the
    window mean, summed on the device in fp64 and read back there -- the loop's only read-back.  Checkpoints are ``save_checkpoint``'s
    three files and ``resume`` continues the run exactly; every ``eval_step`` iterations, with an ``eval_loader``, ``validate_sr`` runs
    and its result goes to ``log``.  Data-parallel pretraining is not built: NotImplementedError before anything touches the device."""
    if _forced() or (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        raise NotImplementedError("do_pretrain_sr is single-GPU: data-parallel SR pretraining is not built")
    check_downscale_agrees(model, train_loader, eval_loader)

    def losses(iteration, batch):
        x, hr, k = batch
        sr = model(iteration, x, sr_targets=hr, kernel_targets=k.detach())[0].mean()
        return sr, (sr,)
    regime = _Regime({"sr_loss_func": cfg.SOLVER.SR_LOSS_FUNC}, 1, None, losses, lambda window: {"sr_loss": window[0]},
                     lambda iteration: validate_sr(model, eval_loader, iteration))
    _loop(regime, model, optimizer, scheduler, train_loader, eval_loader, resume_iter, log_step, save_step, eval_step, output_dir, log, hooks)
