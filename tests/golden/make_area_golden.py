"""tests/golden/e2e_pspnet_area_it1.npz and e2e_pspnet_area_it40000.npz: the REFERENCE's JointModelWithLoss (KBPN + PSPNet) with
SOLVER.DOWNSCALE_INTERPOLATION = 'area' -- FactorResize(scale, 'area') handed to the model, so KBPNLoss's pseudo-LR is the box mean of the
blurred SR image (sr_loss_functions.py:94) -- run on the CPU through ref_shims like make_golden.py, at B = 2, LR 16 -> HR 64, x4:

    python tests/golden/make_area_golden.py

    it1       SR phase (the loss is the SR loss alone)
    it40000   joint phase, alpha 0.7

The LR input ``x`` is made with 'area' too (crack_dataset.py:62: the datasets use the same FactorResize): the synthetic HR texture, masks
and blur kernels of csbsr_amd.data.synthetic with the same draws as make_batch, blurred, FactorResize'd by the reference's class, clamped.
Weights: the deterministic fill of the e2e_* fixtures.  Only data is written.  Each file holds the inputs, the losses, sr_preds /
kernel_preds / segment_preds, the reference's pseudo-LR ``lr_pred``, make_golden's gradient digest (and the same digest with 32 sampled
elements per tensor, ``grad_samples32``, the form tests/test_wc_parity_gpu.py's comparison reads); it1 also d sr_loss.sum() / d sr_preds and
/ d kernel_preds (``dsr``, ``dkpred``; retain_grad on the tensors the model returns) and the same two from a CONTROL run of the same
inputs with 'bicubic' (``ctl_dsr``, ``ctl_dkpred``, plus ``ctl_sr_loss`` / ``ctl_lr_pred``).

Two conditions, asserted here:
  * the LR term's gradient is sign(lr_pred - x): the seed is the first from 1121 upward (at most 32 tries) for which min |lr_pred - x| >=
    1e-4 in the it1 case -- ten times the bound csbsr_blur_fwd is held to -- so no implementation within that bound flips a sign; the value
    is recorded (``min_abs_lr_diff``), as is the control's (``ctl_min_abs_lr_diff``, not part of the search);
  * sr_preds and kernel_preds of the area run equal those of its bicubic control bit for bit: KBPN's forward never sees the down-sampler.
"""
import argparse
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the shims; DropCapture, deterministic_fill, grad_digest)

B, LR, SCALE, ALPHA, SEED0, TRIES, MIN_DIFF = 2, 16, 4, 0.7, 1121, 32, 1e-4
# the BatchNorm running buffers make_golden.run_case records for PSPNet
BUFFERS = ("segmentation_model.feats.bn1.running_mean", "segmentation_model.feats.bn1.running_var",
           "segmentation_model.up_3.conv.1.running_var", "segmentation_model.aux.1.running_mean")


def make_inputs(seed, FR, ksize):
    """make_batch's draws (csbsr_amd.data.synthetic) with the reference's FactorResize('area') in place of the bicubic resize"""
    from csbsr_amd.data.synthetic import make_hr_mask, gaussian_kernels
    gen = torch.Generator().manual_seed(seed)
    H = LR * SCALE
    hr, mask = make_hr_mask(B, H, gen)
    k = gaussian_kernels(B, ksize, gen)
    blurred = F.conv2d(hr.reshape(1, B * 3, H, H), k.repeat_interleave(3, dim=0), padding=(ksize - 1) // 2, groups=B * 3).reshape(B, 3, H, H)
    x = FR(SCALE, "area")(blurred).clamp(0, 1)
    return x.contiguous(), hr, mask, k


def digest32(model):
    samples = []
    for n, p in model.named_parameters():
        if p.grad is None:
            samples.append(np.zeros(32, np.float32))
            continue
        g = p.grad.detach().reshape(-1)
        samples.append(g[[(zlib.crc32((n + str(j)).encode()) % g.numel()) for j in range(32)]].numpy().astype(np.float32))
    return np.stack(samples)


def run(mode, it, inputs, alpha=None, loss_grads=False):
    """one step of the reference with FactorResize(SCALE, mode) -> dict of detached results"""
    ref_shims.ANTIALIAS = True
    cfg, JM, J, FR = ref_shims.build_reference(detector="PSPNet", scale=SCALE, overrides=("SOLVER.DOWNSCALE_INTERPOLATION", mode))
    from model.engine.trainer import calc_loss
    from model.utils.sr_loss_functions import Get_pseudo_lr
    x, hr, mask, k = inputs
    model = JM(cfg, 1000, 0, FR(SCALE, mode))
    MG.deterministic_fill(model)
    model.train()
    if alpha is not None:
        model.ss_loss_fn.alpha = alpha
    cap = MG.DropCapture(False)
    held = {}
    orig_drop, orig_lr = nn.Dropout2d.forward, Get_pseudo_lr.__call__

    def pseudo_lr(self, sr_t, kernel):
        lrs, weight = orig_lr(self, sr_t, kernel)
        held["lr_pred"] = lrs.detach().clone()
        return lrs, weight
    if loss_grads:
        # at iteration 1 (SR-module pretraining) the kernel predictor is frozen and KBPN's kernel output requires no gradient; the loss is
        # a function of it all the same, so it is made a leaf that does: no value and no parameter gradient changes
        sr_fwd = model.sr_model.forward

        def fwd(x_, it_, k_):
            sr_, kp_ = sr_fwd(x_, it_, k_)
            return sr_, (kp_ if kp_.requires_grad else kp_.detach().requires_grad_(True))
        model.sr_model.forward = fwd
    nn.Dropout2d.forward = lambda self, x_: cap(self, x_)
    Get_pseudo_lr.__call__ = pseudo_lr
    try:
        seg_loss, sr_loss, seg, sr, kpred = model(it, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
        out = {}
        if loss_grads:
            sr.retain_grad()
            kpred.retain_grad()
            sr_loss.sum().backward(retain_graph=True)
            out["dsr"], out["dkpred"] = sr.grad.detach().clone(), kpred.grad.detach().clone()
            sr.grad = kpred.grad = None
        loss, _, _ = calc_loss(seg_loss, 0.0, sr_loss, 0.0, it, cfg, argparse.Namespace())
        model.zero_grad()
        loss.backward()
    finally:
        nn.Dropout2d.forward, Get_pseudo_lr.__call__ = orig_drop, orig_lr
    names, norms, samples = MG.grad_digest(model)
    out["bufs"] = {n: b.detach().clone() for n, b in model.named_buffers() if n in BUFFERS}
    out.update(cfg=cfg, segment_loss=seg_loss.detach(), sr_loss=sr_loss.detach(), loss=float(loss.detach()), segment_preds=seg.detach(), sr_preds=sr.detach(),
               kernel_preds=kpred.detach(), lr_pred=held["lr_pred"], grad_names=np.array(names), grad_norms=norms, grad_samples=samples,
               grad_samples32=digest32(model), alpha=float(model.ss_loss_fn.alpha))
    return out


def write(name, it, seed, inputs, a, extra):
    x, hr, mask, k = inputs
    cfg = a["cfg"]
    out = dict(x=x.numpy(), hr=hr.numpy(), mask=mask.numpy(), kernel=k.numpy(), it=np.int64(it), seed=np.int64(seed),
               segment_loss=a["segment_loss"].numpy(), sr_loss=a["sr_loss"].numpy(), loss=np.float64(a["loss"]),
               segment_preds=a["segment_preds"].numpy(), sr_preds=a["sr_preds"].numpy(), kernel_preds=a["kernel_preds"].numpy(),
               lr_pred=a["lr_pred"].numpy(), grad_names=a["grad_names"], grad_norms=a["grad_norms"], grad_samples=a["grad_samples"],
               grad_samples32=a["grad_samples32"], alpha=np.float64(a["alpha"]), antialias=np.bool_(True), scale=np.int64(SCALE),
               detector=np.array("PSPNet"), sfo_sr_amp=np.float64(cfg.SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SR_AMP),
               oriented_w_iter=np.int64(cfg.SOLVER.ORIENTED_WEIGHT_ITER), beta=np.float64(cfg.SOLVER.TASK_LOSS_WEIGHT),
               downscale=np.array("area"), fill=np.array("random"), torch_version=np.array(torch.__version__),
               min_abs_lr_diff=np.float64(float((a["lr_pred"] - x).abs().min())), **extra,
               **{"buf." + n: v.numpy() for n, v in a["bufs"].items()})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{name}: seed {seed} loss={a['loss']:.6f} sr={a['sr_loss'].tolist()} min|lr_pred - x| {float(out['min_abs_lr_diff']):.3e} -> {size / 1e3:.0f} kB")
    assert size < (1 << 19), size          # well under the 1 MiB limit


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    _, _, _, FR = ref_shims.build_reference(detector="PSPNet", scale=SCALE)
    for seed in range(SEED0, SEED0 + TRIES):
        inputs = make_inputs(seed, FR, 21)
        a1 = run("area", 1, inputs, loss_grads=True)
        gap = float((a1["lr_pred"] - inputs[0]).abs().min())
        print(f"seed {seed}: min |lr_pred - x| = {gap:.3e}")
        if gap >= MIN_DIFF:
            break
    else:
        raise SystemExit(f"no seed in [{SEED0}, {SEED0 + TRIES}) keeps |lr_pred - x| >= {MIN_DIFF}")
    assert float((a1["lr_pred"] - inputs[0]).abs().min()) >= MIN_DIFF
    c1 = run("bicubic", 1, inputs, loss_grads=True)
    # KBPN's forward never sees the down-sampler
    assert torch.equal(a1["sr_preds"], c1["sr_preds"]) and torch.equal(a1["kernel_preds"], c1["kernel_preds"])
    assert not torch.equal(a1["lr_pred"], c1["lr_pred"]) and not torch.equal(a1["sr_loss"], c1["sr_loss"])
    write("e2e_pspnet_area_it1", 1, seed, inputs, a1,
          dict(dsr=a1["dsr"].numpy(), dkpred=a1["dkpred"].numpy(), ctl_dsr=c1["dsr"].numpy(), ctl_dkpred=c1["dkpred"].numpy(),
               ctl_sr_loss=c1["sr_loss"].numpy(), ctl_lr_pred=c1["lr_pred"].numpy(),
               ctl_min_abs_lr_diff=np.float64(float((c1["lr_pred"] - inputs[0]).abs().min()))))
    a2 = run("area", 40000, inputs, alpha=ALPHA)
    c2 = run("bicubic", 40000, inputs, alpha=ALPHA)
    assert torch.equal(a2["sr_preds"], c2["sr_preds"]) and torch.equal(a2["kernel_preds"], c2["kernel_preds"])
    write("e2e_pspnet_area_it40000", 40000, seed, inputs, a2, {})


if __name__ == "__main__":
    main()
