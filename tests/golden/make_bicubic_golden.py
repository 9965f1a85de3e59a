"""tests/golden/bicubic_pspnet.npz: the REFERENCE's JointModelWithLoss with MODEL.SR="bicubic" + PSPNet, train mode, one step at iteration
40000, and its JointModel in eval mode, run on the CPU through ref_shims like make_golden.py -- on the inputs (make_batch, seed 1121, LR 64
-> HR 256) and the detector weights (deterministic "random" fill, alpha 0.7, no dropout) of wc_pspnet_it40000.

    python tests/golden/make_bicubic_golden.py

Only data is written.  The repository's contribution rule is that no newly committed file exceeds 1 MiB (the wc_*
fixtures predate it) and an fp32 SR image does not compress, so the fixture holds the FIRST sample of that batch (B = 1: 0.79 MB of
sr_preds); the LR input, the BatchNorm buffers and the eval-mode outputs go to a file of their own, bicubic_pspnet_eval.npz
(tests/bicubic_cases.fixture() reads the two as one mapping), which leaves the first file about 10 % under the limit; and the eval-mode SR
image is not repeated: the reference's JointModel returns exactly clamp(sr_preds, 0, 1) of the training-mode image -- same Resize on the
same input -- which this script asserts and records as ``eval_sr_is_clamped_sr``.  The eval-mode map is stored as returned.

The eval-mode JointModel carries the CONTRACTIVE fill (csbsr_amd.utils.detfill, the fill of the wc2_* fixtures), not the random one of the
training-mode run.  In eval mode BatchNorm uses the fill's running statistics, not the batch's, and the random-fill detector then is no
network any more: the reference's own eval-mode map is saturated (96 % of its pixels are exactly 0.0 or 1.0) and moves by 5.4e-4 when the
LR input moves by 1e-6 and by 3.1e-2 when it moves by 1e-4 (uniform noise; measured with this reference on the CPU), so no implementation
that is not bit-identical can be held to 1e-3 on it -- this build's split-precision detector lands at 4.1e-2 there with an SR image that
equals the reference's bit for bit.  With the contractive fill the same experiment gives 2.5e-6 and 1.6e-4 (a gain of 2), the map spans
0.06 .. 0.65, and the 1e-3 bound is a statement about the code.  Both responses are recorded in the file (``eval_cond_*``).
"""
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the shims; DropCapture, deterministic_fill, make_batch)

NAME, IT, B, LR, SCALE, ALPHA, SEED = "bicubic_pspnet", 40000, 1, 64, 4, 0.7, 1121


def main():
    ref_shims.ANTIALIAS = True
    cfg, JM, J, FR = ref_shims.build_reference(detector="PSPNet", scale=SCALE, overrides=("MODEL.SR", "bicubic"))
    x, hr, mask, k = (t[:B].contiguous() for t in MG.make_batch(2, LR, scale=SCALE, ksize=cfg.BLUR.KERNEL_SIZE_OUTPUT, seed=SEED))
    from model.engine.trainer import calc_loss
    import argparse
    model = JM(cfg, 1000, 0, FR(SCALE, "bicubic"))
    assert model.sr_model == "bicubic" and not any(n.startswith("sr_model") for n in model.state_dict())
    MG.deterministic_fill(model, "random")
    model.train()
    model.ss_loss_fn.alpha = ALPHA
    cap = MG.DropCapture(False)
    orig = nn.Dropout2d.forward
    nn.Dropout2d.forward = lambda self, x_: cap(self, x_)
    try:
        seg_loss, sr_loss, seg, sr, kpred = model(IT, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
        assert sr_loss is None and float(kpred.abs().max()) == 0.0 and kpred.shape == k.shape
        loss, _, _ = calc_loss(seg_loss, 0.0, sr_loss, 0.0, IT, cfg, argparse.Namespace())
        model.zero_grad()
        loss.backward()
    finally:
        nn.Dropout2d.forward = orig
    names, norms, samples = [], [], []
    for n, p in model.named_parameters():
        names.append(n)
        if p.grad is None:
            norms.append(-1.0)
            samples.append(np.zeros(32, np.float32))
            continue
        flat = p.grad.detach().reshape(-1)
        norms.append(float(flat.double().norm()))
        idx = [(zlib.crc32((n + str(j)).encode()) % flat.numel()) for j in range(32)]
        samples.append(flat[idx].numpy().astype(np.float32))
    bufs = {n: b.detach().clone() for n, b in model.named_buffers() if "running" in n and n.startswith("segmentation_model")}
    # the inference class: contractive fill (module docstring), and the reference's own conditioning under both fills
    cond = {}
    for fill in ("random", "contractive"):
        ev = J(cfg)
        MG.deterministic_fill(ev, fill)
        ev.eval()
        with torch.no_grad():
            e_sr, e_seg, e_k = ev(x, torch.zeros(B, 1, 21, 21), sr_targets=hr)
            gen = torch.Generator().manual_seed(4242)
            for eps in (1e-6, 1e-4):
                moved = ev(x + (torch.rand(x.shape, generator=gen) * 2 - 1) * eps, torch.zeros(B, 1, 21, 21), sr_targets=hr)[1]
                cond[f"eval_cond_{fill}_{eps:g}"] = np.float64(float((moved - e_seg).abs().max()))
        cond[f"eval_saturated_{fill}"] = np.float64(float(((e_seg == 0) | (e_seg == 1)).float().mean()))
    assert torch.equal(e_sr, sr.detach().clamp(0, 1)) and float(e_k.abs().max()) == 0.0
    out = dict(seed=np.int64(SEED), B=np.int64(B), lr=np.int64(LR), it=np.int64(IT), kernel=k.numpy(),
               hr_sum=np.float64(hr.double().sum()), mask_sum=np.float64(mask.double().sum()),
               segment_loss=seg_loss.detach().numpy(), loss=np.float64(float(loss)), segment_preds=seg.detach().numpy(),
               sr_preds=sr.detach().numpy(), kernel_preds_shape=np.array(kpred.shape, dtype=np.int64),
               grad_names=np.array(names), grad_norms=np.array(norms), grad_samples32=np.stack(samples),
               alpha=np.float64(model.ss_loss_fn.alpha), antialias=np.bool_(True), scale=np.int64(SCALE), detector=np.array("PSPNet"),
               beta=np.float64(cfg.SOLVER.TASK_LOSS_WEIGHT), fill=np.array("random"), torch_version=np.array(torch.__version__),
               eval_sr_is_clamped_sr=np.bool_(True), eval_sr_clipped_pixels=np.int64(int((e_sr != sr.detach()).sum())))
    np.savez_compressed(os.path.join(HERE, NAME + "_eval.npz"), x=x.numpy(), eval_segment_preds=e_seg.numpy(), eval_fill=np.array("contractive"),
                        eval_kernel_preds_shape=np.array(e_k.shape, dtype=np.int64), **cond, **{"buf." + kname: v.numpy() for kname, v in bufs.items()})
    print({k: float(v) for k, v in cond.items()})
    path = os.path.join(HERE, NAME + ".npz")
    np.savez_compressed(path, **out)
    size, wc = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "wc_pspnet_it40000.npz"))
    print(f"{NAME}: loss={float(loss):.6f} seg_loss={seg_loss.tolist()} clipped pixels {int(out['eval_sr_clipped_pixels'])} -> {size / 1e6:.3f} MB")
    assert size <= wc and size <= 0.95 * (1 << 20), (size, wc)          # (a margin for another zlib)


if __name__ == "__main__":
    main()
