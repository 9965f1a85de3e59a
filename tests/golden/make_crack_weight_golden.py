"""Fixtures of the crack-oriented SR-loss weight  w^C = lambda * exp(-amp * d)  (SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP), produced by the
REFERENCE on the CPU through ref_shims like make_golden.py / make_bicubic_golden.py:

    python tests/golden/make_crack_weight_golden.py

  crack_weight_maps.npz            masks and the reference's own CrackOrientedExpWeight output (and its F.interpolate LR map, s = 4) for
                                   (4,1,40,300) -- sparse cracks / all background / all foreground / one corner pixel plus the soft values
                                   0.5 and 0.99, which the reference's uint8 cast makes background -- and (2,1,64,64) at 30 % foreground,
                                   each at amp 0.1 and 2.0 (the second reaches the fp32 underflow region), lambda = 2 (the class default)
  e2e_pspnet_wco_it40000.npz       make_golden.run_case's recipe and key set of e2e_pspnet_wf_it40000 with w^C alone (amp 0.1,
                                   ORIENTED_WEIGHT_ITER 100), plus ``co_sr_amp`` and the digests below
  e2e_pspnet_wcofo_it40000.npz     the same with w^F on as well (its amp the wf fixture's, 1.0)
  e2e_pspnet_it40000_srgrad.npz    the digests alone for the unweighted e2e_pspnet_it40000 case (that file is not rewritten)

The digests (``srgrad_names`` / ``srgrad_norms`` / ``srgrad_samples32``): a second reference backward, of sr_loss.mean() alone, recorded per
``sr_model.*`` parameter as the gradient's L2 norm and 32 crc-indexed elements, the way make_bicubic_golden.py records its gradients.  Every
other parameter is asserted to get no gradient from that scalar.  Only data is written.

The files are reproducible byte for byte: numpy stamps the members of an .npz with the wall clock, so they are written here with the fixed
date 1980-01-01 (``save_npz``; the arrays and the compression are numpy's own).
"""
import io
import os
import sys
import zipfile
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_shims  # noqa: E402
import make_golden as MG  # noqa: E402  (installs the shims; DropCapture, deterministic_fill, make_batch, run_case)

IT, ALPHA, SCALE, LAMBDA = 40000, 0.7, 4, 2
WCO = ("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", 0.1, "SOLVER.ORIENTED_WEIGHT_ITER", 100)
WCOFO = WCO + ("SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SR_AMP", 1.0)


def save_npz(path, arrays):
    """np.savez_compressed's file with a fixed member date."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())


def masks_40x300():
    rng = np.random.RandomState(20)
    m = np.zeros((4, 1, 40, 300), np.float32)
    m[0, 0] = (rng.rand(40, 300) < 0.01).astype(np.float32)      # sparse cracks; sample 1 stays all background
    m[2] = 1.0
    m[3, 0, 39, 299] = 1.0
    m[3, 0, 5, 7], m[3, 0, 20, 150] = 0.5, 0.99                  # soft values: background after the uint8 cast
    return m


def masks_64x64():
    return (np.random.RandomState(21).rand(2, 1, 64, 64) < 0.3).astype(np.float32)


def weight_maps():
    from model.utils.oriented_weight import CrackOrientedExpWeight
    out = {"lambda": np.float64(LAMBDA), "scale": np.int64(SCALE), "amps": np.array([0.1, 2.0])}
    for tag, m in (("a", masks_40x300()), ("b", masks_64x64())):
        out[f"mask_{tag}"] = m
        for amp in (0.1, 2.0):
            w = CrackOrientedExpWeight(None, amp, 0.0)(torch.from_numpy(m))
            assert w.dtype == torch.float32 and w.shape == m.shape
            out[f"w_hr_{tag}_{amp:g}"] = w.numpy()
            out[f"w_lr_{tag}_{amp:g}"] = F.interpolate(w, scale_factor=1 / SCALE, mode="bilinear").numpy()
    save_npz(os.path.join(HERE, "crack_weight_maps.npz"), out)
    print("crack_weight_maps:", {k: v.shape for k, v in out.items() if k.startswith("w_")})


def sr_grad_digest(overrides, seed):
    """The reference model of run_case (same cfg, fill, inputs, no dropout), backward of sr_loss.mean() alone -> the digests and sr_loss."""
    ref_shims.ANTIALIAS = True
    cfg, JM, J, FR = ref_shims.build_reference(detector="PSPNet", scale=SCALE, overrides=overrides)
    model = JM(cfg, 1000, 0, FR(SCALE, "bicubic"))
    MG.deterministic_fill(model)
    model.train()
    model.ss_loss_fn.alpha = ALPHA
    cap = MG.DropCapture(False)
    orig = nn.Dropout2d.forward
    nn.Dropout2d.forward = lambda self, x_: cap(self, x_)
    x, hr, mask, k = MG.make_batch(2, 16, scale=SCALE, ksize=cfg.BLUR.KERNEL_SIZE_OUTPUT, seed=seed, antialias=True)
    try:
        seg_loss, sr_loss, seg, sr, kpred = model(IT, x, sr_targets=hr, segment_targets=mask, kernel_targets=k)
        model.zero_grad()
        sr_loss.mean().backward()
    finally:
        nn.Dropout2d.forward = orig
    names, norms, samples = [], [], []
    for n, p in model.named_parameters():
        if not n.startswith("sr_model."):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            continue
        if p.grad is None:
            continue
        flat = p.grad.detach().reshape(-1)
        names.append(n)
        norms.append(float(flat.double().norm()))
        idx = [(zlib.crc32((n + str(j)).encode()) % flat.numel()) for j in range(32)]
        samples.append(flat[idx].numpy().astype(np.float32))
    return dict(srgrad_names=np.array(names), srgrad_norms=np.array(norms), srgrad_samples32=np.stack(samples)), sr_loss.detach().numpy()


def e2e(name, overrides, seed):
    MG.run_case(name, IT, alpha=ALPHA, seed=seed, overrides=overrides)
    path = os.path.join(HERE, name + ".npz")
    with np.load(path) as z:
        out = {k: z[k] for k in z.files}
    dig, sr_loss = sr_grad_digest(overrides, seed)
    assert np.array_equal(sr_loss, out["sr_loss"]), (sr_loss, out["sr_loss"])      # the second forward is the first one's
    out.update(dig, co_sr_amp=np.float64(overrides[1]))
    save_npz(path, out)
    print(f"{name}: {len(dig['srgrad_names'])} sr_model tensors -> {os.path.getsize(path) / 1e3:.0f} kB")
    assert os.path.getsize(path) < (1 << 20)


def main():
    weight_maps()
    dig, sr_loss = sr_grad_digest((), 1121)
    with np.load(os.path.join(HERE, "e2e_pspnet_it40000.npz")) as z:
        assert np.array_equal(sr_loss, z["sr_loss"]), (sr_loss, z["sr_loss"])
    save_npz(os.path.join(HERE, "e2e_pspnet_it40000_srgrad.npz"), dig)
    e2e("e2e_pspnet_wco_it40000", WCO, 43)
    e2e("e2e_pspnet_wcofo_it40000", WCOFO, 47)


if __name__ == "__main__":
    main()
