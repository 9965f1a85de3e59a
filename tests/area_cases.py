"""The numpy restatement of csbsr_area_down_fwd / csbsr_area_down_bwd as include/csbsr_hip.h states them, and the shapes the device test
runs them on.

    y[p,oy,ox]  = (sum_{a<f} sum_{b<f} x[p, oy*f+a, ox*f+b]) / (f*f)      one fp32 chain, a outer and b inner, then ONE division
    dx[p,iy,ix] = dy[p, iy/f, ix/f] / (f*f)

Every operation below is an fp32 operation on fp32 arrays (numpy keeps float32 + float32 in float32), in exactly that order."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

def kernel_shapes(f):
    """(planes, H, W) per factor f: one output per plane; a few rows of a narrow image; 65 outputs per row (one lane past a wave) on 36
    rows -- 40 at f = 8, the next multiple of the factor: 36 x 520 is no legal input there."""
    return [(6, f, f), (6, 32, 40), (6, -(-36 // f) * f, 65 * f)]


def torch_area(x, f, dy=None):
    """F.interpolate(mode='area') of fp32 planes [P,H,W] on the CPU -> y [P,H/f,W/f], and with ``dy`` also its autograd's dx.

    One detour: for an output of 1 x 1 per plane torch does not run its pooling loop at all -- adaptive_avg_pool2d hands that size to
    ``mean()``, whose vectorised reduction adds in another order (f = 4, 8: the last bit differs on most planes; measured 3e-8).  The
    windows of an area resize do not interact, so there the planes are laid side by side as ONE image of H x (P*W): the same windows, the
    same operator, its pooling loop."""
    import torch
    import torch.nn.functional as F
    P, H, W = x.shape
    t = torch.from_numpy(np.ascontiguousarray(x)).requires_grad_(dy is not None)
    if (H // f, W // f) == (1, 1):
        img = t.permute(1, 0, 2).reshape(1, 1, H, P * W)
        y = F.interpolate(img, size=(1, P), mode="area").reshape(1, P, 1).permute(1, 0, 2)
    else:
        y = F.interpolate(t[None], size=(H // f, W // f), mode="area")[0]
    if dy is None:
        return y.numpy()
    y.backward(torch.from_numpy(np.ascontiguousarray(dy)))
    return y.detach().numpy(), t.grad.numpy()


WRAP_CASE = (3, 1700, 1704, 2)          # 2.17 M outputs (and float4s of dx) > 8192 x 256 threads: the grid-stride loop wraps
WRAP_CASE_TWO_PER_LANE = (6, 1700, 1704, 2)      # ... and still does where a lane of the f = 2 forward owns two outputs


def area_down(x, f):
    x = np.asarray(x, dtype=np.float32)
    H, W = x.shape[-2:]
    assert f >= 1 and H % f == 0 and W % f == 0
    acc = np.zeros(x.shape[:-2] + (H // f, W // f), dtype=np.float32)
    for a in range(f):
        for b in range(f):
            acc = acc + x[..., a::f, b::f]
            assert acc.dtype == np.float32
    return acc / np.float32(f * f)


def area_down_bwd(dy, f):
    dy = np.asarray(dy, dtype=np.float32)
    g = dy / np.float32(f * f)
    return np.repeat(np.repeat(g, f, axis=-2), f, axis=-1)


def random_input(planes, H, W, seed):
    """fp32 values in [-1.2, 1.2) with full mantissas (a sum in another order differs in the last bits)"""
    rng = np.random.default_rng(seed)
    return ((rng.random((planes, H, W)) * 2.4 - 1.2)).astype(np.float32)


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
