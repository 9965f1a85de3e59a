"""Shared by tests/test_crack_weight_cpu.py and tests/test_crack_weight_gpu.py: the fixture of the crack-oriented weight
(tests/golden/crack_weight_maps.npz, made by the reference: tests/golden/make_crack_weight_golden.py), a numpy / scipy restatement of the
weight, and the call of the kernel."""
import numpy as np

from golden_utils import load_golden

LAMBDA, SCALE = 2.0, 4
CASES = [(tag, amp) for tag in ("a", "b") for amp in (0.1, 2.0)]      # "a": (4,1,40,300), "b": (2,1,64,64)
FLT_MIN = float(np.finfo(np.float32).tiny)

_maps = None


def maps():
    global _maps
    if _maps is None:
        _maps = load_golden("crack_weight_maps")
        assert float(_maps["lambda"]) == LAMBDA and int(_maps["scale"]) == SCALE
    return _maps


def foreground(mask):
    """the reference's rule: the mask value truncated to uint8 is non-zero (0.5 and 0.99 are background)"""
    return mask.astype(np.uint8) != 0


def distance(mask):
    """[N,1,H,W] float64: exact Euclidean distance to the nearest foreground pixel of the sample; zeros for a sample without one"""
    from scipy.ndimage import distance_transform_edt
    fg = foreground(mask)
    d = np.zeros(mask.shape, np.float64)
    for n in range(mask.shape[0]):
        if fg[n].any():
            d[n, 0] = distance_transform_edt(~fg[n, 0])
    return d


def restated_weight(mask, amp, lam=LAMBDA):
    """lambda * exp(-amp * d) in fp32: the distance rounded to fp32, the product with fp32(-amp), then the exponential.  torch.exp is the
    reference's own exponential (numpy's fp32 exp may round the last bit differently), so the result can be held to it bit for bit."""
    import torch
    arg = np.float32(-amp) * distance(mask).astype(np.float32)
    return (np.float32(lam) * torch.exp(torch.from_numpy(arg)).numpy()).astype(np.float32)


def run_kernel(mask, amp, lam=LAMBDA, scale=SCALE, lr=True):
    """csbsr_crack_weight on cuda:0 -> (w_hr, w_lr) as numpy arrays"""
    import torch
    from csbsr_amd import _lib as L
    m = torch.from_numpy(np.ascontiguousarray(mask, np.float32)).cuda()
    N, _, H, W = m.shape
    w_hr = torch.empty_like(m)
    w_lr = torch.empty(N, 1, H // scale, W // scale, device=m.device) if lr else None
    scratch = torch.empty(N * H * W, device=m.device)
    L.call("csbsr_crack_weight", m.data_ptr(), w_hr.data_ptr(), w_lr.data_ptr() if lr else None, scratch.data_ptr(), N, H, W, float(amp),
           float(lam), scale, None)
    torch.cuda.synchronize()
    return w_hr.cpu().numpy(), (w_lr.cpu().numpy() if lr else None)
