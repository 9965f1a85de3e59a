"""Adam on the device, hand-written: the optimiser step of the reference's training loop -- ``torch.optim.Adam(params, lr, betas=(0.9, 0.999),
eps=1e-8)``, /root/reference/train.py:91, no weight decay, no amsgrad -- as ONE multi-tensor HIP launch per parameter group
(``csbsr_adam_step``, csrc/multi_tensor.hip) instead of torch's foreach kernels (52 launches, 3 ms per config-2 step; the last vendor /
torch arithmetic on the timed path besides a few [B, 441] einsums).

Drop-in for ``torch.optim.Adam`` in that configuration: a ``torch.optim.Optimizer`` subclass (``LambdaLR`` and the reference's warm-up schedulers
work on it unchanged), the same per-parameter state keys (``step``, ``exp_avg``, ``exp_avg_sq``: ``state_dict()`` interchanges with
``torch.optim.Adam``), the same skip rule (a parameter whose ``.grad`` is None is not touched: no moment decay, no step count -- what the frozen
training phases and an overflowed backward rely on), the same arithmetic operation by operation (agreement to fp32 rounding:
tests/test_elementwise_gpu.py::test_adam_step_matches_torch).  fp32 parameters on the device only; anything else raises.

``SGD`` is the same for ``torch.optim.SGD(params, lr, momentum=0.9, weight_decay=5e-4)`` (train.py:93, MODEL.OPTIMIZER "SGD"): one
``csbsr_sgd_step`` launch per group over the same chunk map and staging table (csbsr_amd/multi_tensor.py), torch's state key
``momentum_buffer``, torch's skip rule, and a ``state_dict()`` that ``torch.optim.SGD`` loads and steps from
(tests/test_trainer_gpu.py::test_sgd_step_matches_torch).
"""
import math

import numpy as np
import torch

from . import _lib as L
from . import multi_tensor as MT

_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("step_size", "<f4"), ("bc2_sqrt", "<f4")])
assert _DT.itemsize == 48
_SGD_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("buf", "<u8"), ("n", "<i8"), ("vec", "<i4"), ("pad", "<i4")])
assert _SGD_DT.itemsize == 40


class _MultiTensor(torch.optim.Optimizer):
    """What the one-launch optimisers share: one pinned staging of the per-step table per parameter group (csbsr_amd/multi_tensor.py)."""

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        L.load()
        self._host = {}          # group index -> Staging of its per-step table

    def _launch(self, name, slot, tab, ps, dev, *scalars):
        """Upload ``tab`` (one row per tensor of ``ps``, the stepped tensors of group ``slot``) and run entry point ``name`` over the chunk
        map of ``ps`` on the current stream."""
        if slot not in self._host or self._host[slot].device != dev:
            self._host[slot] = MT.Staging(dev)
        MT.launch(name, self._host[slot], tab.view(np.uint8), [p.numel() for p in ps], dev, *scalars)


def _check(p, g, dev, who):
    if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and g.dtype == torch.float32 and not g.is_sparse
            and g.is_contiguous() and g.device == p.device == dev):
        raise L.CsbsrHipError(f"csbsr_amd.optim.{who}: contiguous fp32 parameters and gradients on one device only")


def _check_aligned(i, **tensors):
    """csbsr_adam_step moves float4s and its table has no ``vec`` flag (csbsr_hip.h): a view that starts inside an allocation is refused"""
    for name, t in tensors.items():
        if t is not None and t.data_ptr() % 16 != 0:
            raise L.CsbsrHipError(f"csbsr_amd.optim.Adam: {name} of parameter {i} (shape {tuple(t.shape)}) is not 16-byte aligned "
                                  f"(a view that starts inside an allocation?): csbsr_adam_step needs 16-byte aligned p, g, exp_avg and exp_avg_sq")


class Adam(_MultiTensor):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("invalid Adam hyper-parameters")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for slot, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            beta1, beta2 = group["betas"]
            lr = float(group["lr"])
            dev = ps[0].device
            tab = np.zeros(len(ps), dtype=_DT)
            for i, p in enumerate(ps):          # (before any state is created or a step count advances: a refused step changes nothing)
                st = self.state.get(p, {})
                _check_aligned(i, p=p, grad=p.grad, exp_avg=st.get("exp_avg"), exp_avg_sq=st.get("exp_avg_sq"))
            for i, p in enumerate(ps):
                g = p.grad
                _check(p, g, dev, "Adam")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                _check(p, st["exp_avg"], dev, "Adam")          # (a state_dict loaded while the parameters were still on the host)
                _check(p, st["exp_avg_sq"], dev, "Adam")
                st["step"] += 1
                t = float(st["step"])
                tab[i] = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                          lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t))
            self._launch("csbsr_adam_step", slot, tab, ps, dev, float(beta1), float(beta2), float(group["eps"]))
        return loss


class SGD(_MultiTensor):
    """``torch.optim.SGD(params, lr, momentum, weight_decay=...)`` as one launch per group.  ``dampening``, ``nesterov`` and ``maximize`` are
    accepted only at torch's defaults (they are carried in the group so that ``torch.optim.SGD`` can load this optimiser's state_dict and
    step from it); any other value is a ValueError, at construction and again at a step that finds one loaded from a state_dict."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize=False):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("invalid SGD hyper-parameters")
        self._refuse(dict(dampening=dampening, nesterov=nesterov, maximize=maximize))
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=False, maximize=False,
                                      foreach=None, differentiable=False, fused=None))

    @staticmethod
    def _refuse(group):
        if group.get("nesterov") or group.get("dampening", 0) != 0 or group.get("maximize"):
            raise ValueError("csbsr_amd.optim.SGD: nesterov, dampening != 0 and maximize are not built")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for slot, group in enumerate(self.param_groups):
            self._refuse(group)
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            momentum = float(group["momentum"])
            dev = ps[0].device
            tab = np.zeros(len(ps), dtype=_SGD_DT)
            for i, p in enumerate(ps):
                g = p.grad
                _check(p, g, dev, "SGD")
                ptrs = [p.data_ptr(), g.data_ptr(), 0]
                if momentum != 0:
                    st = self.state[p]
                    if st.get("momentum_buffer") is None:      # zeros: the kernel's first step then leaves buf = d, torch's clone
                        st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    buf = st["momentum_buffer"]
                    _check(p, buf, dev, "SGD")
                    ptrs[2] = buf.data_ptr()
                tab[i] = (*ptrs, p.numel(), int(all(a % 16 == 0 for a in ptrs)), 0)
            self._launch("csbsr_sgd_step", slot, tab, ps, dev, float(group["lr"]), momentum, float(group["weight_decay"]))
        return loss
