"""What a detector's backward reads belongs to ONE forward and lives on that forward's tape (``detector.saved``, csbsr_amd/modeling/blocks.py),
never on the shared layer objects: the train step moves the tape to its autograd node (build_model.py, ``psp_saved``), so a later forward
must not change an earlier forward's gradients and a dropped tape must free every activation.  Both detectors, at detector level
(``m._runtime()["psp"]``), HR 96x96 (the smallest size both trunks take), B = 2, both precisions, fixed dropout masks."""
import gc
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H = 2, 96
CASES = [(d, p) for d in ("PSPNet", "HRNet_OCR") for p in ("fp16", "split")]


@pytest.fixture(scope="module")
def models():
    """one model per detector for the whole module (built on first use, dropped with the module)"""
    built = {}
    yield built
    built.clear()


def _setup(models, detector, precision):
    from csbsr_amd.config import cfg as base_cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss
    from csbsr_amd.utils.detfill import deterministic_fill
    if detector not in models:
        cfg = base_cfg.clone()
        cfg.MODEL.DETECTOR_TYPE = detector
        m = JointModelWithLoss(cfg, 1000, 0, None)
        deterministic_fill(m.state_dict())
        m.train()
        models[detector] = m
    m = models[detector]
    m.detector_precision = precision
    rt = m._runtime()
    rt["eng"].grad_scale = float(2 ** round(np.log2(B * H * H)))
    rt["psp"].saved = None      # (whatever an earlier, failed test left)
    return rt, rt["eng"], rt["psp"]


def _sample(eng, det, seed, split):
    """one input with its dropout masks and backward seeds (a fixed random linear functional of the two maps, scaled)"""
    torch.manual_seed(seed)
    xin = eng.nchw32_to_fm(torch.randn(B, 3, H, H).cuda().contiguous(), split=split)
    r_seg, r_aux = (c * torch.randn(B, 1, H, H) / (H * H) * eng.grad_scale for c in (1.0, 0.4))
    return xin, det.make_dropout(B, True), r_seg.cuda().contiguous(), r_aux.cuda().contiguous()


def _backward(rt, eng, det, r_seg, r_aux):
    """-> (every gradient accumulator of the detector, d/d xin); the accumulators are zeroed again"""
    dxin = det.backward(r_seg, r_aux)
    eng.join_wgrad()
    torch.cuda.synchronize()
    out = rt["flat"]["seg"].clone(), dxin.t.clone()
    rt["flat"]["seg"].zero_()
    assert det.saved is None
    return out


@pytest.mark.parametrize("detector,precision", CASES)
def test_two_forwards_then_the_first_backward(models, detector, precision):
    """forward(A), forward(B), backward of A with A's tape, backward of B with B's: every output, accumulator and input gradient equals,
    bit for bit (the library is order-fixed), the same model running A alone and B alone, each forward followed by its backward."""
    rt, eng, det = _setup(models, detector, precision)
    rt["flat"]["seg"].zero_()
    A, Bs = (_sample(eng, det, seed, precision == "split") for seed in (11, 12))
    alone = []
    for xin, drop, r_seg, r_aux in (A, Bs):
        seg, aux = det.forward(xin, drop, True)
        alone.append((seg.clone(), aux.clone()) + _backward(rt, eng, det, r_seg, r_aux))
    fwd = []
    for xin, drop, _, _ in (A, Bs):
        seg, aux = det.forward(xin, drop, True)
        fwd.append((seg.clone(), aux.clone(), det.saved))
    assert fwd[0][2] is not fwd[1][2]
    for ref, (seg, aux, tape), (_, _, r_seg, r_aux) in zip(alone, fwd, (A, Bs)):
        det.saved = tape
        del tape
        got = (seg, aux) + _backward(rt, eng, det, r_seg, r_aux)
        assert all(bool(torch.isfinite(t).all()) for t in got)
        assert float(got[2].abs().max()) > 0 and float(got[3].abs().max()) > 0
        for name, g, r in zip(("seg", "aux", "parameter gradients", "d/d xin"), got, ref):
            assert torch.equal(g, r), (detector, precision, name, float((g.float() - r.float()).abs().max()))


@pytest.mark.parametrize("detector,precision", CASES)
def test_nothing_stays_on_the_layers(models, detector, precision):
    """Once the tape and the outputs are dropped no layer references the input map (so none references an activation): after an eval /
    no_grad forward, and after a training forward whose backward never runs (an SR-pretraining-phase iteration frees the detector's
    saves before the KBPN backward, build_model.py ``_hip_backward``)."""
    rt, eng, det = _setup(models, detector, precision)
    for training in (False, True):
        xin, drop, _, _ = _sample(eng, det, 13, precision == "split")
        ref = weakref.ref(xin.t)
        with torch.set_grad_enabled(training):
            out = det.forward(xin, drop if training else {k: None for k in det.drop_keys}, training=training)
        det.saved = None
        del out, xin
        gc.collect()
        assert ref() is None, (detector, precision, training)
