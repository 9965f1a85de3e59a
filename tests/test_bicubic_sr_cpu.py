"""MODEL.SR="bicubic" (the paper's lower-bound row: the detector on the bicubically up-scaled LR image), host side: the NumPy restatement
of the up-scale against torch, construction without a GPU, the loss mixing, the validation bookkeeping and the reference fixture."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bicubic_cases as BC


def _cfg(**over):
    from csbsr_amd.config import cfg
    c = cfg.clone()
    c.MODEL.SR = "bicubic"
    for k, v in over.items():
        c.merge_from_list([k.replace("__", "."), v])
    return c


@pytest.mark.parametrize("antialias", [True, False])
@pytest.mark.parametrize("case", BC.KERNEL_CASES)
def test_restatement_matches_torch(case, antialias):
    """the fp64 restatement against torch's own fp32 resize on the CPU at every GPU case shape: 1e-6 absolute (fp32 against fp64)"""
    planes, H, W, s = case
    x = BC.case_input(*case)
    want = F.interpolate(torch.from_numpy(x)[None], size=(H * s, W * s), mode="bicubic", align_corners=False, antialias=antialias)[0]
    err = float(np.abs(BC.case_reference(planes, H, W, s, antialias) - want.double().numpy()).max())
    print(f"{case} antialias={antialias}: restatement vs torch {err:.2e}")
    assert err <= 1e-6
    # the two modes cannot be confused by a test
    assert float(np.abs(BC.case_reference(planes, H, W, s, True) - BC.case_reference(planes, H, W, s, False)).max()) > 1e-2


@pytest.mark.parametrize("detector", ["PSPNet", "HRNet_OCR"])
def test_bicubic_model_builds_with_the_detector_alone(detector):
    from csbsr_amd.config import cfg
    from csbsr_amd.modeling.build_model import JointModelWithLoss, JointModel
    kb = cfg.clone()
    kb.MODEL.DETECTOR_TYPE = detector
    want = [k for k in JointModelWithLoss(kb, 1000, 0, None).state_dict().keys() if k.startswith("segmentation_model.")]
    for m in (JointModelWithLoss(_cfg(MODEL__DETECTOR_TYPE=detector), 1000, 0, None), JointModel(_cfg(MODEL__DETECTOR_TYPE=detector))):
        assert m.sr_model == "bicubic"
        assert list(m.state_dict().keys()) == want
        names = [n for n, _ in m.named_parameters()]
        assert names and not any(n.startswith("sr_model") for n in names)
        assert sum(p.numel() for p in m.parameters()) == sum(v.numel() for k, v in m._named_full() if isinstance(v, torch.nn.Parameter))
        assert all(m._bucket_of(k) == "seg" for k, _ in m._named_full())


def test_bicubic_refusals_and_ignored_keys():
    from csbsr_amd.modeling.build_model import JointModelWithLoss, JointModel
    for cls, args in ((JointModelWithLoss, (1000, 0, None)), (JointModel, ())):
        with pytest.raises(NotImplementedError, match="bicubic"):
            cls(_cfg(MODEL__DETECTOR_TYPE="PSPNet_BlurSkip"), *args)
    with pytest.raises(NotImplementedError):
        JointModelWithLoss(_cfg(SOLVER__SEG_LOSS_FUNC="Dice"), 1000, 0, None)
    # the keys that only shape KBPN or the SR loss have no effect (build_model.py:163-166: calc_sr_loss returns before the loss function)
    base = list(JointModelWithLoss(_cfg(), 1000, 0, None).state_dict().keys())
    m = JointModelWithLoss(_cfg(SOLVER__SR_LOSS_FUNC="L1", SOLVER__SEG_FAIL_ORIENTED_WEIGHT4SR_AMP=1.0, SOLVER__ONLY_KERNEL_LOSS_FOR_PRETRAIN=True,
                                MODEL__KBPN_KERNEL_SFT=False, MODEL__SR_PIXEL_SHUFFLE=True, MODEL__NUM_STAGES=2), 1000, 0, None)
    assert list(m.state_dict().keys()) == base


def test_calc_loss_is_the_segmentation_mean():
    from csbsr_amd.config import cfg
    from csbsr_amd.trainer import calc_loss
    seg, sr = torch.tensor([0.5, 1.5, 4.0]), torch.tensor([3.0, 5.0, 10.0])
    for over in ({}, {"SOLVER__TASK_LOSS_WEIGHT": -1}):
        c = _cfg(**over)
        for it in (1, 30000, 30001, 40000, 200000):          # inside and outside SR_PRETRAIN_ITER = [1, 30001]
            assert float(calc_loss(seg, None, it, c)) == float(seg.mean())
            assert float(calc_loss(seg, sr, it, c)) == float(seg.mean())
    # KBPN: unchanged
    k = cfg.clone()
    assert float(calc_loss(seg, sr, 5, k)) == float(sr.mean())
    assert float(calc_loss(seg, sr, 40000, k)) == pytest.approx(0.7 * 6.0 + 0.3 * 2.0, rel=1e-6)
    k.SOLVER.TASK_LOSS_WEIGHT = -1
    w = min(1.0 / 140000 * (100000 - 30000), 1)
    assert float(calc_loss(seg, sr, 100000, k)) == pytest.approx((1 - w) * 6.0 + w * 2.0, rel=1e-6)


def test_validation_accumulator_takes_no_sr_loss():
    from csbsr_amd.trainer import ValidationAccumulator
    g = torch.Generator().manual_seed(5)
    batches = [(torch.rand(n, generator=g), *(torch.rand(n, generator=g) for _ in range(4))) for n in (4, 4, 3)]
    a, b = ValidationAccumulator(), ValidationAccumulator()
    for seg, ps, ss, kp, iou in batches:
        a.add(seg, None, ps, ss, kp, iou)
        b.add(seg, torch.zeros_like(seg), ps, ss, kp, iou)
    ra, rb = a.result(), b.result()
    assert ra["eval_sr_loss"] == 0.0
    assert ra == rb and set(ra) == {"eval_segment_loss", "eval_sr_loss", "psnr", "ssim", "kernel_psnr", "iou", "batches", "images"}


def test_fixture_sr_preds_are_the_restatement():
    """the reference's own sr_preds (torchvision Resize(BICUBIC), antialias on) against the restatement: 1e-6"""
    g = BC.fixture()
    assert int(g["B"]) == 1 and str(g["detector"]) == "PSPNet" and bool(g["antialias"]) and bool(g["eval_sr_is_clamped_sr"])
    assert not any(str(n).startswith("sr_model") for n in g["grad_names"])
    assert tuple(g["kernel_preds_shape"]) == g["kernel"].shape
    err = float(np.abs(BC.bicubic_up_ref(g["x"], int(g["scale"]), True) - g["sr_preds"].astype(np.float64)).max())
    print(f"fixture sr_preds vs restatement {err:.2e}")
    assert err <= 1e-6
    import os
    from golden_utils import GOLDEN
    assert os.path.getsize(os.path.join(GOLDEN, "bicubic_pspnet.npz")) <= os.path.getsize(os.path.join(GOLDEN, "wc_pspnet_it40000.npz"))
