"""SOLVER.DOWNSCALE_INTERPOLATION = 'area', host side (no GPU): the numpy restatement of the two kernel contracts (tests/area_cases.py)
against torch's own F.interpolate(mode='area') and its autograd, the ABI declaration, the config key from the tree to the model
constructors and the loaders, the trainer's data-against-loss check, and the conditions the reference fixtures were made under."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import area_cases as AC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("f", [2, 4, 8])
def test_restatement_is_torch_area_bit_for_bit(f):
    """f*f a power of two: the fp32 window sum taken row by row, left to right, divided by f*f IS F.interpolate(mode='area') on the CPU, and
    dy / (f*f) replicated IS its autograd -- bit for bit, on every shape the device test uses.  (An output of 1 x 1 per plane: see
    area_cases.torch_area -- torch's ``mean()`` shortcut for that size is within f*f * 2^-23 * max|x| of the loop, not equal to it.)"""
    for n, (planes, H, W) in enumerate(AC.kernel_shapes(f)):
        x = AC.random_input(planes, H, W, seed=100 * f + n)
        dy = AC.random_input(planes, H // f, W // f, seed=100 * f + n + 50)
        y, dx = AC.torch_area(x, f, dy)
        assert np.array_equal(AC.area_down(x, f).view(np.int32), y.view(np.int32)), (f, planes, H, W)
        assert np.array_equal(AC.area_down_bwd(dy, f).view(np.int32), dx.view(np.int32)), (f, planes, H, W)
        literal = F.interpolate(torch.from_numpy(x)[None], size=(H // f, W // f), mode="area")[0].numpy()
        assert float(np.abs(literal - y).max()) <= f * f * 2.0 ** -23 * float(np.abs(x).max())
        if (H // f, W // f) != (1, 1):
            assert np.array_equal(literal, y)


def test_restatement_by_hand():
    x = np.arange(2 * 4 * 6, dtype=np.float32).reshape(2, 4, 6)
    y = AC.area_down(x, 2)
    assert y.shape == (2, 2, 3) and y[0, 0, 0] == (0 + 1 + 6 + 7) / 4 and y[1, 1, 2] == (40 + 41 + 46 + 47) / 4
    d = AC.area_down_bwd(np.array([[[4.0, 8.0]]], np.float32), 2)
    assert d.tolist() == [[[1.0, 1.0, 2.0, 2.0], [1.0, 1.0, 2.0, 2.0]]]
    with pytest.raises(AssertionError):
        AC.area_down(np.zeros((1, 5, 4), np.float32), 2)


def test_header_and_signatures_declare_both_kernels():
    from csbsr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "int32_t": _lib.i32, "csbsr_stream_t": _lib.vp}
    for name, n_args in (("csbsr_area_down_fwd", 7), ("csbsr_area_down_bwd", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/csbsr_hip.h"
        declared = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.i32 and len(args) == n_args and list(args) == declared, name
    assert "image_ops.hip" in open(os.path.join(ROOT, "csbsr_amd", "csrc", "Makefile")).read()
    src = open(os.path.join(ROOT, "csbsr_amd", "csrc", "image_ops.hip")).read()
    assert 'extern "C" int csbsr_area_down_fwd(' in src and 'extern "C" int csbsr_area_down_bwd(' in src


# ------------------------------------------------------------------------------------------------------------------ config
def _cfg(**kv):
    from csbsr_amd.config import cfg
    c = cfg.clone()
    for k, v in kv.items():
        c.merge_from_list([k.replace("__", "."), v])
    return c


def test_path_config_reads_the_key():
    from csbsr_amd.config import path_config
    assert path_config(_cfg()).downscale == "bicubic"
    assert path_config(_cfg(SOLVER__DOWNSCALE_INTERPOLATION="area")).downscale == "area"


def test_models_carry_the_key_and_refuse_unknown_values():
    from csbsr_amd.modeling.build_model import JointModelWithLoss, SRModelWithLoss, JointModel
    area = _cfg(SOLVER__DOWNSCALE_INTERPOLATION="area")
    assert JointModelWithLoss(_cfg(), 1000, 0, None).downscale == "bicubic" and SRModelWithLoss(_cfg()).downscale == "bicubic"
    assert JointModelWithLoss(area, 1000, 0, None).downscale == "area" and SRModelWithLoss(area).downscale == "area"
    # no SR loss: the key is accepted and has no effect, as in the reference
    JointModel(area)
    JointModelWithLoss(_cfg(SOLVER__DOWNSCALE_INTERPOLATION="area", MODEL__SR="bicubic"), 1000, 0, None)
    for bad in ("bilinear", "Area", "nearest", None):
        c = _cfg(SOLVER__DOWNSCALE_INTERPOLATION=bad)
        for build in (lambda: JointModelWithLoss(c, 1000, 0, None), lambda: SRModelWithLoss(c), lambda: JointModel(c)):
            with pytest.raises(NotImplementedError):
                build()


class _Resize:          # what arrives as ``sr_transforms`` under csbsr_amd.dropin: the reference's FactorResize carries .interpolation
    def __init__(self, interpolation):
        self.factor, self.interpolation = 4, interpolation


def test_a_contradicting_sr_transforms_is_refused():
    import enum
    from csbsr_amd.modeling.build_model import JointModelWithLoss, SRModelWithLoss

    class InterpolationMode(enum.Enum):          # torchvision's enum, restated: FactorResize('bicubic') holds BICUBIC
        BICUBIC = "bicubic"
    area = _cfg(SOLVER__DOWNSCALE_INTERPOLATION="area")
    for build in (lambda c, t: JointModelWithLoss(c, 1000, 0, t), lambda c, t: SRModelWithLoss(c, t)):
        assert build(area, _Resize("area")).downscale == "area"
        assert build(_cfg(), _Resize(InterpolationMode.BICUBIC)).downscale == "bicubic"
        assert build(_cfg(), _Resize("bicubic")).downscale == "bicubic"
        assert build(area, object()).downscale == "area"          # nothing to compare with
        with pytest.raises(ValueError):
            build(area, _Resize(InterpolationMode.BICUBIC))
        with pytest.raises(ValueError):
            build(_cfg(), _Resize("area"))


# ------------------------------------------------------------------------------------------------------------------ loaders
def test_loaders_keep_the_name_and_refuse_unknown_ones():
    from csbsr_amd.data.degrade import DeviceDegradation
    from csbsr_amd.data import resident as R
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, size=(40, 48, 3), dtype=np.uint8) for _ in range(3)]
    masks = [rng.integers(0, 2, size=(40, 48), dtype=np.uint8) * 255 for _ in range(3)]
    ds = R.ResidentDataset(images, masks, device="cpu")
    assert DeviceDegradation(4, device="cpu").interpolation == "bicubic"
    assert DeviceDegradation(4, device="cpu", interpolation="area").interpolation == "area"
    bic = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=2, seed=5)
    area = R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=2, seed=5, interpolation="area")
    assert (bic.interpolation, bic.deg.interpolation, area.interpolation, area.deg.interpolation) == ("bicubic", "bicubic", "area", "area")
    for bad in ("bilinear", "AREA", None):
        with pytest.raises(ValueError):
            DeviceDegradation(4, device="cpu", interpolation=bad)
        with pytest.raises(ValueError):
            R.DeviceTrainLoader(ds, (24, 32), 4, batch_size=2, interpolation=bad)
    # the name changes no draw and no state
    for _ in range(3):
        (s1, p1), (s2, p2) = bic.draw(), area.draw()
        assert torch.equal(s1, s2) and torch.equal(p1, p2)
    st1, st2 = bic.state_dict(), area.state_dict()
    assert st1.keys() == st2.keys() and all(torch.equal(torch.as_tensor(st1[k]), torch.as_tensor(st2[k])) for k in st1 if st1[k] is not None)
    # from_cfg hands the key on
    c = _cfg(SOLVER__DOWNSCALE_INTERPOLATION="area", INPUT__IMAGE_SIZE=[24, 32])
    assert R.DeviceTrainLoader.from_cfg(c, ds, seed=0).interpolation == "area"
    assert R.DeviceTrainLoader.from_cfg(_cfg(INPUT__IMAGE_SIZE=[24, 32]), ds, seed=0).interpolation == "bicubic"


# ------------------------------------------------------------------------------------------------------------------ trainer
class _Model:
    def __init__(self, downscale):
        self.downscale = downscale


class _Loader:
    def __init__(self, interpolation):
        self.interpolation = interpolation

    def __iter__(self):
        raise AssertionError("the check comes before the first batch")


def test_trainer_refuses_data_and_loss_that_disagree():
    from csbsr_amd import trainer as T
    cfg = _cfg()
    for model, loader in ((_Model("area"), _Loader("bicubic")), (_Model("bicubic"), _Loader("area"))):
        with pytest.raises(ValueError):
            T.do_train(cfg, model, None, None, loader)
        with pytest.raises(ValueError):
            T.do_train(cfg, model, None, None, [], _Loader(loader.interpolation))          # the eval loader is checked too
        with pytest.raises(ValueError):
            T.do_pretrain_sr(cfg, model, None, None, loader)
        with pytest.raises(ValueError):
            T.validate(model, loader, 1)
        with pytest.raises(ValueError):
            T.validate_sr(model, loader, 1)
    # agreement, a loader without the attribute and a model without it pass the check
    T.check_downscale_agrees(_Model("area"), _Loader("area"), None, [], object())
    T.check_downscale_agrees(object(), _Loader("area"))


# ------------------------------------------------------------------------------------------------------------------ fixtures
def test_fixture_pseudo_lr_is_the_restatement_of_the_blurred_sr_image():
    """lr_pred of the it1 fixture is FactorResize('area') of the per-sample blur of its own sr_preds (sr_loss_functions.py:84-102).  The blur
    is recomputed here with torch's conv2d; a CPU may sum its 441 products in another order than the one the fixture was made on, so the
    comparison allows K*K * 2^-24 * max|sr| (each of the K*K roundings of a sum of magnitude <= max|sr|; the area mean adds none beyond
    one more rounding of the same size)."""
    g = AC.load_fixture("e2e_pspnet_area_it1")
    sr, w = torch.from_numpy(g["sr_preds"]), torch.from_numpy(g["kernel_preds"])
    K = w.shape[-1]
    blurred = torch.cat([F.conv2d(sr[b:b + 1], w[b].expand(3, 1, K, K), padding=(K - 1) // 2, groups=3) for b in range(sr.shape[0])])
    want = AC.area_down(blurred.numpy(), int(g["scale"]))
    bound = (K * K + 1) * 2.0 ** -24 * float(sr.abs().max())
    err = float(np.abs(want.astype(np.float64) - g["lr_pred"]).max())
    print(f"lr_pred vs restatement(blur(sr_preds)): max |diff| {err:.2e} (bound {bound:.2e}), bit-equal: {np.array_equal(want, g['lr_pred'])}")
    assert want.shape == g["lr_pred"].shape and err <= bound
    # and it is NOT the bicubic pseudo-LR
    assert float(np.abs(g["ctl_lr_pred"] - g["lr_pred"]).max()) > 100 * bound


def test_fixture_conditions():
    g1, g2 = AC.load_fixture("e2e_pspnet_area_it1"), AC.load_fixture("e2e_pspnet_area_it40000")
    # no sign of the LR term's gradient can flip within ten times csbsr_blur_fwd's bound
    assert float(g1["min_abs_lr_diff"]) >= 1e-4
    assert float(np.abs(g1["lr_pred"] - g1["x"]).min()) == float(g1["min_abs_lr_diff"])
    assert 1121 <= int(g1["seed"]) < 1121 + 32 and int(g1["seed"]) == int(g2["seed"])
    for g, it in ((g1, 1), (g2, 40000)):
        assert int(g["it"]) == it and str(g["downscale"]) == "area" and g["x"].shape == (2, 3, 16, 16) and g["hr"].shape == (2, 3, 64, 64)
        assert len(g["grad_names"]) == len(g["grad_norms"]) == len(g["grad_samples"]) == len(g["grad_samples32"])
        assert os.path.getsize(os.path.join(AC.GOLDEN, f"e2e_pspnet_area_it{it}.npz")) < (1 << 19)
    assert float(g2["alpha"]) == 0.7
    for k in ("dsr", "ctl_dsr"):
        assert g1[k].shape == g1["sr_preds"].shape
    for k in ("dkpred", "ctl_dkpred"):
        assert g1[k].shape == g1["kernel_preds"].shape
    assert not np.array_equal(g1["dsr"], g1["ctl_dsr"]) and not np.array_equal(g1["sr_loss"], g1["ctl_sr_loss"])
    # x IS the area down-scale: in [0, 1], and every sample of the two fixtures is the same input
    assert np.array_equal(g1["x"], g2["x"]) and g1["x"].min() >= 0 and g1["x"].max() <= 1
