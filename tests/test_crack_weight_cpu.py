"""SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP without a GPU: which models take the key, the C ABI of csbsr_crack_weight, and the tests' own
restatement of the weight against the reference-generated maps."""
import os
import re

import numpy as np
import pytest

import crack_weight_cases as CW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(*pairs):
    from csbsr_amd.config import cfg
    c = cfg.clone()
    c.merge_from_list(list(pairs))
    return c


def test_refusal_matrix():
    from csbsr_amd.modeling.build_model import JointModelWithLoss, SRModelWithLoss
    amp = 0.25
    # ORIENTED_WEIGHT_ITER = -1: KBPNLoss never applies an oriented weight, the key could not act -> refused, and the message says why
    with pytest.raises(NotImplementedError, match="ORIENTED_WEIGHT_ITER"):
        JointModelWithLoss(_cfg("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", amp), 1000, 0, None)
    m = JointModelWithLoss(_cfg("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", amp, "SOLVER.ORIENTED_WEIGHT_ITER", 100), 1000, 0, None)
    assert m.pc.co_sr_amp == amp and m.pc.oriented_w_iter == 100 and m.pc.sfo_sr_amp == 0.0
    m = JointModelWithLoss(_cfg("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", amp, "SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SR_AMP", 1.0,
                                "SOLVER.ORIENTED_WEIGHT_ITER", 0), 1000, 0, None)
    assert (m.pc.co_sr_amp, m.pc.sfo_sr_amp) == (amp, 1.0)
    assert JointModelWithLoss(_cfg(), 1000, 0, None).pc.co_sr_amp == 0.0
    # the SR-only model has no mask to take distances in
    with pytest.raises(NotImplementedError):
        SRModelWithLoss(_cfg("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", amp, "SOLVER.ORIENTED_WEIGHT_ITER", 100))
    # the segmentation-side weights stay refused, with the key on as well
    for key, val in (("SOLVER.SEG_FAIL_ORIENTED_WEIGHT4SS_AMP", 1.0), ("SOLVER.INTERM_SSLOSSWEGHT4SR", True)):
        for extra in ((), ("SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", amp, "SOLVER.ORIENTED_WEIGHT_ITER", 100)):
            with pytest.raises(NotImplementedError):
                JointModelWithLoss(_cfg(key, val, *extra), 1000, 0, None)
    # MODEL.SR = "bicubic" has no SR loss: accepted without effect where the reference's gate is open, refused like everywhere at -1
    b = JointModelWithLoss(_cfg("MODEL.SR", "bicubic", "SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", amp, "SOLVER.ORIENTED_WEIGHT_ITER", 100), 1000, 0, None)
    assert b.bicubic and b.pc.co_sr_amp == amp
    with pytest.raises(NotImplementedError):
        JointModelWithLoss(_cfg("MODEL.SR", "bicubic", "SOLVER.CRACK_ORIENTED_WEIGHT4SR_AMP", amp), 1000, 0, None)


def test_abi_matches_the_header():
    from csbsr_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "csbsr_hip.h")).read()
    decl = re.search(r"int\s+csbsr_crack_weight\s*\(([^)]*)\)\s*;", hdr)
    assert decl, "csbsr_crack_weight is not declared in include/csbsr_hip.h"
    ctype = {"const float*": L.vp, "float*": L.vp, "csbsr_stream_t": L.vp, "int32_t": L.i32, "float": L.f32}
    args = [ctype[" ".join(a.split()[:-1])] for a in decl.group(1).replace("\n", " ").split(",")]
    res, sig = L.SIGNATURES["csbsr_crack_weight"]
    assert res is L.i32 and sig == args and len(args) == 11


@pytest.mark.parametrize("tag,amp", CW.CASES)
def test_restatement_equals_the_reference_bit_for_bit(tag, amp):
    g = CW.maps()
    mask, ref = g[f"mask_{tag}"], g[f"w_hr_{tag}_{amp:g}"]
    got = CW.restated_weight(mask, amp)
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), int((got != ref).sum())


def test_fixture_holds_the_cases_it_is_meant_to():
    g = CW.maps()
    a, b = g["mask_a"], g["mask_b"]
    assert a.shape == (4, 1, 40, 300) and b.shape == (2, 1, 64, 64)
    fg = CW.foreground(a)
    assert 0.005 < fg[0].mean() < 0.02 and not fg[1].any() and fg[2].all()
    assert fg[3].sum() == 1 and fg[3, 0, 39, 299] and sorted(np.unique(a[3]).tolist()) == [0.0, 0.5, np.float32(0.99), 1.0]
    assert 0.25 < CW.foreground(b).mean() < 0.35
    for amp in (0.1, 2.0):
        w = g[f"w_hr_a_{amp:g}"]
        assert (w[1] == CW.LAMBDA).all() and (w[2] == CW.LAMBDA).all() and (w[0][fg[0]] == CW.LAMBDA).all()
        # the soft pixels are background: they carry the weight of their distance to the corner pixel, not lambda
        assert w[3, 0, 5, 7] < CW.LAMBDA and w[3, 0, 20, 150] < CW.LAMBDA and w[3, 0, 39, 299] == CW.LAMBDA
    w2 = g["w_hr_a_2"]
    assert (w2[3] == 0).any() and ((w2[3] > 0) & (w2[3] < CW.FLT_MIN)).any()      # amp 2 reaches the underflow region
