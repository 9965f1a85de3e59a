"""Backward of the per-stage kernel predictor with the weight gradients taken from passes that already read the maps
(csbsr_amd/modeling/kp_bwd.py, KBPN.kp_pairs):

* fe_cat.2: the weight gradient under a spatially constant dPre as a fold of the 16 border-class sums of the layer's input, and the
  entry point that takes those sums in the pass of the masked fill (csbsr_border_class_fill_masked_sums);
* fe_SR.1 / fe_cat.0: input gradient and weight gradient of the 1x1 layers from one kernel (csrc/conv_pair.hip) -- the input gradient
  bit-identical to Conv.bwd_input(mask=), the weight gradient against autograd and against Conv.bwd_weights;
* the whole backward with the attribute on and off.

Tolerances: 2e-3 of the tensor's maximum against autograd and 1e-3 between two kernels (test_conv_kernels_gpu.py, weight gradients); 1e-5
between two fixed-order fp32 sums of the same fp16 values (that file's mirrored-vs-plain comparison)."""
import types

import pytest
import torch
import torch.nn.functional as F

from golden_utils import load_golden
from test_conv_kernels_gpu import _eng, from_fm, relmax, to_fm

pytestmark = pytest.mark.gpu


def _mtap():
    from csbsr_amd.modeling.kbpn import border_tap_mask
    return border_tap_mask().cuda()


@pytest.mark.parametrize("H,W", [(9, 12), (1, 7), (16, 33), (3, 3)])
def test_constant_gradient_wgrad_fold(H, W):
    """kp_bwd.fold_const_wgrad (wgrad of fe_cat.2 behind the global average pool) against torch autograd of F.conv2d under the broadcast
    gradient, and against the MFMA weight-gradient kernels run on the broadcast FM."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, FM, pad8
    from csbsr_amd.modeling.kbpn import KBPN
    from csbsr_amd.modeling.kp_bwd import const_wgrad_ok, fold_const_wgrad
    torch.manual_seed(H * 100 + W)
    eng = _eng()
    N, cin, cout, slope = 2, 32, 49, 0.1
    w = (torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5).half().float()
    g = (torch.randn(N, cout) * 0.01).half().float()
    x = torch.randn(N, cin, H, W).half().float()
    wr = w.clone().requires_grad_(True)
    F.conv2d(x, wr, None, 1, 1).backward(g[:, :, None, None].expand(N, cout, H, W))
    # the fold, with the sums from the dgrad's fill pass as the model takes them
    pf = {"l.weight": w.clone().cuda()}
    conv = Conv(eng, "l", pf, 3, 1, 1, 1, bias=False, act=L.ACT_LRELU, slope=slope)
    assert const_wgrad_ok(conv)
    stub = types.SimpleNamespace(eng=eng, Mtap=_mtap())
    xfm = to_fm(eng, x)
    sums = torch.zeros(N, 16, xfm.cp, device="cuda")
    KBPN._fold_const_dgrad(stub, conv, g.cuda(), (xfm, slope), H, W, sums=sums)
    fold_const_wgrad(conv, g.cuda(), sums, stub.Mtap)
    # the MFMA kernels on the broadcast FM
    pm = {"l.weight": w.clone().cuda()}
    conv2 = Conv(eng, "l", pm, 3, 1, 1, 1, bias=False, act=L.ACT_LRELU, slope=slope)
    t = torch.zeros(N, 1, 1, pad8(cout), dtype=torch.float16, device="cuda")
    t[:, 0, 0, :cout] = g.cuda().half()
    conv2.bwd_weights(FM(t, cout, bcast=True, H=H, W=W), xfm)
    torch.cuda.synchronize()
    got, mfma = pf["l.weight"].gacc.cpu(), pm["l.weight"].gacc.cpu()
    print(f"{H}x{W}: fold vs autograd {relmax(got, wr.grad):.2e}, fold vs MFMA wgrad {relmax(got, mfma):.2e}")
    assert relmax(got, wr.grad) < 2e-3
    assert relmax(got, mfma) < 2e-3


# (the first four shapes take the entry point's small-map route; 32 x 32 = 1024 pixels is the first size of the one-pass kernel, 40 x 33 a
# ragged one with more than one chunk per sample and pixels per chunk that are no multiple of the lanes)
@pytest.mark.parametrize("H,W", [(9, 12), (1, 7), (16, 33), (3, 3), (32, 32), (40, 33)])
def test_fill_masked_sums_entry(H, W):
    """csbsr_border_class_fill_masked_sums against csbsr_border_class_fill_masked + csbsr_border_class_sums of the mask map"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import _ptr
    torch.manual_seed(H * 7 + W)
    eng = _eng()
    N, c, slope = 2, 32, 0.1
    V = torch.randn(N, 16, c, device="cuda")
    mfm = to_fm(eng, torch.randn(N, c, H, W).half().float())
    outs, sums = [], []
    for fused in (True, False):
        out = eng.new(N, H, W, c)
        s = torch.zeros(N, 16, c, device="cuda")
        if fused:
            L.call("csbsr_border_class_fill_masked_sums", _ptr(V), _ptr(out.t), out.ld, _ptr(mfm.t), mfm.ld, slope, _ptr(s), N, H, W, c, eng.stream)
        else:
            L.call("csbsr_border_class_fill_masked", _ptr(V), _ptr(out.t), out.ld, _ptr(mfm.t), mfm.ld, slope, N, H, W, c, eng.stream)
            L.call("csbsr_border_class_sums", _ptr(mfm.t), mfm.ld, _ptr(s), N, H, W, c, eng.stream)
        torch.cuda.synchronize()
        outs.append(out.t.cpu())
        sums.append(s.cpu())
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    print(f"{H}x{W}: class sums, one pass vs stand-alone {relmax(sums[0], sums[1]):.2e}")
    assert relmax(sums[0], sums[1]) < 1e-5
    # ... and they are the class sums: against a plain torch binning
    x = from_fm(mfm)
    ys, xs = torch.arange(H)[:, None], torch.arange(W)[None, :]
    cls = (ys == 0) * 8 + (ys == H - 1) * 4 + (xs == 0) * 2 + (xs == W - 1)
    ref = torch.stack([(x * (cls == k)).sum((2, 3)) for k in range(16)], 1)
    assert float((sums[0] - ref).abs().max()) < 1e-5 * max(1.0, float(x.abs().sum((2, 3)).max()))


@pytest.mark.parametrize("slope", [0.0, 0.1])
@pytest.mark.parametrize("N,H,W,cin_tot", [(3, 19, 45, 49), (3, 16, 64, 49), (3, 8, 32, 49), (3, 1, 7, 49), (3, 19, 45, 98),
                                           # 1104 tiles: every workgroup walks its ring of tile buffers round more than once, and the
                                           # map is large enough for bwd_input to run on the direct full-resolution kernel
                                           (2, 363, 371, 49)])
def test_pair_1x1_backward(N, H, W, cin_tot, slope):
    """csbsr_conv_pair1x1_backward (49 -> 32 channels; cin_tot 98: fe_cat.0's form, the gradient for the first 49 input columns only):
    dIn bit-identical to Conv.bwd_input(mask=), the weight gradient against autograd and Conv.bwd_weights, accumulating."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    from csbsr_amd.modeling.kp_bwd import pair1x1_backward, pair1x1_ok
    torch.manual_seed(H * 100 + W + cin_tot)
    eng = _eng()
    cin, cout = 49, 32
    split = (cin, cin_tot - cin) if cin_tot > cin else None
    w = (torch.randn(cout, cin_tot, 1, 1) / cin_tot ** 0.5).half().float()
    dpre = torch.randn(N, cout, H, W).half().float()
    x = torch.randn(N, cin, H, W).half().float()
    wr = w.clone().requires_grad_(True)
    F.conv2d(torch.cat((x, torch.zeros(N, cin_tot - cin, H, W)), 1), wr, None, 1, 0).backward(dpre)
    dfm, xfm = to_fm(eng, dpre), to_fm(eng, x)
    # today's two launches
    p0 = {"l.weight": w.clone().cuda()}
    c0 = Conv(eng, "l", p0, 1, 1, 0, 1, bias=False, act=L.ACT_NONE, split=split)
    ref_din = c0.bwd_input(dfm, seg=0, mask=(xfm, slope))
    torch.cuda.synchronize()
    assert ((L.load().csbsr_debug_last_conv_kernel() & 255) == 8) == (N * H * W >= 256 * 1024)      # (the direct kernel from 2^18 pixels)
    c0.bwd_weights(dfm, xfm, split_override=(cin, 0))
    # the pair kernel, twice
    p1 = {"l.weight": w.clone().cuda()}
    c1 = Conv(eng, "l", p1, 1, 1, 0, 1, bias=False, act=L.ACT_NONE, split=split)
    assert pair1x1_ok(c1, dfm, xfm)
    din = pair1x1_backward(c1, dfm, xfm, slope)
    torch.cuda.synchronize()
    g1 = p1["l.weight"].gacc.clone()
    din2 = pair1x1_backward(c1, dfm, xfm, slope)
    torch.cuda.synchronize()
    assert (din.c, din.cp) == (ref_din.c, ref_din.cp)
    nbad = int((din.t.view(torch.int16) != ref_din.t.view(torch.int16)).sum())
    g, gref = g1.cpu(), p0["l.weight"].gacc.cpu()
    print(f"{H}x{W} cin {cin_tot} slope {slope}: dIn elements that differ {nbad}; wgrad vs autograd {relmax(g, wr.grad):.2e}, vs bwd_weights {relmax(g, gref):.2e}")
    assert torch.equal(din.t, ref_din.t) and torch.equal(din2.t, ref_din.t)
    assert relmax(g, wr.grad) < 2e-3
    assert relmax(g, gref) < 1e-3
    assert torch.equal(p1["l.weight"].gacc, 2 * g1)
    if cin_tot > cin:           # the folded half's columns belong to another writer
        assert not bool(g[:, cin:].any())


PAIR_LAYERS = ("kernel_predictor.fe_SR.0.", "kernel_predictor.fe_SR.1.", "kernel_predictor.fe_cat.0.", "kernel_predictor.fe_cat.2.")


@pytest.mark.parametrize("case", ["e2e_pspnet_it40000", "e2e_blurskip_x8_it40000", "e2e_pspnet_it1"])
def test_whole_backward_with_and_without_pairs(case):
    from test_determinism_gpu import _step
    from test_joint_gpu import build_model
    g = load_golden(case)
    m, _ = build_model(g, 8)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    kb = m._runtime()["kbpn"]
    on = kb.kp_pairs
    assert on == 3          # both parts: the fe_cat.2 fold and the 1x1 pairs
    a = _step(m, g)
    m.load_state_dict(sd0)
    kb.kp_pairs = 0
    try:
        b = _step(m, g)
    finally:
        kb.kp_pairs = on
    assert set(a) == set(b)
    worst, n = 0.0, 0
    for k in a:
        if k.startswith("grad.") and k.endswith("weight") and any(l in k for l in PAIR_LAYERS):
            x, y = a[k].double(), b[k].double()
            worst = max(worst, float((x - y).norm() / y.norm()))
            n += 1
        else:
            assert torch.equal(a[k], b[k]), k            # the forward and every other gradient are untouched
    print(f"{case}: {n} weight gradients of the paired layers, worst relative L2 difference {worst:.2e}")
    # four per stage wherever the per-stage predictors take gradients: the joint phase of the PSPNet fixture.  (PSPNet_BlurSkip trains its
    # detector on a frozen KBPN, and iteration 1 lies in the SR pretraining phase, which runs without the predictors: no such gradient
    # exists there, and everything must be equal.)
    trains = m._kbpn_trains and kb.use_predictor
    want = sum(1 for st in kb.stages for c in (st.fe_sr[0], st.fe_sr[1], st.fe_cat[0], st.fe_cat[2]) if not c.frozen) if trains else 0
    assert want == (4 * len(kb.stages) if case == "e2e_pspnet_it40000" else 0)
    assert n >= want and worst < 1e-3
