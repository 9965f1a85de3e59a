"""GPU parity of the MFMA convolution kernels (forward, dgrad, wgrad) through the C ABI against
torch fp32 CPU ops on the same fp16-rounded operands.  Tolerance: fp16 output rounding (2^-11) plus fp32
accumulation-order noise -> 2e-3 relative to the tensor's max magnitude."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _eng():
    from csbsr_amd.engine import Engine
    return Engine("cuda:0")


def to_fm(eng, x):        # NCHW fp32 cpu -> FM
    from csbsr_amd.engine import FM, pad8
    N, C, H, W = x.shape
    t = torch.zeros(N, H, W, pad8(C), dtype=torch.float16)
    t[..., :C] = x.permute(0, 2, 3, 1).half()
    return FM(t.cuda(), C)


def from_fm(fm):
    return fm.t[..., :fm.c].float().cpu().permute(0, 3, 1, 2)


def relmax(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-20))


CASES = [
    # cin, cout, k, stride, pad, dil, transposed, H, W
    (16, 32, 3, 1, 1, 1, False, 9, 11),
    (3, 49, 3, 1, 1, 1, False, 12, 12),
    (128, 128, 3, 1, 1, 1, False, 16, 16),
    (64, 128, 3, 1, 2, 2, False, 14, 10),
    (40, 24, 1, 1, 0, 1, False, 10, 10),
    (3, 64, 7, 2, 3, 1, False, 32, 32),
    (64, 128, 3, 2, 1, 1, False, 16, 16),
    (128, 128, 8, 4, 2, 1, False, 32, 32),
    (128, 128, 8, 4, 2, 1, True, 8, 8),
    (3, 128, 8, 4, 2, 1, True, 8, 8),
    (24, 16, 12, 8, 2, 1, True, 4, 4),
    (24, 16, 12, 8, 2, 1, False, 32, 32),
    (200, 136, 3, 1, 1, 1, False, 8, 8),
    (32, 32, 3, 1, 1, 1, False, 40, 70),           # streaming small-channel kernel, ragged 64-pixel strips
    (49, 49, 3, 1, 1, 1, False, 17, 64),           # two cout tiles, channel padding 49 -> 56
    (56, 32, 1, 1, 0, 1, False, 12, 128),          # 1x1
    (64, 128, 3, 1, 1, 1, False, 192, 190),        # > 65536 pixels: the 256x128 LDS-DMA kernel, ragged last tile
    (128, 192, 8, 4, 2, 1, True, 96, 96),          # LDS-DMA kernel, transposed, two cout tiles (second one half empty)
    (128, 3, 3, 1, 1, 1, False, 20, 24),           # 3-channel image head (kb.sr_reconst): taps-in-rows wgrad kernel
    (200, 3, 3, 1, 1, 1, False, 9, 70),            # same, two input-channel tiles, ragged
    (64, 2, 3, 1, 1, 1, False, 8, 8),
    (32, 32, 3, 1, 1, 1, False, 130, 140),         # small-channel HR kernel (>= 128x128 pixels), ragged tiles
    (49, 49, 3, 1, 1, 1, False, 129, 131),         # channel padding 49 -> 56: K steps straddle taps
    (32, 49, 1, 1, 0, 1, False, 128, 160),         # 1x1
    (56, 24, 3, 1, 1, 1, False, 128, 128),
    (3, 128, 3, 1, 1, 1, False, 20, 24),           # 3-channel image in (dgrad side of the heads): dense-K kernel
    (2, 200, 3, 1, 1, 1, False, 9, 70),            # ragged tile, last cout tile partial
    (128, 128, 12, 8, 2, 1, True, 8, 8),           # x8 KBPN up-projection (config 5): 64 phases, 4 taps each
    (128, 128, 12, 8, 2, 1, False, 64, 64),        # x8 down-projection: 144 taps (> the 64-bit tap mask)
    (64, 505, 3, 1, 1, 1, False, 20, 24),          # blur_skip conv_scale.0 feature part (cout padded 505 -> 512)
    (505, 64, 3, 1, 1, 1, False, 20, 24),          # blur_skip conv_scale.1 (cin padded 505 -> 512)
    (128, 128, 8, 4, 2, 1, False, 256, 256),       # strided gather: 2-D pixel tiles, residue-grouped tap order; wgrad tap order + row shift
    (256, 128, 3, 1, 1, 1, False, 192, 192),       # 256x128 LDS-DMA tile with 2-D (16 x 16) pixel tiles
    (128, 128, 8, 4, 2, 1, False, 768, 768),       # the same strided gather on the 256x128 tile (> 65536 output pixels)
    (768, 128, 3, 1, 1, 1, False, 24, 24),         # 6912 wgrad columns: the 128 x 256 eight-wave wgrad tile
    (256, 256, 3, 1, 1, 1, False, 192, 192),       # 256 px x 256 cout LDS-DMA tile (two staged epilogue passes), 2-D pixel tiles
    (264, 505, 3, 1, 1, 1, False, 190, 194),       # the same with a partly empty second cout tile, ragged pixel tiles, K padding
    (64, 64, 3, 1, 1, 1, False, 40, 70),           # 64-cout LDS-DMA tile (33..64 couts, input channels a multiple of 64), ragged pixel tiles
    (128, 49, 3, 1, 2, 2, False, 14, 18),          # the same, dilated, couts padded 49 -> 56 (dgrad: 128 couts from 64 padded channels -> general kernel)
    (256, 64, 1, 1, 0, 1, False, 32, 48),          # 1x1, 2-D pixel tiles off
    (128, 64, 8, 4, 2, 1, True, 12, 8),            # transposed into 64 couts: 16 phases on the 64-cout tile
    (64, 64, 3, 2, 1, 1, False, 48, 64),           # strided; its dgrad is a gather-form transposed conv on the 64-cout tile
    (48, 48, 3, 1, 1, 1, False, 40, 44),           # HRNet-W48 branch widths: the LDS-DMA kernels' general K walk (a 64-wide K slice straddles taps)
    (96, 96, 3, 1, 1, 1, False, 24, 40),
    (48, 96, 3, 2, 1, 1, False, 40, 40),           # transition / fuse layers between the branches (strided; dgrad = gather-form transposed conv)
    (96, 48, 1, 1, 0, 1, False, 24, 24),
    (720, 512, 3, 1, 1, 1, False, 20, 24),         # the 720-channel concat of the four branches into the OCR head's 3x3 conv
    (720, 720, 1, 1, 0, 1, False, 24, 24),
    (40, 72, 3, 1, 1, 1, False, 24, 24),           # 40 channels: five 8-channel units per tap
    (3, 64, 7, 2, 3, 1, False, 192, 256),          # PSPNet stem at a size whose dgrad (64 -> 3, 4x4 taps per phase) takes conv_thin_tpd
    (3, 64, 3, 2, 1, 1, False, 200, 168),          # HRNet stem (2x2 taps per phase), ragged 16 x 32 output tiles
    (2, 64, 7, 2, 3, 1, False, 130, 258),          # two image channels, tiles ragged in both directions
]


@pytest.mark.parametrize("case", CASES)
# wgrad: default (LDS-DMA kernel for every eligible problem: 128x128 / 128x256 / 256x256 tiles) | register-staged, scalar LDS transposition |
# register-staged, hardware transpose | LDS-DMA 256x256 tiles where eligible, register-staged elsewhere
# ... | the 128 x 256 tap-pair wgrad tile for the 8x8 stride-4 layers instead of the 128 x 512 four-tap one (bit 23)
@pytest.mark.parametrize("use_tr", [1, 0, 129, 1025, 1 | (1 << 23)])
def test_conv_fwd_dgrad_wgrad(case, use_tr):
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    cin, cout, k, s, p, d, tr, H, W = case
    L.load().csbsr_debug_set_wgrad_tr(use_tr)
    torch.manual_seed(hash(case) % 1000)
    eng = _eng()
    N = 2
    x = torch.randn(N, cin, H, W).half().float()
    wshape = (cin, cout, k, k) if tr else (cout, cin, k, k)
    w = (torch.randn(wshape) / (cin * k * k) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    params = {"l.weight": w.cuda(), "l.bias": b.cuda()}
    conv = Conv(eng, "l", params, k, s, p, d, transposed=tr, bias=True, act=L.ACT_LRELU, slope=0.1)
    y = conv.fwd(to_fm(eng, x))
    if tr:
        ref_pre = F.conv_transpose2d(x, w, b, s, p)
    else:
        ref_pre = F.conv2d(x, w, b, s, p, d)
    ref = F.leaky_relu(ref_pre, 0.1)
    torch.cuda.synchronize()
    assert tuple(from_fm(y).shape) == tuple(ref.shape)
    assert relmax(from_fm(y), ref) < 2e-3
    # dgrad / wgrad for a random dPre
    dpre = torch.randn_like(ref_pre).half().float()
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    out = F.conv_transpose2d(xr, wr, None, s, p) if tr else F.conv2d(xr, wr, None, s, p, d)
    out.backward(dpre)
    dfm = to_fm(eng, dpre)
    dx = conv.bwd_input(dfm, in_hw=(H, W))
    conv.bwd_weights(dfm, to_fm(eng, x))
    torch.cuda.synchronize()
    assert relmax(from_fm(dx), xr.grad) < 2e-3
    assert relmax(params["l.weight"].gacc.cpu(), wr.grad) < 2e-3
    L.load().csbsr_debug_set_wgrad_tr(1)


@pytest.mark.parametrize("shape", [
    # cin, cout, k, stride, pad, transposed, H, W  -- one launch per kernel family whose epilogue is the straight-line row of conv_common.h
    (128, 128, 3, 1, 1, False, 16, 16),            # LDS-DMA 128 x 128 tile
    (256, 256, 3, 1, 1, False, 192, 192),          # 256 px x 256 cout tile
    (832, 384, 3, 1, 1, False, 64, 64),            # conv_x3<3, 1024>
    (128, 128, 8, 4, 2, False, 256, 256),          # conv_x3<2, 1024>
    (16, 32, 3, 1, 1, False, 9, 11),               # register-staged kernel
])
@pytest.mark.parametrize("act", ["relu", "prelu", "none"])
def test_non_finite_accumulators_reach_the_output(shape, act):
    """an overflowed (inf / NaN) accumulator must leave the epilogue non-finite -- the optimiser's overflow check
    (modeling/build_model.py: isfinite over the gradient accumulators) only sees what the dgrad chain hands on.  Round 4's
    max(t, 0) + s * min(t, 0) activation turned NaN into 0 (maxnum / minnum return the non-NaN operand)."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    cin, cout, k, s, p, tr, H, W = shape
    torch.manual_seed(5)
    eng = _eng()
    x = torch.randn(1, cin, H, W).half().float() * 0.1
    w = torch.randn(cout, cin, k, k) / (cin * k * k) ** 0.5
    params = {"l.weight": w.cuda(), "l.slope": torch.tensor([0.25]).cuda()}
    a = {"relu": L.ACT_RELU, "prelu": L.ACT_PRELU, "none": L.ACT_NONE}[act]
    conv = Conv(eng, "l", params, k, s, p, 1, bias=False, act=a, prelu="l.slope" if act == "prelu" else False)
    OH, OW = conv.out_size(H, W)
    for bad in (float("nan"), float("inf"), float("-inf")):
        xb = x.clone()
        xb[0, 1, H // 2, W // 2] = bad                       # one poisoned input element: every output its taps reach must be non-finite
        y = from_fm(conv.fwd(to_fm(eng, xb)))
        torch.cuda.synchronize()
        cy, cx = (H // 2) // s, (W // 2) // s
        hit = y[0, :, cy, cx]                                # the output pixel straight under it
        nf = ~torch.isfinite(hit)
        if act == "relu" and bad != float("nan"):
            # relu(-inf) = 0 and relu(+inf * w) is inf only where w > 0: at least the positive-weight channels must show it
            assert nf.any(), (bad, act)
        else:
            assert nf.all(), (bad, act, int(nf.sum()), cout)


@pytest.mark.parametrize("case", [
    # cin (segments), cout, k, pad, dil, H, W
    ((505,), 64, 3, 1, 1, 20, 24),          # blur_skip conv_scale.1
    ((256,), 64, 3, 2, 2, 14, 18),          # dilated
    ((128, 128), 3, 3, 1, 1, 20, 24),       # kb.sr_reconst: two input segments -> two mirrored launches at a column offset
    ((264, 136), 17, 3, 1, 1, 9, 30),       # ragged everything
    ((256,), 32, 1, 0, 1, 12, 16),          # 1x1
])
def test_mirrored_wgrad_of_few_output_channels(case):
    """engine.Conv._bwd_weights_impl: layers with <= 64 output channels run the mirrored problem (rows = input channels); against torch
    autograd, and against the plain form of the same launch"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, grad_acc
    segs, cout, k, p, d, H, W = case
    cin = sum(segs)
    torch.manual_seed(11)
    eng = _eng()
    x = torch.randn(2, cin, H, W).half().float()
    w = (torch.randn(cout, cin, k, k) / (cin * k * k) ** 0.5)
    dpre = torch.randn(2, cout, H, W).half().float()
    wr = w.clone().requires_grad_(True)
    F.conv2d(x, wr, None, 1, p, d).backward(dpre)
    fx = tuple(to_fm(eng, t) for t in torch.split(x, list(segs), 1))
    got = {}
    for mirror in (True, False):
        params = {"l.weight": w.clone().cuda()}
        conv = Conv(eng, "l", params, k, 1, p, d, bias=False, split=segs if len(segs) > 1 else None)
        eng.wgrad_mirror = mirror
        conv.bwd_weights(to_fm(eng, dpre), fx if len(fx) > 1 else fx[0])
        conv.bwd_weights(to_fm(eng, dpre), fx if len(fx) > 1 else fx[0])          # accumulates
        torch.cuda.synchronize()
        got[mirror] = params["l.weight"].gacc.cpu() / 2
        assert relmax(got[mirror], wr.grad) < 2e-3, mirror
    assert relmax(got[True], got[False]) < 1e-5


@pytest.mark.parametrize("cout,h,w", [(128, 12, 20), (128, 9, 33), (64, 16, 8)])
def test_fused_backward_of_the_thin_transposed_prelu_layer(cout, h, w):
    """csrc/conv_kbup.hip (kb.up_conv1: ConvTranspose2d 3 -> C 8x8 s4 + PReLU, output added to a residual): dPre, weight gradient and
    slope gradient from one pass over dOut with the pre-activation rebuilt from the input -- against torch autograd and against the
    epilogue-backward + wgrad launches it replaces"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, grad_acc
    torch.manual_seed(3)
    eng = _eng()
    N = 2
    x = (torch.randn(N, 3, h, w) * 0.5).half().float()
    wt = (torch.randn(3, cout, 8, 8) / 6.0).half().float()
    a = torch.tensor([0.25])
    res = torch.randn(N, cout, 4 * h, 4 * w).half().float()
    dout = torch.randn(N, cout, 4 * h, 4 * w).half().float()
    xr, wr, ar = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), a.clone().requires_grad_(True)
    pre = F.conv_transpose2d(xr, wr, None, 4, 2)
    (F.prelu(pre, ar) + res).backward(dout)
    got = {}
    for fused in (True, False):
        params = {"l.weight": wt.clone().cuda(), "l.a": a.clone().cuda()}
        conv = Conv(eng, "l", params, 8, 4, 2, 1, transposed=True, bias=False, act=L.ACT_PRELU, prelu="l.a")
        conv.frozen = False
        fx, fres, fd = to_fm(eng, x), to_fm(eng, res), to_fm(eng, dout)
        out = conv.fwd(fx, res=fres, res_mode=L.RES_ADD)
        dpk = eng.new(N, 4 * h, 4 * w, cout)
        if fused:
            assert conv.thin_tp_fused_ok(fx)
            conv.bwd_thin_tp_fused(fd, fx, dpk)
        else:
            eng.epilogue_bwd(fd, out=out, act=conv.act, slope=conv.slope, prelu=conv.prelu, res=fres, res_mode=L.RES_ADD, dpre=dpk,
                             dprelu=grad_acc(conv.prelu), creal=cout)
            conv.bwd_weights(dpk, fx)
        torch.cuda.synchronize()
        got[fused] = (from_fm(dpk), params["l.weight"].gacc.cpu(), params["l.a"].gacc.cpu())
    gate = torch.where(pre.detach() > 0, torch.ones_like(pre), torch.full_like(pre, 0.25))
    assert relmax(got[True][0], dout * gate) < 2e-3
    assert relmax(got[True][1], wr.grad) < 2e-3
    assert abs(float(got[True][2]) - float(ar.grad)) < 2e-3 * float((dout * pre.detach()).abs().sum()) ** 0.5 + 2e-3 * abs(float(ar.grad))
    # the launches it replaces recover the pre-activation's sign from (stored output - residual): where the residual is much larger than
    # the pre-activation (as here, and as in the network: a small error image's response added to the up-block's features) the fp16
    # rounding of the sum hides it, so that form is the LESS accurate of the two (measured here: weight gradient 7e-2 off autograd's)
    e_old, e_new = relmax(got[False][1], wr.grad), relmax(got[True][1], wr.grad)
    print(f"   weight gradient vs autograd: fused {e_new:.1e}, epilogue-backward + wgrad {e_old:.1e}")
    assert e_new <= e_old + 1e-4


@pytest.mark.parametrize("cout,H,W", [(128, 24, 40), (128, 9, 70), (64, 16, 32)])
def test_thin_input_dgrad_with_the_layer_belows_epilogue_backward(cout, H, W):
    """csrc/conv_thin.hip, DACT: the accumulating 3x3 dgrad from a 3-channel image gradient that completes dOut of a layer
    out = prelu(pre) + res also writes that layer's dPre, the residual's gradient and the slope-gradient sum -- against fp64"""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, grad_acc
    torch.manual_seed(5)
    eng = _eng()
    eng.thin_dact = True
    N = 2
    w = (torch.randn(3, cout, 3, 3) / 5.0).half().float()           # the head conv: cout features -> 3 image channels (OIHW [3, cout])
    a = torch.tensor([0.2])
    dimg = torch.randn(N, 3, H, W).half().float()                     # gradient wrt the 3-channel image
    old = torch.randn(N, cout, H, W).half().float()                   # what dOut held before this contribution
    h0 = torch.randn(N, cout, H, W).half().float()
    pre = torch.randn(N, cout, H, W)
    hh = (F.prelu(pre, a) + h0).half().float()                        # the layer below's saved output
    head = Conv(eng, "l", {"l.weight": w.cuda()}, 3, 1, 1, 1, bias=False)
    below = Conv(eng, "b", {"b.weight": torch.zeros(8, cout, 8, 8).cuda(), "b.a": a.clone().cuda()}, 8, 4, 2, 1, transposed=True, bias=False,
                 act=L.ACT_PRELU, prelu="b.a")
    below.frozen = False
    f_old, f_h, f_h0, f_d = to_fm(eng, old), to_fm(eng, hh), to_fm(eng, h0), to_fm(eng, dimg)
    spare = eng.new(N, H, W, cout)
    head.bwd_input(f_d, out=f_old, accumulate=True, dact=(below, f_h), dres=(f_h0, spare, L.RES_ADD))
    torch.cuda.synchronize()
    assert head.last_fused
    tot = old.double() + F.conv_transpose2d(dimg.double(), w.double(), None, 1, 1)      # dgrad of conv2d(x, w[3, cout]) wrt x
    y = hh.double() - h0.double()
    pos = y > 0
    ref_dpre = torch.where(pos, tot, tot * 0.2)
    ref_da = float((tot * y / 0.2)[~pos].sum())
    assert relmax(from_fm(f_old), ref_dpre.float()) < 2e-3
    assert relmax(from_fm(spare), tot.float()) < 2e-3
    got_da = float(below.prelu.gacc.cpu())
    assert abs(got_da - ref_da) < 1e-3 * float((tot * y / 0.2)[~pos].abs().sum()) ** 0.5 + 1e-3 * abs(ref_da), (got_da, ref_da)


@pytest.mark.parametrize("cin,cout,H,W", [(32, 32, 19, 45), (32, 32, 16, 64), (49, 32, 24, 33), (32, 49, 9, 40), (49, 49, 17, 70), (64, 64, 8, 32)])
def test_full_resolution_thin_wgrad(cin, cout, H, W):
    """csrc/conv_wgrad_hr.hip (dPre tile + input halo tile in LDS once per 8 x 32 pixels, nine taps from the one halo, one slab per
    workgroup) against torch autograd on fp16-rounded operands and against the tiled GEMM kernel: the 32 / 49 / 64-channel 3x3 layers of
    the kernel predictor and the decoder head, ragged tiles included."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(cin * 100 + cout + H)
    eng = _eng()
    lib = L.load()
    N = 3
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5).half().float()
    dpre = torch.randn(N, cout, H, W).half().float()
    wr = w.clone().requires_grad_(True)
    F.conv2d(x, wr, None, 1, 1).backward(dpre)
    grads = []
    for mode in (2, 0):
        lib.csbsr_debug_set_wgrad_hr(mode)
        try:
            params = {"l.weight": w.clone().cuda()}
            conv = Conv(eng, "l", params, 3, 1, 1, 1, bias=False, act=L.ACT_NONE)
            conv.bwd_weights(to_fm(eng, dpre), to_fm(eng, x))
            torch.cuda.synchronize()
            assert (lib.csbsr_debug_last_wgrad_kernel() == 8) == (mode == 2)
        finally:
            lib.csbsr_debug_set_wgrad_hr(1)
        grads.append(params["l.weight"].gacc.cpu())
        assert relmax(grads[-1], wr.grad) < 2e-3
    assert relmax(grads[0], grads[1]) < 1e-3


@pytest.mark.parametrize("H,W", [(9, 12), (1, 7), (16, 33)])
def test_constant_gradient_dgrad_fold(H, W):
    """KBPN._fold_const_dgrad (dgrad of fe_cat.2 behind the global average pool: one value per border class, masked fill) against the
    convolution kernels run on the broadcast gradient, and against torch autograd."""
    import types
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, FM, pad8
    from csbsr_amd.modeling.kbpn import KBPN
    torch.manual_seed(H * 100 + W)
    eng = _eng()
    N, cin, cout, slope = 2, 32, 49, 0.1
    w = (torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5).half().float()
    conv = Conv(eng, "l", {"l.weight": w.cuda()}, 3, 1, 1, 1, bias=False, act=L.ACT_LRELU, slope=slope)
    g = (torch.randn(N, cout) * 0.01).half().float()
    below = torch.randn(N, cin, H, W).half().float()
    xr = torch.zeros(N, cin, H, W, requires_grad=True)
    F.conv2d(xr, w, None, 1, 1).backward(g[:, :, None, None].expand(N, cout, H, W))
    ref = xr.grad * torch.where(below > 0, torch.ones(()), torch.full((), slope))
    m = torch.ones(4, 3)
    m[2, 0] = m[3, 0] = 0.0
    m[1, 2] = m[3, 2] = 0.0
    stub = types.SimpleNamespace(eng=eng, Mtap=m.cuda())
    mfm = to_fm(eng, below)
    out = KBPN._fold_const_dgrad(stub, conv, g.cuda(), (mfm, slope), H, W)
    t = torch.zeros(N, 1, 1, pad8(cout), dtype=torch.float16, device="cuda")
    t[:, 0, 0, :cout] = g.cuda().half()
    out2 = conv.bwd_input(FM(t, cout, bcast=True, H=H, W=W), mask=(mfm, slope))
    torch.cuda.synchronize()
    assert relmax(from_fm(out), ref) < 2e-3
    assert relmax(from_fm(out), from_fm(out2)) < 2e-3


@pytest.mark.parametrize("cout,H,W,acc,act", [(128, 19, 45, True, "none"), (49, 16, 64, False, "relu"), (200, 9, 40, True, "none"),
                                              (384, 8, 32, False, "lrelu"), (32, 11, 33, True, "none")])
def test_streaming_thin_input_kernel(cout, H, W, acc, act):
    """conv_thin_cin2_kernel (3-channel image -> cout channels, 3x3, plain or accumulating epilogue; the dgrads of kb.sr_reconst /
    output_conv into the feature gradient and fe_SR.0 forward) against F.conv2d on fp16-rounded operands and against the
    general-epilogue kernel it takes these launches from."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(cout + H * W)
    eng = _eng()
    lib = L.load()
    N = 2
    # as a dgrad: the layer is Conv2d(cout -> 3); its input gradient = conv of dPre (3 channels) with the flipped, transposed weights
    w = (torch.randn(3, cout, 3, 3) / (cout * 9) ** 0.5).half().float()
    conv = Conv(eng, "l", {"l.weight": w.cuda()}, 3, 1, 1, 1, bias=False, act=L.ACT_NONE)
    dpre = torch.randn(N, 3, H, W).half().float()
    old = torch.randn(N, cout, H, W).half().float()
    xr = torch.zeros(N, cout, H, W, requires_grad=True)
    F.conv2d(xr, w, None, 1, 1).backward(dpre)
    refd = xr.grad + (old if acc else 0.0)
    # as a forward: Conv2d(3 -> cout), no bias, activation
    wf = (torch.randn(cout, 3, 3, 3) / 27 ** 0.5).half().float()
    a = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU}[act]
    fconv = Conv(eng, "f", {"f.weight": wf.cuda()}, 3, 1, 1, 1, bias=False, act=a, slope=0.1)
    x = torch.randn(N, 3, H, W).half().float()
    pre = F.conv2d(x, wf, None, 1, 1)
    reff = {"none": pre, "relu": F.relu(pre), "lrelu": F.leaky_relu(pre, 0.1)}[act]
    outs = []
    for mode in (2, 2 | 512):            # csbsr_debug_set_conv_glds: default, streaming variant off
        lib.csbsr_debug_set_conv_glds(mode)
        try:
            dx = to_fm(eng, old)
            conv.bwd_input(to_fm(eng, dpre), out=dx, accumulate=acc)
            torch.cuda.synchronize()
            assert (lib.csbsr_debug_last_conv_kernel() & 255) == (13 if mode == 2 else 6)
            y = fconv.fwd(to_fm(eng, x))
            torch.cuda.synchronize()
            assert (lib.csbsr_debug_last_conv_kernel() & 255) == (13 if mode == 2 else 6)
        finally:
            lib.csbsr_debug_set_conv_glds(2)
        outs.append((from_fm(dx), from_fm(y)))
        assert relmax(outs[-1][0], refd) < 2e-3
        assert relmax(outs[-1][1], reff) < 2e-3
    assert relmax(outs[0][0], outs[1][0]) < 1e-3 and relmax(outs[0][1], outs[1][1]) < 1e-3


def test_two_segment_broadcast_and_epilogue():
    """cat(features, spatially-constant code) conv with FMA epilogue, fp32 planar side output and GAP stat."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, FM, pad8
    eng = _eng()
    torch.manual_seed(3)
    N, H, W, c0, c1, cout = 2, 10, 12, 24, 441, 40
    x0 = torch.randn(N, c0, H, W).half().float()
    kv = (torch.rand(N, c1) / c1).half().float()
    w = (torch.randn(cout, c0 + c1, 3, 3) / 30).half().float()
    b = torch.randn(cout) * 0.1
    r1 = torch.randn(N, cout, H, W).half().float()
    r2 = torch.randn(N, cout, H, W).half().float()
    params = {"l.weight": w.cuda(), "l.bias": b.cuda()}
    conv = Conv(eng, "l", params, 3, 1, 1, act=L.ACT_NONE, split=(c0, c1))
    kt = torch.zeros(N, 1, 1, pad8(c1), dtype=torch.float16)
    kt[:, 0, 0, :c1] = kv.half()
    kfm = FM(kt.cuda(), c1, bcast=True, H=H, W=W)
    stat = torch.zeros(N, pad8(cout), device="cuda")
    y = conv.fwd((to_fm(eng, x0), kfm), res=to_fm(eng, r1), res2=to_fm(eng, r2), res_mode=L.RES_FMA, stat=stat,
                 stat_mode=L.STAT_SAMPLE_SUM)
    cat = torch.cat((x0, kv[:, :, None, None].expand(N, c1, H, W)), 1)
    pre = F.conv2d(cat, w, b, 1, 1)
    ref = pre + r1 * r2
    torch.cuda.synchronize()
    assert relmax(from_fm(y), ref) < 2e-3
    assert relmax(stat[:, :cout].cpu(), pre.sum((2, 3))) < 2e-3
    # dgrad wrt the broadcast segment = per-sample sum over pixels
    dpre = torch.randn_like(pre).half().float()
    catr = cat.clone().requires_grad_(True)
    F.conv2d(catr, w, None, 1, 1).backward(dpre)
    dk = torch.zeros(N, pad8(c1), device="cuda")
    conv.bwd_input(to_fm(eng, dpre), seg=1, stat=dk)
    d0 = conv.bwd_input(to_fm(eng, dpre), seg=0)
    conv.bwd_weights(to_fm(eng, dpre), (to_fm(eng, x0), kfm))
    wr = w.clone().requires_grad_(True)
    F.conv2d(cat, wr, None, 1, 1).backward(dpre)
    torch.cuda.synchronize()
    assert relmax(dk[:, :c1].cpu(), catr.grad[:, c0:].sum((2, 3))) < 2e-3
    assert relmax(from_fm(d0), catr.grad[:, :c0]) < 2e-3
    assert relmax(params["l.weight"].gacc.cpu(), wr.grad) < 3e-3


@pytest.mark.parametrize("cin,cout,H,W,acc", [(32, 49, 40, 36, False), (128, 128, 24, 24, True), (256, 128, 192, 192, False), (49, 32, 33, 70, True)])
def test_dgrad_with_fused_activation_mask(cin, cout, H, W, acc):
    """dgrad whose epilogue applies the activation derivative of the layer below (mask = that layer's saved output): equals the
    plain dgrad (+ old contents when accumulating) times (out > 0 ? 1 : slope) -- the stand-alone epilogue-backward pass, fused."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(cin * 7 + cout)
    eng = _eng()
    N, slope = 2, 0.01
    w = (torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5).half().float()
    params = {"l.weight": w.cuda()}
    conv = Conv(eng, "l", params, 3, 1, 1, 1, bias=False, act=L.ACT_NONE)
    dpre = torch.randn(N, cout, H, W).half().float()
    below = torch.randn(N, cin, H, W).half().float()          # saved output of the layer below (sign decides the mask)
    old = torch.randn(N, cin, H, W).half().float()
    xr = torch.zeros(N, cin, H, W, requires_grad=True)
    F.conv2d(xr, w, None, 1, 1).backward(dpre)
    ref = (xr.grad + (old if acc else 0.0)) * torch.where(below > 0, torch.ones(()), torch.full((), slope))
    out = to_fm(eng, old)
    conv.bwd_input(to_fm(eng, dpre), out=out, accumulate=acc, mask=(to_fm(eng, below), slope))
    torch.cuda.synchronize()
    assert relmax(from_fm(out), ref) < 2e-3


@pytest.mark.parametrize("cin,cout,act,ks", [(32, 32, "lrelu", 3), (32, 49, "none", 3), (49, 49, "lrelu", 3), (49, 32, "relu", 3), (3, 49, "relu", 3),
                                             (49, 32, "lrelu", 1), (32, 49, "none", 1), (32, 32, "relu", 1)])
def test_hr_direct_conv_kernel(cin, cout, act, ks):
    """The direct 3x3 / 1x1 kernel of the full-resolution 32 / 49-channel layers (csrc/conv_hr.hip: halo tile in LDS, weights in registers),
    forward (+ per-sample channel sums without a stored output for the 32 -> 49 case, as fe_cat.2 runs) and dgrad with the fused
    activation mask, against torch on the same fp16-rounded operands; ragged tiles on both axes; (3, 49) is NOT eligible and must
    still come out right through the other kernels."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(cin * 100 + cout)
    eng = _eng()
    N, H, W = 2, 363, 371
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cout, cin, ks, ks) / (cin * ks * ks) ** 0.5).half().float()
    params = {"l.weight": w.cuda()}
    a = {"lrelu": L.ACT_LRELU, "relu": L.ACT_RELU, "none": L.ACT_NONE}[act]
    conv = Conv(eng, "l", params, ks, 1, ks // 2, 1, bias=False, act=a, slope=0.01)
    ref_pre = F.conv2d(x, w, None, 1, ks // 2)
    ref = {"lrelu": F.leaky_relu(ref_pre, 0.01), "relu": F.relu(ref_pre), "none": ref_pre}[act]
    xf = to_fm(eng, x)
    y = conv.fwd(xf)
    torch.cuda.synchronize()
    used_hr = (L.load().csbsr_debug_last_conv_kernel() & 255) == 8
    assert used_hr == (cin in (32, 49))
    assert relmax(from_fm(y), ref) < 2e-3
    if act == "none":       # global-average-pool sums, output not stored (fe_cat.2)
        from csbsr_amd.engine import pad8
        stat = torch.zeros(N, pad8(cout), device="cuda")
        conv.fwd(xf, stat=stat, stat_mode=L.STAT_SAMPLE_SUM, store=False)
        torch.cuda.synchronize()
        assert (L.load().csbsr_debug_last_conv_kernel() & 255) == 8
        assert relmax(stat[:, :cout].cpu(), ref.sum((2, 3))) < 2e-3
    # dgrad with the activation mask of the layer below
    dpre = torch.randn(N, cout, H, W).half().float()
    below = torch.randn(N, cin, H, W).half().float()
    xr = torch.zeros(N, cin, H, W, requires_grad=True)
    F.conv2d(xr, w, None, 1, ks // 2).backward(dpre)
    refd = xr.grad * torch.where(below > 0, torch.ones(()), torch.full((), 0.01))
    dx = conv.bwd_input(to_fm(eng, dpre), mask=(to_fm(eng, below), 0.01))
    torch.cuda.synchronize()
    assert (L.load().csbsr_debug_last_conv_kernel() & 255) == 8          # the dgrad's own input is the 32 / 49-channel dPre: always eligible here
    assert relmax(from_fm(dx), refd) < 2e-3


@pytest.mark.parametrize("k,s,N,h,w", [(8, 4, 4, 130, 141), (12, 8, 8, 96, 101)])
def test_thin_strided_dgrad_kernel(k, s, N, h, w):
    """The dgrad of kb.up_conv1 (ConvTranspose2d 3 -> 128, k = 2 x stride; kbpn.py:372-374) -- a strided conv from 128 channels into 3 --
    on its own streaming kernel (csrc/conv_thin.hip, conv_thin_sc_kernel): fp32 planar output as the backward requests it, and the fp16
    output; ragged tiles on both axes; against autograd on the same fp16-rounded operands."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(k)
    eng = _eng()
    wt = (torch.randn(3, 128, k, k) / (3 * k * k / s / s) ** 0.5).half().float()
    conv = Conv(eng, "l", {"l.weight": wt.cuda()}, k, s, 2, 1, transposed=True, bias=False)
    dpre = torch.randn(N, 128, h * s, w * s).half().float()
    xr = torch.zeros(N, 3, h, w, requires_grad=True)
    F.conv_transpose2d(xr, wt, None, s, 2).backward(dpre)
    dfm = to_fm(eng, dpre)
    d32 = torch.empty(N, 3, h, w, device="cuda")
    conv.bwd_input(dfm, out32=d32, in_hw=(h, w))
    torch.cuda.synchronize()
    assert (L.load().csbsr_debug_last_conv_kernel() & 255) == 15
    assert relmax(d32.cpu(), xr.grad) < 2e-3
    d16 = conv.bwd_input(dfm, in_hw=(h, w))
    torch.cuda.synchronize()
    assert (L.load().csbsr_debug_last_conv_kernel() & 255) == 15
    assert relmax(from_fm(d16), xr.grad) < 2e-3


def test_hr_direct_conv_kernel_128_couts():
    """32 -> 128 channels: the launch that gathers a stage's slice of the concatenated feature gradient from the 3-channel dPre slots
    (KBPN._gather_conv) -- forward form, and the dgrad form the backward actually uses (a conv with 32 'output' channels whose dgrad has
    128), plain epilogue, ragged tiles.  Since round 6 the wide form of conv_x3n takes it (one 32-channel chunk of K, LDS-transposed
    whole-line stores: 4.8 -> 2.6 ms at the model's size); with that form off (debug mode 3) the direct kernel (two groups of workgroups,
    two 32-cout tiles each) still does.  Both against autograd, and against each other."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(5)
    eng = _eng()
    lib = L.load()
    N, H, W = 2, 363, 371
    x = torch.randn(N, 32, H, W).half().float()
    x[:, 3:8] = 0
    w = (torch.randn(128, 32, 3, 3) / 17.0).half().float()
    wt = (torch.randn(32, 128, 3, 3) / 17.0).half().float()          # a conv 128 -> 32: its dgrad maps 32 channels to 128
    xr = torch.zeros(N, 128, H, W, requires_grad=True)
    F.conv2d(xr, wt, None, 1, 1).backward(x)
    ref = F.conv2d(x, w, None, 1, 1)
    outs = []
    for xn_mode, kid in ((1, 20), (3, 8)):
        lib.csbsr_debug_set_conv_x3n(xn_mode)
        try:
            conv = Conv(eng, "l", {"l.weight": w.cuda()}, 3, 1, 1, 1, bias=False)
            y = conv.fwd(to_fm(eng, x))
            torch.cuda.synchronize()
            assert (lib.csbsr_debug_last_conv_kernel() & 255) == kid
            conv2 = Conv(eng, "m", {"m.weight": wt.cuda()}, 3, 1, 1, 1, bias=False)
            out = eng.new(N, H, W, 128)
            conv2.bwd_input(to_fm(eng, x), out=out, accumulate=False)
            torch.cuda.synchronize()
            assert (lib.csbsr_debug_last_conv_kernel() & 255) == kid
        finally:
            lib.csbsr_debug_set_conv_x3n(1)
        outs.append((from_fm(y), from_fm(out)))
        assert relmax(outs[-1][0], ref) < 2e-3
        assert relmax(outs[-1][1], xr.grad) < 2e-3
    assert relmax(outs[0][0], outs[1][0]) < 1e-3 and relmax(outs[0][1], outs[1][1]) < 1e-3


@pytest.mark.parametrize("k,s,p,cin,cout,H,W,mode", [
    (8, 4, 2, 128, 128, 24, 40, "prelu_add"),      # up_conv3: PReLU + residual add, ragged tiles on both axes
    (8, 4, 2, 128, 128, 16, 64, "prelu"),          # up_conv1
    (8, 4, 2, 128, 128, 17, 33, "prelu_sub"),      # down_conv2: PReLU - residual
    (12, 8, 2, 128, 128, 9, 34, "prelu_add"),      # x8 variant: 64 phases, phases with a single valid tap per axis
    (8, 4, 2, 64, 128, 16, 32, "relu"),            # 64 input channels: not eligible, general kernel
    (8, 4, 2, 100, 128, 16, 32, "relu"),           # padded input channels
    (8, 4, 2, 128, 100, 10, 20, "none"),           # padded output channels
])
def test_phase_decomposed_transposed_conv(k, s, p, cin, cout, H, W, mode):
    """csrc/conv_tp.hip (halo tile resident in LDS for all phases and taps, streamed fragment-ordered weights, register epilogue)
    against conv_transpose2d on the same fp16-rounded operands, and the same launches through the general LDS-DMA kernel."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(k * 1000 + cin + cout + H)
    eng = _eng()
    N = 2
    lib = L.load()
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cin, cout, k, k) / (cin * 4) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    a = torch.tensor([0.25])
    params = {"l.weight": w.cuda(), "l.bias": b.cuda(), "a": a.cuda()}
    act = {"prelu": L.ACT_PRELU, "relu": L.ACT_RELU, "none": L.ACT_NONE}[mode.split("_")[0]]
    conv = Conv(eng, "l", params, k, s, p, 1, transposed=True, bias=True, act=act, prelu="a" if act == L.ACT_PRELU else False)
    pre = F.conv_transpose2d(x, w, b, s, p)
    ref = {L.ACT_PRELU: F.prelu(pre, a), L.ACT_RELU: F.relu(pre), L.ACT_NONE: pre}[act]
    res = torch.randn_like(ref).half().float()
    rm = L.RES_ADD if mode.endswith("_add") else (L.RES_SUB if mode.endswith("_sub") else L.RES_NONE)
    if rm == L.RES_ADD: ref = ref + res
    if rm == L.RES_SUB: ref = ref - res
    outs = []
    for tp_mode in (2, 0):
        lib.csbsr_debug_set_conv_tp(tp_mode)
        try:
            y = conv.fwd(to_fm(eng, x), res=to_fm(eng, res) if rm != L.RES_NONE else None, res_mode=rm)
            torch.cuda.synchronize()
            from csbsr_amd.engine import pad8
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 9) == (tp_mode == 2 and pad8(cin) == 128 and pad8(cout) > 64)
        finally:
            lib.csbsr_debug_set_conv_tp(1)
        outs.append(from_fm(y))
        assert relmax(outs[-1], ref) < 2e-3
    assert relmax(outs[0], outs[1]) < 1e-3


@pytest.mark.parametrize("cin,cout,H,W,acc,masked", [(128, 128, 16, 32, True, True), (128, 128, 9, 40, False, True), (128, 128, 24, 33, True, False),
                                                     (128, 96, 8, 32, False, False), (128, 64, 12, 36, True, True), (100, 128, 8, 32, False, True)])
def test_phase_decomposed_strided_dgrad(cin, cout, H, W, acc, masked):
    """dgrad of the 8x8 stride-4 convolutions (a transposed conv over dOut) through csrc/conv_tp.hip, accumulating into the gradient
    buffer and applying the fused activation-derivative mask of the layer below, as up_conv2 / down_conv1 / down_conv3 run it."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(cin + cout + H * W)
    eng = _eng()
    lib = L.load()
    N, slope, k, s, p = 2, 0.2, 8, 4, 2
    w = (torch.randn(cout, cin, k, k) / (cin * 4) ** 0.5).half().float()
    conv = Conv(eng, "l", {"l.weight": w.cuda()}, k, s, p, 1, bias=False, act=L.ACT_NONE)
    dpre = torch.randn(N, cout, H, W).half().float()
    IH, IW = s * H, s * W
    below = torch.randn(N, cin, IH, IW).half().float()
    old = torch.randn(N, cin, IH, IW).half().float()
    xr = torch.zeros(N, cin, IH, IW, requires_grad=True)
    F.conv2d(xr, w, None, s, p).backward(dpre)
    ref = xr.grad + (old if acc else 0.0)
    if masked:
        ref = ref * torch.where(below > 0, torch.ones(()), torch.full((), slope))
    outs = []
    for tp_mode in (2, 0):
        lib.csbsr_debug_set_conv_tp(tp_mode)
        try:
            out = to_fm(eng, old)
            conv.invalidate()
            conv.bwd_input(to_fm(eng, dpre), out=out, accumulate=acc, in_hw=(IH, IW), mask=(to_fm(eng, below), slope) if masked else None)
            torch.cuda.synchronize()
            from csbsr_amd.engine import pad8
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 9) == (tp_mode == 2 and pad8(cout) == 128 and pad8(cin) > 64)
        finally:
            lib.csbsr_debug_set_conv_tp(1)
        outs.append(from_fm(out))
        assert relmax(outs[-1], ref) < 2e-3
    assert relmax(outs[0], outs[1]) < 1e-3


@pytest.mark.parametrize("H,W,frozen", [(16, 32, False), (8, 64, False), (16, 32, True), (12, 32, False)])
def test_phase_decomposed_dgrad_takes_over_the_epilogue_backward(H, W, frozen):
    """The dgrad of an 8x8 stride-4 conv that completes a gradient (accumulate) and is handed the layer below (``dact``): csrc/conv_tp.hip
    applies that layer's PReLU derivative from its saved output and adds its bias / PReLU-slope gradient sums -- everything
    csbsr_epilogue_backward would do in a pass of its own -- against torch autograd of  conv2d(prelu(z + b, a)) ; (12, 32) is not
    whole tiles: the launch must decline (``last_fused`` False) and leave the gradient unmasked for the stand-alone pass."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, grad_acc
    torch.manual_seed(H * W + int(frozen))
    eng = _eng()
    lib = L.load()
    N, C, k, s, p = 2, 128, 8, 4, 2
    IH, IW = s * H, s * W
    w = (torch.randn(C, C, k, k) / (C * 4) ** 0.5).half().float()
    conv = Conv(eng, "l", {"l.weight": w.cuda()}, k, s, p, 1, bias=False, act=L.ACT_NONE)
    a0, b0 = torch.tensor([0.25]), (torch.randn(C) * 0.1)
    pb = {"b.weight": torch.zeros(C, C, k, k).cuda(), "b.bias": b0.clone().cuda(), "a": a0.clone().cuda()}
    below = Conv(eng, "b", pb, k, s, p, 1, transposed=True, bias=True, act=L.ACT_PRELU, prelu="a")
    below.frozen = frozen
    z = torch.randn(N, C, IH, IW, requires_grad=True)
    b = b0.clone().requires_grad_(True)
    a = a0.clone().requires_grad_(True)
    y = F.prelu(z + b[None, :, None, None], a)
    y16 = y.detach().half().float()                      # the saved output as the kernels see it
    dpre = torch.randn(N, C, H, W).half().float()
    old = torch.randn(N, C, IH, IW).half().float()
    # reference on the fp16-rounded saved output (the mask / slope sums read that)
    yr = y16.clone().requires_grad_(True)
    (F.conv2d(yr, w, None, s, p) * dpre).sum().backward()
    dy = yr.grad + old
    neg = ~(y16 > 0)
    ref_dz = torch.where(neg, dy * a0, dy)
    ref_db = ref_dz.sum((0, 2, 3))
    ref_da = (dy * (y16 / a0))[neg].sum()
    lib.csbsr_debug_set_conv_tp(2)
    try:
        out = to_fm(eng, old)
        conv.bwd_input(to_fm(eng, dpre), out=out, accumulate=True, in_hw=(IH, IW), dact=(below, to_fm(eng, y16)))
        torch.cuda.synchronize()
    finally:
        lib.csbsr_debug_set_conv_tp(1)
    whole = H % 8 == 0 and W % 32 == 0
    assert conv.last_fused == whole
    if not whole:
        assert relmax(from_fm(out), dy) < 2e-3              # plain dgrad + old: the caller runs the epilogue-backward pass itself
        return
    assert (lib.csbsr_debug_last_conv_kernel() & 255) == 9
    assert relmax(from_fm(out), ref_dz) < 2e-3
    if frozen:
        assert getattr(pb["b.bias"], "gacc", None) is None and getattr(pb["a"], "gacc", None) is None
    else:
        assert relmax(grad_acc(pb["b.bias"]).cpu(), ref_db) < 2e-3
        assert abs(float(grad_acc(pb["a"]).cpu()) - float(ref_da)) < 2e-3 * float((dy * (y16 / a0))[neg].abs().sum()) ** 0.5 + 2e-3 * abs(float(ref_da))


@pytest.mark.parametrize("cin,cout,H,W,mode", [
    (128, 128, 19, 45, "lrelu"),            # ragged tiles on both axes, two 64-channel chunks
    (384, 825, 16, 32, "lrelu"),            # SFT conv0 shape: 6 chunks, 7 cout tiles (the last one 57 wide)
    (825, 384, 9, 40, "none_fma"),          # SFT conv1 shape: 825 -> 832 padded input channels (13 chunks), out = conv + res * res2
    (192, 100, 24, 33, "relu_add"),         # three chunks (odd: the chunk buffers alternate across chunks), padded couts, residual add (12 tiles: one per
                                            # workgroup here -- the multi-tile walk runs under CU budgets in tests/test_conv_exact_gpu.py)
    (256, 256, 8, 64, "none"),
])
def test_wide_3x3_kernel(cin, cout, H, W, mode):
    """csrc/conv_x3.hip (per-chunk halo tile in LDS, fragment-ordered weights from L2, general fused epilogue) against F.conv2d on the
    same fp16-rounded operands and against the implicit-GEMM kernels: forward with the fused epilogue modes the SFT layers use, and
    the dgrad (flipped, transposed weights) accumulating into an existing gradient."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(cin + cout + H)
    eng = _eng()
    lib = L.load()
    N = 2
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    act = {"lrelu": L.ACT_LRELU, "relu": L.ACT_RELU, "none": L.ACT_NONE}[mode.split("_")[0]]
    conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True, act=act, slope=0.1)
    pre = F.conv2d(x, w, b, 1, 1)
    ref = {L.ACT_LRELU: F.leaky_relu(pre, 0.1), L.ACT_RELU: F.relu(pre), L.ACT_NONE: pre}[act]
    res = torch.randn_like(ref).half().float()
    res2 = torch.randn_like(ref).half().float()
    kw = {}
    if mode.endswith("_add"):
        ref = ref + res; kw = dict(res=res, res_mode=L.RES_ADD)
    if mode.endswith("_fma"):
        ref = ref + res * res2; kw = dict(res=res, res2=res2, res_mode=L.RES_FMA)
    dpre = torch.randn(N, cout, H, W).half().float()
    old = torch.randn(N, cin, H, W).half().float()
    xr = torch.zeros(N, cin, H, W, requires_grad=True)
    F.conv2d(xr, w, None, 1, 1).backward(dpre)
    refd = xr.grad + old
    outs = []
    for x3_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3(x3_mode)
        try:
            conv.invalidate()
            y = conv.fwd(to_fm(eng, x), **{k_: (to_fm(eng, v) if isinstance(v, torch.Tensor) else v) for k_, v in kw.items()})
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) in (10, 17)) == (x3_mode == 2 and cin % 64 == 0 or x3_mode == 2 and cin == 825)
            dx = to_fm(eng, old)
            conv.bwd_input(to_fm(eng, dpre), out=dx, accumulate=True)
            torch.cuda.synchronize()
            from csbsr_amd.engine import pad8
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) in (10, 17)) == (x3_mode == 2 and pad8(cout) % 64 == 0 and pad8(cout) >= 128)
        finally:
            lib.csbsr_debug_set_conv_x3(1)
        outs.append((from_fm(y), from_fm(dx)))
        assert relmax(outs[-1][0], ref) < 2e-3
        assert relmax(outs[-1][1], refd) < 2e-3
    assert relmax(outs[0][0], outs[1][0]) < 1e-3 and relmax(outs[0][1], outs[1][1]) < 1e-3


@pytest.mark.parametrize("cin,cout,H,W,mode", [
    (128, 128, 19, 45, "lrelu"),            # ragged tiles on both axes, odd width (the last x-tile's second output is outside), four chunks
    (384, 825, 16, 32, "lrelu"),            # SFT conv0 shape: 12 chunks, 7 cout tiles (the last one 57 wide), half a tile wide
    (825, 384, 9, 40, "none_fma"),          # SFT conv1 shape (shift branch): 825 -> 832 padded input channels (26 chunks), out = conv + res * res2
    (825, 384, 8, 64, "sigmoid"),           # SFT conv1 shape (scale branch)
    (192, 100, 24, 133, "relu_add"),        # six chunks, three tile columns, padded couts, residual add
    (96, 256, 8, 64, "none"),               # three chunks (odd: the V buffers alternate across chunks; 8 tiles, one per workgroup)
    (256, 256, 12, 128, "none"),
])
def test_wide_3x3_winograd_kernel(cin, cout, H, W, mode):
    """csrc/conv_x3w.hip (Winograd F(2, 3) along x: input transform registers -> LDS, transformed fp16 weights, output transform on the
    accumulators, general fused epilogue) against F.conv2d on the same fp16-rounded operands and against the direct kernels: forward
    with the fused epilogue modes the SFT layers use, and the dgrad (flipped, transposed weights) accumulating into an existing gradient.
    The transformed operands are rounded to fp16 once more than the direct product's: the bound is the direct kernels' 2e-3."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, pad8
    torch.manual_seed(cin + cout + H)
    eng = _eng()
    eng.use_x3w = 2             # opt-in kernel; 2 = any eligible layer (1 = the layers marked Conv.winograd: KBPN's SFT convs)
    lib = L.load()
    N = 2
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    act = {"lrelu": L.ACT_LRELU, "relu": L.ACT_RELU, "none": L.ACT_NONE, "sigmoid": L.ACT_SIGMOID}[mode.split("_")[0]]
    conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True, act=act, slope=0.1)
    pre = F.conv2d(x, w, b, 1, 1)
    ref = {L.ACT_LRELU: F.leaky_relu(pre, 0.1), L.ACT_RELU: F.relu(pre), L.ACT_NONE: pre, L.ACT_SIGMOID: torch.sigmoid(pre)}[act]
    res = torch.randn_like(ref).half().float()
    res2 = torch.randn_like(ref).half().float()
    kw = {}
    if mode.endswith("_add"):
        ref = ref + res; kw = dict(res=res, res_mode=L.RES_ADD)
    if mode.endswith("_fma"):
        ref = ref + res * res2; kw = dict(res=res, res2=res2, res_mode=L.RES_FMA)
    dpre = torch.randn(N, cout, H, W).half().float()
    old = torch.randn(N, cin, H, W).half().float()
    xr = torch.zeros(N, cin, H, W, requires_grad=True)
    F.conv2d(xr, w, None, 1, 1).backward(dpre)
    refd = xr.grad + old
    outs = []
    for xw_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3w(xw_mode)
        try:
            conv.invalidate()
            y = conv.fwd(to_fm(eng, x), **{k_: (to_fm(eng, v) if isinstance(v, torch.Tensor) else v) for k_, v in kw.items()})
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 19) == (xw_mode == 2 and pad8(cin) % 32 == 0 and pad8(cout) >= 72)
            dx = to_fm(eng, old)
            conv.bwd_input(to_fm(eng, dpre), out=dx, accumulate=True)
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 19) == (xw_mode == 2 and pad8(cout) % 32 == 0 and pad8(cin) >= 72)
        finally:
            lib.csbsr_debug_set_conv_x3w(1)
        outs.append((from_fm(y), from_fm(dx)))
        print(f"   x3w mode {xw_mode}: forward {relmax(outs[-1][0], ref):.2e}  dgrad {relmax(outs[-1][1], refd):.2e}")
        assert relmax(outs[-1][0], ref) < 2e-3
        assert relmax(outs[-1][1], refd) < 2e-3
    assert relmax(outs[0][0], outs[1][0]) < 2e-3 and relmax(outs[0][1], outs[1][1]) < 2e-3


def test_wide_3x3_winograd_kernel_with_folded_constant_segment():
    """SFT conv0 as the model runs it (Conv.fwd_folded: features through the conv kernel, the spatially constant kernel-code segment as a
    per-border-class bias) on conv_x3w_kernel against the direct kernels and against F.conv2d on the concatenated input."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(11)
    eng = _eng()
    eng.use_x3w = 2             # opt-in kernel; 2 = any eligible layer (1 = the layers marked Conv.winograd: KBPN's SFT convs)
    lib = L.load()
    N, cf, cc, cout, H, W = 2, 384, 21, 100, 12, 40
    x = torch.randn(N, cf, H, W).half().float()
    kv = (torch.rand(N, cc) / cc).half().float()
    w = (torch.randn(cout, cf + cc, 3, 3) / ((cf + cc) * 9) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    ref = F.leaky_relu(F.conv2d(torch.cat([x, kv[:, :, None, None].expand(N, cc, H, W)], 1), w, b, 1, 1), 0.1)
    m = torch.ones(4, 3)
    m[2, 0] = m[3, 0] = 0.0
    m[1, 2] = m[3, 2] = 0.0
    outs = []
    for xw_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3w(xw_mode)
        try:
            conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True, act=L.ACT_LRELU, slope=0.1, split=(cf, cc))
            y, _ = conv.fwd_folded(to_fm(eng, x), kv.cuda(), m.cuda())
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 19) == (xw_mode == 2)
        finally:
            lib.csbsr_debug_set_conv_x3w(1)
        outs.append(from_fm(y))
        assert relmax(outs[-1], ref) < 2e-3
    assert relmax(outs[0], outs[1]) < 2e-3


def test_wide_3x3_kernel_with_folded_constant_segment():
    """SFT conv0 as the model runs it (Conv.fwd_folded: features through the conv kernel, the spatially constant kernel-code segment as a
    per-border-class bias) on conv_x3_kernel<3> against the implicit-GEMM kernel and against F.conv2d on the concatenated input."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(11)
    eng = _eng()
    lib = L.load()
    N, cf, cc, cout, H, W = 2, 384, 21, 100, 12, 40
    x = torch.randn(N, cf, H, W).half().float()
    kv = (torch.rand(N, cc) / cc).half().float()
    w = (torch.randn(cout, cf + cc, 3, 3) / ((cf + cc) * 9) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    ref = F.leaky_relu(F.conv2d(torch.cat([x, kv[:, :, None, None].expand(N, cc, H, W)], 1), w, b, 1, 1), 0.1)
    m = torch.ones(4, 3)
    m[2, 0] = m[3, 0] = 0.0
    m[1, 2] = m[3, 2] = 0.0
    outs = []
    for x3_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3(x3_mode)
        try:
            conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True, act=L.ACT_LRELU, slope=0.1, split=(cf, cc))
            y, _ = conv.fwd_folded(to_fm(eng, x), kv.cuda(), m.cuda())
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) in (10, 17)) == (x3_mode == 2)
        finally:
            lib.csbsr_debug_set_conv_x3(1)
        outs.append(from_fm(y))
        assert relmax(outs[-1], ref) < 2e-3
    assert relmax(outs[0], outs[1]) < 1e-3


@pytest.mark.parametrize("split", [0, 1])
def test_wide_form_of_narrow_kernel_with_folded_constant_segment(split):
    """Conv.fwd_folded on the WIDE form of conv_x3n (its LEAN instance: bias + the interior class row through LDS, the pixel's class row per
    piece on border tiles, rows transposed through LDS into whole-line stores): a map large enough to have interior tiles (rows 8..15,
    columns 32..63) next to border tiles and ragged edges; plain input (KBPN's SFT conv0 of stage 1) and split hi + lo input / output in the
    two-product plan (BlurSkip's conv0's); against the kernels that ran these launches before and against fp64 on the concatenated input."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv
    torch.manual_seed(13 + split)
    eng = _eng()
    lib = L.load()
    N, cf, cc, cout, H, W = 2, (64 if split else 128), 21, 200, 27, 100
    x = torch.randn(N, cf, H, W)
    if not split:
        x = x.half().float()
    kv = (torch.rand(N, cc) / cc).half().float()
    w = (torch.randn(cout, cf + cc, 3, 3) / ((cf + cc) * 9) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    m = torch.ones(4, 3)
    m[2, 0] = m[3, 0] = 0.0
    m[1, 2] = m[3, 2] = 0.0
    xs = to_fm_split(eng, x) if split else to_fm(eng, x)
    xv = from_fm_split(xs).double() if split else x.double()
    ref = F.leaky_relu(F.conv2d(torch.cat([xv, kv.double()[:, :, None, None].expand(N, cc, H, W)], 1), w.double(), b.double(), 1, 1), 0.1)
    outs = []
    for xn_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3n(xn_mode)
        try:
            conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True, act=L.ACT_LRELU, slope=0.1, split=(cf, cc))
            if split:
                conv.fwd_blocks, conv.dc_comp = 2, True
            y, _ = conv.fwd_folded(xs, kv.cuda(), m.cuda())
            torch.cuda.synchronize()
            kid = lib.csbsr_debug_last_conv_kernel()
            assert ((kid & 255) == 20) == (xn_mode == 2), kid
            if xn_mode == 2:
                assert (kid >> 8) & 8, "the LEAN instance"
        finally:
            lib.csbsr_debug_set_conv_x3n(1)
        outs.append((from_fm_split(y) if split else from_fm(y)).double())
        assert float((outs[-1] - ref).abs().max() / ref.abs().max()) < 2e-3
    e01 = float((outs[0] - outs[1]).abs().max() / ref.abs().max())
    print(f"   wide form, folded segment (split={split}): vs the previous kernel {e01:.2e}")
    assert e01 < (2e-5 if split else 1e-3)


@pytest.mark.parametrize("H,W", [(5, 5), (12, 40), (33, 70), (363, 371)])
def test_conv_with_two_ring_class_bias(H, W):
    """fe_cat.0 as the model runs it (Conv.fwd_classbias, conv desc cbias_mode 1): a 1x1 conv over cat(features, a map that is the
    output of TWO zero-padded 3x3 convs of a spatially constant code) with the second segment folded into a [B, 25, cout] table by
    csbsr_amd.modeling.kbpn.kernel_branch_table, against F.conv2d on the literally computed concatenated input."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, pad8
    from csbsr_amd.modeling.kbpn import kernel_branch_table, border_tap_mask, ring_tap_classes
    torch.manual_seed(H * W)
    eng = _eng()
    N, cf, ccode, c0, c1, cout = 2, 49, 21, 49, 49, 32
    x = torch.randn(N, cf, H, W).half().float()
    kv = torch.rand(N, ccode) / ccode
    w0, w1 = torch.randn(c0, ccode, 3, 3) / (ccode * 9) ** 0.5, torch.randn(c1, c0, 3, 3) / (c0 * 9) ** 0.5
    w = (torch.randn(cout, cf + c1, 1, 1) / (cf + c1) ** 0.5)
    act = lambda t: F.leaky_relu(t, 0.01)
    b2 = act(F.conv2d(act(F.conv2d(kv[:, :, None, None].expand(N, ccode, H, W), w0, None, 1, 1)), w1, None, 1, 1))
    w16 = w.clone()
    w16[:, :cf] = w[:, :cf].half().float()          # the feature half goes through the MFMA in fp16, the folded half stays fp32
    ref = F.leaky_relu(F.conv2d(torch.cat([x, b2], 1), w16), 0.01)
    tab = kernel_branch_table(kv, w0, w1, w[:, cf:, 0, 0], border_tap_mask(), ring_tap_classes(), act, act)       # [N, 5, 5, cout]
    cb = torch.zeros(N, 25, pad8(cout), device="cuda")
    cb[:, :, :cout] = tab.reshape(N, 25, cout).cuda()
    conv = Conv(eng, "l", {"l.weight": w.cuda()}, 1, 1, 0, 1, bias=False, act=L.ACT_LRELU, slope=0.01, split=(cf, c1))
    y = conv.fwd_classbias(to_fm(eng, x), cb, 1)
    torch.cuda.synchronize()
    # (full-resolution maps take the direct kernel's class-bias variant, csrc/conv_hr.hip; small ones the general kernel)
    assert ((L.load().csbsr_debug_last_conv_kernel() & 255) == 8) == (N * H * W >= 256 * 1024)
    assert relmax(from_fm(y), ref) < 2e-3


@pytest.mark.parametrize("cin,cout,k,s,p,OH,OW,mode", [
    (128, 128, 8, 4, 2, 19, 45, "prelu_sub"),      # up_conv2 / down_conv shapes, ragged tiles on both axes
    (128, 128, 8, 4, 2, 16, 64, "prelu_add"),      # whole tiles
    (64, 128, 8, 4, 2, 8, 32, "none"),             # one 64-channel chunk per phase
    (192, 100, 8, 4, 1, 9, 40, "lrelu"),           # three chunks per phase (odd chunk count), padded couts, another padding
    (256, 200, 4, 2, 1, 12, 33, "none_add"),       # 4x4 stride 2: four phases, two cout tiles
])
def test_phase_accumulated_strided_conv(cin, cout, k, s, p, OH, OW, mode):
    """The k = 2 x stride convolutions (8x8 stride 4: DownBlock / UpBlock strided convs, dgrads of the deconvolutions) through
    conv_x3_kernel<2> (csrc/conv_x3.hip: one chunk per input phase and 64 channels, 2 x 2 taps on the phase's sub-sampled halo tile)
    against F.conv2d on the same fp16-rounded operands and against the implicit-GEMM kernel: forward with the fused epilogues the
    blocks use, and the dgrad of the matching ConvTranspose2d accumulating into an existing gradient."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, pad8
    torch.manual_seed(cin + cout + OH * OW)
    eng = _eng()
    lib = L.load()
    N = 2
    H, W = s * (OH - 1) + k - 2 * p, s * (OW - 1) + k - 2 * p
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cout, cin, k, k) / (cin * k * k) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    a0 = torch.tensor([0.25])
    actn = mode.split("_")[0]
    act = {"prelu": L.ACT_PRELU, "lrelu": L.ACT_LRELU, "none": L.ACT_NONE}[actn]
    params = {"l.weight": w.cuda(), "l.bias": b.cuda(), "a": a0.clone().cuda()}
    conv = Conv(eng, "l", params, k, s, p, 1, bias=True, act=act, slope=0.1, prelu="a" if act == L.ACT_PRELU else None)
    pre = F.conv2d(x, w, b, s, p)
    assert pre.shape[-2:] == (OH, OW)
    ref = {"prelu": F.prelu(pre, a0), "lrelu": F.leaky_relu(pre, 0.1), "none": pre}[actn]
    res = torch.randn_like(ref).half().float()
    kw = {}
    if mode.endswith("_add"):
        ref = ref + res; kw = dict(res=res, res_mode=L.RES_ADD)
    if mode.endswith("_sub"):
        ref = ref - res; kw = dict(res=res, res_mode=L.RES_SUB)
    # the dgrad of ConvTranspose2d(cout -> cin) with an IOHW weight [cout][cin]: a strided conv over dOut contracting its cin
    wt = (torch.randn(cout, cin, k, k) / (cin * 4) ** 0.5).half().float()
    tconv = Conv(eng, "t", {"t.weight": wt.cuda()}, k, s, p, 1, transposed=True, bias=False, act=L.ACT_NONE)
    dpre = torch.randn(N, cin, H, W).half().float()          # gradient wrt the deconv's (H x W) output
    old = torch.randn(N, cout, OH, OW).half().float()
    zr = torch.zeros(N, cout, OH, OW, requires_grad=True)
    yt = F.conv_transpose2d(zr, wt, None, s, p)
    assert yt.shape[-2:] == (H, W)
    yt.backward(dpre)
    refd = zr.grad + old
    outs = []
    for x3_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3(x3_mode)
        try:
            conv.invalidate(); tconv.invalidate()
            y = conv.fwd(to_fm(eng, x), **{k_: (to_fm(eng, v) if isinstance(v, torch.Tensor) else v) for k_, v in kw.items()})
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) in (12, 18)) == (x3_mode == 2 and pad8(cout) >= 72)
            dz = to_fm(eng, old)
            tconv.bwd_input(to_fm(eng, dpre), out=dz, accumulate=True, in_hw=(OH, OW))
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) in (12, 18)) == (x3_mode == 2 and pad8(cout) >= 72)
        finally:
            lib.csbsr_debug_set_conv_x3(1)
        outs.append((from_fm(y), from_fm(dz)))
        assert relmax(outs[-1][0], ref) < 2e-3
        assert relmax(outs[-1][1], refd) < 2e-3
    assert relmax(outs[0][0], outs[1][0]) < 1e-3 and relmax(outs[0][1], outs[1][1]) < 1e-3


@pytest.mark.parametrize("k,s,p,cout,H,W,mode", [(8, 4, 2, 128, 13, 21, "prelu_add"), (8, 4, 2, 128, 16, 16, "prelu"), (12, 8, 2, 128, 7, 9, "prelu_add"),
                                               (8, 4, 2, 64, 10, 12, "none_sub"), (8, 4, 2, 49, 10, 12, "prelu")])
def test_thin_transposed_conv_from_image(k, s, p, cout, H, W, mode):
    """kb.up_conv1 (DeconvBlock 3 -> 128, 8x8 stride 4 / 12x12 stride 8, PReLU, + residual): the streaming kernel
    conv_thin_tp_kernel (csrc/conv_thin.hip) against conv_transpose2d on fp16-rounded operands; 49 couts (7 octets) is not eligible
    and must come out right through the general kernel."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, pad8
    torch.manual_seed(k + cout + H)
    eng = _eng()
    N, cin = 2, 3
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cin, cout, k, k) / (cin * 4) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    a = torch.tensor([0.25])
    act = {"prelu": L.ACT_PRELU, "none": L.ACT_NONE}[mode.split("_")[0]]
    conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda(), "a": a.cuda()}, k, s, p, 1, transposed=True, bias=True, act=act,
                prelu="a" if act == L.ACT_PRELU else False)
    pre = F.conv_transpose2d(x, w, b, s, p)
    ref = F.prelu(pre, a) if act == L.ACT_PRELU else pre
    res = torch.randn_like(ref).half().float()
    rm = L.RES_ADD if mode.endswith("_add") else (L.RES_SUB if mode.endswith("_sub") else L.RES_NONE)
    if rm == L.RES_ADD: ref = ref + res
    if rm == L.RES_SUB: ref = ref - res
    y = conv.fwd(to_fm(eng, x), res=to_fm(eng, res) if rm != L.RES_NONE else None, res_mode=rm)
    torch.cuda.synchronize()
    c8 = pad8(cout) // 8
    assert ((L.load().csbsr_debug_last_conv_kernel() & 255) == 11) == (256 % c8 == 0 and (256 // c8) % s == 0)
    assert relmax(from_fm(y), ref) < 2e-3


@pytest.mark.parametrize("H,W", [(16, 32), (8, 64)])
def test_phase_decomposed_dgrad_with_the_residual_layers_epilogue_backward(H, W):
    """down_conv3's dgrad completing d(dd) where the layer below is down_conv2, out = PReLU(deconv + b) - xd (kbpn.py:254-256): the
    activation is rebuilt as (dd + xd), the masked gradient + bias / slope sums leave as for the plain case, and d(xd) = -dOut is the
    second output -- against torch autograd of  conv2d(prelu(z + b, a) - xd)."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, grad_acc
    torch.manual_seed(H + W)
    eng = _eng()
    lib = L.load()
    N, C, k, s, p = 2, 128, 8, 4, 2
    IH, IW = s * H, s * W
    w = (torch.randn(C, C, k, k) / (C * 4) ** 0.5).half().float()
    conv = Conv(eng, "l", {"l.weight": w.cuda()}, k, s, p, 1, bias=False, act=L.ACT_NONE)
    a0, b0 = torch.tensor([0.25]), (torch.randn(C) * 0.1)
    pb = {"b.weight": torch.zeros(C, C, k, k).cuda(), "b.bias": b0.clone().cuda(), "a": a0.clone().cuda()}
    below = Conv(eng, "b", pb, k, s, p, 1, transposed=True, bias=True, act=L.ACT_PRELU, prelu="a")
    below.frozen = False
    act16 = F.prelu(torch.randn(N, C, IH, IW) + b0[None, :, None, None], a0).half().float()       # act(pre) as stored
    xd = torch.randn(N, C, IH, IW).half().float()
    dd = (act16 - xd).half().float()                     # the saved output of the layer below
    y = dd + xd                                          # what the kernel rebuilds the activation from
    dpre = torch.randn(N, C, H, W).half().float()
    ddr = dd.clone().requires_grad_(True)
    (F.conv2d(ddr, w, None, s, p) * dpre).sum().backward()
    dy = ddr.grad                                        # d(dd): no accumulate in this launch
    neg = ~(y > 0)
    ref_dz = torch.where(neg, dy * a0, dy)
    ref_db = ref_dz.sum((0, 2, 3))
    ref_da = (dy * (y / a0))[neg].sum()
    lib.csbsr_debug_set_conv_tp(2)
    try:
        dxd = to_fm(eng, torch.zeros_like(xd))
        out = conv.bwd_input(to_fm(eng, dpre), in_hw=(IH, IW), dact=(below, to_fm(eng, dd)), dres=(to_fm(eng, xd), dxd, L.RES_SUB))
        torch.cuda.synchronize()
    finally:
        lib.csbsr_debug_set_conv_tp(1)
    assert conv.last_fused and (lib.csbsr_debug_last_conv_kernel() & 255) == 9
    assert relmax(from_fm(out), ref_dz) < 2e-3
    assert relmax(from_fm(dxd), -dy) < 2e-3
    assert relmax(grad_acc(pb["b.bias"]).cpu(), ref_db) < 2e-3
    assert abs(float(grad_acc(pb["a"]).cpu()) - float(ref_da)) < 2e-3 * float((dy * (y / a0))[neg].abs().sum()) ** 0.5 + 2e-3 * abs(float(ref_da))



# ---------------------------------------------------------------------------------------------- split-fp16 (hi + lo) forward convs
def to_fm_split(eng, x):      # NCHW fp32 cpu -> split FM (value = hi + lo)
    from csbsr_amd.engine import pad8
    N, C, H, W = x.shape
    fm = eng.new(N, H, W, C, zero=True, split=True)
    v = x.permute(0, 2, 3, 1).contiguous()
    hi = v.half()
    fm.t[..., :C] = hi.cuda()
    fm.t.as_strided(fm.t.shape, fm.t.stride(), fm.t.storage_offset() + fm.lo)[..., :C] = (v - hi.float()).half().cuda()
    return fm


def from_fm_split(fm):
    lo = fm.t.as_strided(fm.t.shape, fm.t.stride(), fm.t.storage_offset() + fm.lo)
    return (fm.t[..., :fm.c].float() + lo[..., :fm.c].float()).cpu().permute(0, 3, 1, 2)


SPLIT_CASES = [
    # cin, cout, k, stride, pad, dil, H, W, N          (input channels a multiple of 32: the fused form; else the three-block form)
    (64, 64, 3, 1, 1, 1, 40, 70, 2),          # 64-cout tile, ragged pixel tiles
    (128, 128, 3, 1, 1, 1, 24, 24, 2),        # 128 x 128 tile
    (64, 128, 3, 2, 1, 1, 48, 64, 2),         # strided
    (512, 512, 3, 1, 2, 2, 64, 64, 4),        # dilated, 256 px x 256 cout tile (K >= 2304, >= 65536 px at N >= 16: forced below by the size)
    (256, 256, 3, 1, 1, 1, 192, 192, 2),      # 256 x 256 tile, 2-D pixel tiles
    (1024, 256, 3, 1, 1, 1, 96, 96, 8),       # up_1
    (2560, 1024, 1, 1, 0, 1, 24, 24, 2),      # PSP bottleneck (1x1)
    (96, 192, 3, 2, 1, 1, 40, 40, 2),         # HRNet transition (32-multiple that is not a 64-multiple)
    (48, 48, 3, 1, 1, 1, 40, 40, 2),          # HRNet branch width 48: a 32-channel K slice straddles taps (fused form + general K walk)
    (48, 192, 3, 2, 1, 1, 40, 40, 2),
    (720, 512, 3, 1, 1, 1, 20, 24, 2),
    (64, 505, 3, 1, 1, 1, 20, 24, 2),         # blur_skip conv0 feature part
]


@pytest.mark.parametrize("case", SPLIT_CASES)
@pytest.mark.parametrize("fused", [1, 0])
def test_split_precision_forward_conv(case, fused):
    """The detector precision mode's forward conv (x_hi w_hi + x_lo w_hi + x_hi w_lo in one fp32 accumulator) in its fused form (one
    staged K slice of [x_hi | x_lo] x [w_hi | w_lo] feeds all three products) and its three-block form, against fp64 torch on the SAME
    hi + lo input: ~22 mantissa bits -> 2e-5 of the output's maximum (fp32 accumulation over up to 2.3e4 terms included), BatchNorm sums
    to 1e-5 relative; the two forms agree with each other to accumulation-order noise."""
    from csbsr_amd.engine import Conv
    from csbsr_amd import _lib as L
    cin, cout, k, stride, pad, dil, H, W, N = case
    eng = _eng()
    eng.split_fused = bool(fused)
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    xs = to_fm_split(eng, x)
    xv = from_fm_split(xs).double()                 # what the kernel actually sees
    conv = Conv(eng, "l", {"l.weight": w.cuda()}, k, stride, pad, dil, bias=False)
    from csbsr_amd.engine import pad8
    stat = eng.f32(2, pad8(cout))
    out = conv.fwd(xs, stat=stat, stat_mode=L.STAT_BN)
    torch.cuda.synchronize()
    assert out.lo, "the output of a split conv is a hi + lo pair"
    ref = F.conv2d(xv, w.double(), None, stride, pad, dil)
    got = from_fm_split(out).double()
    err = float((got - ref).abs().max() / ref.abs().max())
    s_ref = torch.stack([ref.sum((0, 2, 3)), (ref * ref).sum((0, 2, 3))])
    e_stat = float((stat[:, :cout].double().cpu() - s_ref).abs().max() / s_ref.abs().max())
    print(f"split conv {case} fused={fused}: max err {err:.2e} of max, BN sums {e_stat:.2e}")
    assert err < 2e-5 and e_stat < 1e-5


@pytest.mark.parametrize("cin,cout,H,W,mode", [
    (512, 64, 19, 70, "lrelu"),             # ragged tiles on both axes (two tile columns), 16 chunks
    (505, 64, 16, 64, "none_add"),          # blur_skip conv1 shape: 505 -> 512 padded input channels, residual add
    (505, 64, 9, 130, "sigmoid"),           # three tile columns, the general (non-straight-line) epilogue row
    (96, 40, 8, 64, "relu"),                # three chunks (odd: the halo buffers alternate across chunks; 2 tiles, one per workgroup -- the
                                            # multi-tile walk runs under CU budgets in tests/test_conv_exact_gpu.py), 40 -> 40 padded couts
    (288, 64, 24, 33, "none"),
    (64, 505, 19, 70, "lrelu"),             # the WIDE form (8 x 32 pixels x 128 couts, two workgroups per CU): blur_skip conv0 shape, ragged tiles
    (128, 200, 9, 40, "none_add"),          # four chunks, 200 -> 256 padded weight rows (the second cout tile half empty), residual add
    (96, 136, 8, 33, "sigmoid"),            # three chunks, the general epilogue row
])
def test_narrow_output_3x3_kernel(cin, cout, H, W, mode):
    """csrc/conv_x3n.hip (8 x 64-pixel x 64-cout tile, per-32-channel halo tile in LDS, fragment-ordered weights from L2) against F.conv2d
    on the same fp16-rounded operands and against the LDS-DMA kernels: forward with fused epilogue modes, and -- the other launch shape it
    takes in the model -- the dgrad of the REVERSE convolution (cout -> cin channels: flipped, transposed weights) accumulating."""
    from csbsr_amd import _lib as L
    from csbsr_amd.engine import Conv, pad8
    torch.manual_seed(cin + cout + H)
    eng = _eng()
    lib = L.load()
    N = 2
    x = torch.randn(N, cin, H, W).half().float()
    w = (torch.randn(cout, cin, 3, 3) / (cin * 9) ** 0.5).half().float()
    b = torch.randn(cout) * 0.1
    act = {"lrelu": L.ACT_LRELU, "relu": L.ACT_RELU, "none": L.ACT_NONE, "sigmoid": L.ACT_SIGMOID}[mode.split("_")[0]]
    conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True, act=act, slope=0.1)
    pre = F.conv2d(x, w, b, 1, 1)
    ref = {L.ACT_LRELU: F.leaky_relu(pre, 0.1), L.ACT_RELU: F.relu(pre), L.ACT_NONE: pre, L.ACT_SIGMOID: torch.sigmoid(pre)}[act]
    res = torch.randn_like(ref).half().float()
    kw = {}
    if mode.endswith("_add"):
        ref = ref + res; kw = dict(res=res, res_mode=L.RES_ADD)
    # the reverse layer: a conv cout -> cin whose dgrad maps a cin-channel gradient to cout channels (many -> few)
    w2 = (torch.randn(cin, cout, 3, 3) / (cout * 9) ** 0.5).half().float()
    rev = Conv(eng, "r", {"r.weight": w2.cuda()}, 3, 1, 1, 1, bias=False)
    dpre = torch.randn(N, cin, H, W).half().float()
    old = torch.randn(N, cout, H, W).half().float()
    xr = torch.zeros(N, cout, H, W, requires_grad=True)
    F.conv2d(xr, w2, None, 1, 1).backward(dpre)
    refd = xr.grad + old
    outs = []
    elig = pad8(cin) % 32 == 0 and pad8(cout) > 32
    for xn_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3n(xn_mode)
        try:
            conv.invalidate(); rev.invalidate()
            y = conv.fwd(to_fm(eng, x), **{k_: (to_fm(eng, v) if isinstance(v, torch.Tensor) else v) for k_, v in kw.items()})
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 20) == (xn_mode == 2 and elig)
            dx = to_fm(eng, old)
            rev.bwd_input(to_fm(eng, dpre), out=dx, accumulate=True)
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 20) == (xn_mode == 2 and elig)
        finally:
            lib.csbsr_debug_set_conv_x3n(1)
        outs.append((from_fm(y), from_fm(dx)))
        assert relmax(outs[-1][0], ref) < 2e-3
        assert relmax(outs[-1][1], refd) < 2e-3
    assert relmax(outs[0][0], outs[1][0]) < 1e-3 and relmax(outs[0][1], outs[1][1]) < 1e-3


@pytest.mark.parametrize("cin,cout,H,W", [(505, 64, 16, 70), (256, 64, 9, 64), (64, 505, 16, 70)])
def test_narrow_output_3x3_kernel_split_input(cin, cout, H, W):
    """The two-product plan of a split (hi + lo) input on conv_x3n -- [x_hi | x_lo] w_hi as a plain convolution over 2 x Cp channels, the pack
    repeating the tap-sum-rounded weights for the lo plane, hi + lo output -- against fp64 torch on the SAME hi + lo input and the SAME
    rounded weights, and against the fused two-product stage of the LDS-DMA kernel."""
    from csbsr_amd.engine import Conv
    from csbsr_amd import _lib as L
    eng = _eng()
    lib = L.load()
    N = 2
    g = torch.Generator().manual_seed(cin * 7 + cout)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    xs = to_fm_split(eng, x)
    xv = from_fm_split(xs).double()
    outs = []
    for xn_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3n(xn_mode)
        try:
            conv = Conv(eng, "l", {"l.weight": w.cuda()}, 3, 1, 1, 1, bias=False)
            conv.fwd_blocks, conv.dc_comp = 2, True          # a layer of the two-product plan (build_model._runtime sets both)
            out = conv.fwd(xs)
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 20) == (xn_mode == 2)
            wq = conv._wq().float().cpu().double()               # the weights both forms multiply with: fp16 values (tap-sum-preserving rounding)
        finally:
            lib.csbsr_debug_set_conv_x3n(1)
        assert out.lo
        outs.append(from_fm_split(out).double())
    # reference on the rounded weights + the mean compensation's bias (engine.Conv._dc_bias gives back the rounding residual's response to
    # the per-sample channel means): compare against the exact product with the UNROUNDED weights at the plan's own tolerance instead
    ref_q = F.conv2d(xv, wq, None, 1, 1)
    ref = F.conv2d(xv, w.double(), None, 1, 1)
    e01 = float((outs[0] - outs[1]).abs().max() / ref.abs().max())
    eq = float(((outs[0] - outs[1])).abs().max() / ref.abs().max())
    e_ref = float((outs[0] - ref).abs().max() / ref.abs().max())
    print(f"   conv_x3n split {cin}->{cout}: vs the fused LDS-DMA stage {e01:.2e}, vs fp64 on unrounded weights {e_ref:.2e}")
    assert e01 < 2e-5                 # the same arithmetic in a different summation order
    assert e_ref < 2e-3               # the two-product plan keeps the weights' fp16 rounding (minus its mean response)


def test_narrow_output_3x3_kernel_split_fma_residual():
    """BlurSkip's conv_shift.1 launch (csbsr_amd/modeling/pspnet.py: y = q * scale + shift, all three operands hi + lo pairs) on conv_x3n:
    the general epilogue row reads the split residual operands; against fp64 torch on the same hi + lo values and against the fused
    LDS-DMA stage."""
    from csbsr_amd.engine import Conv
    from csbsr_amd import _lib as L
    eng = _eng()
    lib = L.load()
    N, cin, cout, H, W = 2, 505, 64, 11, 70
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, cin, H, W, generator=g)
    qv = torch.randn(N, cout, H, W, generator=g)
    sc = torch.randn(N, cout, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    xs, qs, ss = to_fm_split(eng, x), to_fm_split(eng, qv), to_fm_split(eng, sc)
    outs = []
    for xn_mode in (2, 0):
        lib.csbsr_debug_set_conv_x3n(xn_mode)
        try:
            conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True)
            conv.fwd_blocks, conv.dc_comp = 2, True
            out = conv.fwd(xs, res=qs, res2=ss, res_mode=L.RES_FMA)
            torch.cuda.synchronize()
            assert ((lib.csbsr_debug_last_conv_kernel() & 255) == 20) == (xn_mode == 2)
        finally:
            lib.csbsr_debug_set_conv_x3n(1)
        outs.append(from_fm_split(out).double())
    ref = F.conv2d(from_fm_split(xs).double(), w.double(), b.double(), 1, 1) + from_fm_split(qs).double() * from_fm_split(ss).double()
    e01 = float((outs[0] - outs[1]).abs().max() / ref.abs().max())
    e_ref = float((outs[0] - ref).abs().max() / ref.abs().max())
    print(f"   conv_x3n split FMA residual: vs the fused LDS-DMA stage {e01:.2e}, vs fp64 {e_ref:.2e}")
    assert e01 < 2e-5 and e_ref < 2e-3


@pytest.mark.parametrize("split", [0, 1])
def test_narrow_output_3x3_kernel_fused_batchnorm_sums(split):
    """conv_x3n with the fused BatchNorm statistics (per-lane register sums over a workgroup's tiles, xor-shuffle + wave-ordered LDS fold,
    one partial row per workgroup, fixed-order fold by csbsr_sum_partials): sum and sum of squares per channel against fp64 on the kernel's own
    output, bit-identical twice, for a plain input and for the two-product plan of a split input (the PSPNet decoder's up_2 / up_3 shape)."""
    from csbsr_amd.engine import Conv, pad8
    from csbsr_amd import _lib as L
    eng = _eng()
    lib = L.load()
    N, cin, cout, H, W = 2, 128, 64, 21, 100
    g = torch.Generator().manual_seed(31 + split)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    xs = to_fm_split(eng, x) if split else to_fm(eng, x)
    stats = []
    lib.csbsr_debug_set_conv_x3n(2)
    try:
        for rep in range(2):
            conv = Conv(eng, "l", {"l.weight": w.cuda()}, 3, 1, 1, 1, bias=False)
            if split:
                conv.fwd_blocks, conv.dc_comp = 2, True
            stat = eng.f32(2, pad8(cout))
            out = conv.fwd(xs, stat=stat, stat_mode=L.STAT_BN)
            torch.cuda.synchronize()
            assert (lib.csbsr_debug_last_conv_kernel() & 255) == 20
            stats.append(stat.clone())
    finally:
        lib.csbsr_debug_set_conv_x3n(1)
    got = (from_fm_split(out) if split else from_fm(out)).double()
    s_ref = torch.stack([got.sum((0, 2, 3)), (got * got).sum((0, 2, 3))])
    e_stat = float((stats[0][:, :cout].double().cpu() - s_ref).abs().max() / s_ref.abs().max())
    print(f"   conv_x3n fused BN sums (split={split}): {e_stat:.2e}")
    assert e_stat < (1e-5 if split else 1e-3)       # (plain mode: the sums are of the fp32 values, the output is their fp16 rounding)
    assert torch.equal(stats[0], stats[1])


def test_fused_split_launch_falls_back_when_the_lds_dma_kernels_are_off():
    """engine.Conv._launch asks csbsr_conv_split_fused_eligible before it hands over the fused [w_hi | w_lo] operand: with the LDS-DMA
    kernels switched off (csbsr_debug_set_conv_glds(0), the debug mode the tests use to reach the register-staged kernels) the launch
    used to fail with 'split_fused launch not eligible'; now it runs the three-block form of the same operand, same result to
    accumulation-order noise."""
    from csbsr_amd.engine import Conv
    from csbsr_amd import _lib as L
    eng = _eng()
    cin, cout, H, W, N = 64, 128, 24, 40, 2
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    xs = to_fm_split(eng, x)
    ref = F.conv2d(from_fm_split(xs).double(), w.double(), None, 1, 1)
    outs = []
    try:
        for mode in (2, 0):
            L.load().csbsr_debug_set_conv_glds(mode)
            conv = Conv(eng, "l", {"l.weight": w.cuda()}, 3, 1, 1, 1, bias=False)
            out = conv.fwd(xs)
            torch.cuda.synchronize()
            kid = L.load().csbsr_debug_last_conv_kernel()
            assert ((kid & 255) in (3, 4, 7, 14)) == (mode == 2) and (mode == 0 or (kid >> 8) & 1), (mode, kid)      # LDS-DMA + FS | register-staged
            outs.append(from_fm_split(out).double())
            assert float((outs[-1] - ref).abs().max() / ref.abs().max()) < 2e-5, mode
    finally:
        L.load().csbsr_debug_set_conv_glds(2)
    assert float((outs[0] - outs[1]).abs().max() / ref.abs().max()) < 1e-5


@pytest.mark.parametrize("cin,split", [(64, 1), (64, 0), (256, 1), (128, 0)])
def test_one_channel_head_kernels(cin, split):
    """csbsr_head1_fwd / csbsr_head1_bwd_input (the 1-channel sigmoid heads of PSPNet: fp32 VALU dot product over a pixel's channels, the
    split planes summed, weights unrounded) through engine.Conv against fp64 torch on the same (hi + lo) input, and against the general
    convolution kernels (CSBSR_HEAD1 = 0 path)."""
    from csbsr_amd.engine import Conv
    from csbsr_amd import _lib as L
    eng = _eng()
    N, H, W = 2, 19, 37
    g = torch.Generator().manual_seed(5 + cin + split)
    x = torch.randn(N, cin, H, W, generator=g)
    w = torch.randn(1, cin, 1, 1, generator=g) * (1.0 / cin) ** 0.5
    b = torch.tensor([0.3])
    xs = to_fm_split(eng, x) if split else to_fm(eng, x)
    xv = (from_fm_split(xs) if split else from_fm(xs)).double()
    ref = torch.sigmoid(F.conv2d(xv, w.double(), b.double()))
    dpre = torch.randn(N, 1, H, W, generator=g).half().float()
    refd = (dpre.double() * w.double().reshape(1, cin, 1, 1))
    outs = []
    for on in (True, False):
        eng.use_head1 = on
        conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 1, bias=True, act=L.ACT_SIGMOID)
        o32 = torch.empty(N, 1, H, W, device="cuda")
        conv.fwd(xs, out32=o32)
        dx = conv.bwd_input(to_fm(eng, dpre))
        torch.cuda.synchronize()
        kid = L.load().csbsr_debug_last_conv_kernel() & 255
        outs.append((o32.cpu().double(), from_fm(dx).double()))
        assert float((outs[-1][0] - ref).abs().max()) < (2e-6 if (on or split) else 2e-3), (on, float((outs[-1][0] - ref).abs().max()))
        assert relmax(outs[-1][1], refd) < 2e-3
    eng.use_head1 = True
    assert float((outs[0][0] - outs[1][0]).abs().max()) < 2e-3 and relmax(outs[0][1], outs[1][1]) < 2e-3
