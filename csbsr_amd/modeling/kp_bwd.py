"""Backward of the per-stage kernel predictor: weight gradients taken from passes that already read the maps (KBPN.kp_pairs).

* ``fold_const_wgrad``: fe_cat.2 sits in front of the global average pool, so its dPre is one vector per sample.  The weight gradient of
  a zero-padded 3x3 conv under a constant dPre needs only the 16 border-class sums of the layer's input -- which the masked fill that
  is this layer's dgrad (KBPN._fold_const_dgrad) streams as its mask operand (csbsr_border_class_fill_masked_sums).
* ``pair1x1_backward``: fe_SR.1 and fe_cat.0 are 1x1 layers whose dgrad applies the activation derivative of the layer below, i.e. reads
  dPre and the layer's own input -- the two operands of the layer's weight gradient.  One kernel produces both (csrc/conv_pair.hip);
  the input gradient is bit-identical to ``conv.bwd_input(dpre, seg=0, mask=(x, slope))``.
"""
import torch

from .. import _lib as L
from ..engine import _ptr, grad_acc, pad8


def fold_const_wgrad(conv, gvec, sums, mtap):
    """wgrad of a zero-padded 3x3 stride-1 conv whose dPre is spatially constant per sample (``gvec`` [B, cout] fp32; the MFMA path reads
    it rounded to fp16, KBPN._bcast_grad) from the border-class sums ``sums`` [B, 16, cp] of the layer's input:
    G[o, c, ky, kx] = sum_n g[n, o] * sum_{a, b} sums[n, a, b, c] mf[a, ky] mf[b, kx] -- an input pixel q meets tap (ky, kx) exactly when
    the output pixel q - (ky - 1, kx - 1) lies inside the image, the flipped tap mask of the dgrad fold.  Exact; fp32 like
    Conv.bwd_weights_folded.  Adds into the layer's gradient accumulator."""
    B, cin = gvec.shape[0], conv.cin
    g16 = gvec.to(torch.float16).float()
    mf = mtap.flip(1)
    S = torch.einsum("nabc,ay,bx->ncyx", sums[:, :, :cin].reshape(B, 4, 4, cin), mf, mf)
    grad_acc(conv.w).add_(torch.einsum("no,ncyx->ocyx", g16, S))


def const_wgrad_ok(conv):
    """layers fold_const_wgrad takes: the shape of KBPN._fold_const_dgrad (3x3, stride 1, zero padding 1, one input segment, no bias)"""
    return (not conv.transposed and conv.k == 3 and conv.stride == 1 and conv.pad == 1 and conv.dil == 1 and conv.split[1] == 0
            and conv.b is None)


def pair1x1_ok(conv, dpre, x, seg0=None):
    """may ``pair1x1_backward`` take this layer's backward?  1x1, stride 1, bias-free, 32 output channels, 49..56 real input channels in
    the segment the gradient is for (stored as 56), plain fp16 maps, the direct full-resolution kernel switched on (whose dgrad the
    pair kernel reproduces bit for bit)"""
    c0 = conv.split[0] if seg0 is None else seg0
    return (conv.eng.use_hr and not conv.transposed and conv.k == 1 and conv.stride == 1 and conv.pad == 0 and conv.b is None
            and not conv.hp_dgrad and conv.cout == 32 and dpre.cp == 32 and pad8(c0) == 56 and x.cp == 56 and x.c == c0
            and c0 <= conv.w.shape[1] and not (dpre.bcast or x.bcast or dpre.lo or x.lo)
            and (dpre.N, dpre.H, dpre.W) == (x.N, x.H, x.W))


def pair1x1_backward(conv, dpre, x, mask_slope, seg0=None):
    """dIn = (dPre . W[:, :seg0]) x (x > 0 ? 1 : mask_slope) and grad(W)[:, :seg0] += sum_pix dPre (x) x in one pass over ``dpre`` and
    ``x`` (the layer's saved input = the saved output of the layer below, whose negative slope is ``mask_slope``).  Returns dIn."""
    eng = conv.eng
    c0 = conv.split[0] if seg0 is None else seg0
    assert pair1x1_ok(conv, dpre, x, seg0)
    # the dgrad operand of the direct full-resolution kernel, from the same cache entry Conv.bwd_input fills (engine.FAMILIES)
    key = ("hr", 1, 0)
    wt = conv._packed.get(key)
    if wt is None:
        wt = conv._pack_new(key, conv._wq(), "csbsr_packed_weight_elems_hr", (1, conv.cout, c0),
                            "csbsr_pack_weights_hr", (1, 1, *conv.w.shape[:2], conv.cout, c0, 0, 0))
    N, H, W = dpre.N, dpre.H, dpre.W
    out = eng.new(N, H, W, c0)
    ns = int(L.load().csbsr_conv_pair1x1_slabs(N, H, W, eng.stream))
    slabs = eng.workspace(ns * 32 * 56)
    L.call("csbsr_conv_pair1x1_backward", _ptr(dpre.t), *dpre.strides(), _ptr(x.t), *x.strides(), _ptr(wt), float(mask_slope), N, H, W,
           _ptr(out.t), *out.strides(), _ptr(slabs), eng.stream)
    L.call("csbsr_unpack_wgrad", _ptr(slabs), _ptr(grad_acc(conv.w)), 32, 1, 1, c0, 0, conv.w.shape[0], conv.w.shape[1], 0, 0, 1.0, ns, 32,
           eng.stream)
    return out
