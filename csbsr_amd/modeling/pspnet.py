"""PSPNet (dilated ResNet-34 + pyramid pooling + 3 upsample stages + aux head) on the HIP engine.

Counterpart of /root/reference/model/modeling/pspnet_pytorch/pspnet.py:23-123 and extractors.py:41-70,
112-161 with the reference's parameter names; train-mode BatchNorm statistics come from the conv
epilogue, Dropout2d channel masks are fused into the following resize / BN-apply, the PSP concat buffer is
written in place by its producers.  Explicit backward; what it needs rides on a per-forward tape (blocks.py).
"""
import os

import torch

from .. import _lib as L
from ..engine import FM, Conv, _ptr
from .blocks import ConvBN, act_bwd, sft_bwd
from .kbpn import border_tap_mask
from .shapes import RESNET34

DROP_P = {"drop_1": 0.3, "drop_2a": 0.15, "drop_2b": 0.15, "drop_2c": 0.15, "aux_drop": 0.1}   # pspnet.py:67,73,83
DROP_C = {"drop_1": 1024, "drop_2a": 256, "drop_2b": 64, "drop_2c": 64, "aux_drop": 256}


class _SFTLike:
    """SFTLikeBlock (blocks.py:86-120): features * sigmoid(conv(prelu(conv(cat)))) + conv(prelu(conv(cat))), cat = features ++ the
    spatially constant kernel code -- the constant 441 channels are folded into border-class biases (Conv.fwd_folded)."""

    def __init__(self, eng, P, pre, cf, cconst):
        def mk(name, act, prelu):
            return Conv(eng, f"{pre}.{name}.layer", P, 3, 1, 1, bias=True, act=act, prelu=f"{pre}.{name}.act.weight" if prelu else False,
                        split=(cf, cconst) if prelu else None)
        self.sc0, self.sc1 = mk("conv_scale.0", L.ACT_PRELU, True), mk("conv_scale.1", L.ACT_SIGMOID, False)
        self.sh0, self.sh1 = mk("conv_shift.0", L.ACT_PRELU, True), mk("conv_shift.1", L.ACT_NONE, False)

    def convs(self):
        return [self.sc0, self.sc1, self.sh0, self.sh1]


class _ResBlock:
    """BasicBlock of the dilated ResNet (extractors.py:41-70): relu(bn2(conv2(relu(bn1(conv1(x))))) + downsample(x))"""

    def __init__(self, eng, P, pre, stride, dil, down, layer):
        self.eng, self.layer = eng, layer
        self.c1 = ConvBN(eng, P, pre + ".conv1", pre + ".bn1", 3, stride, dil, dil)
        self.c2 = ConvBN(eng, P, pre + ".conv2", pre + ".bn2", 3, 1, dil, dil)
        self.down = ConvBN(eng, P, pre + ".downsample.0", pre + ".downsample.1", 1, stride, 0, act=L.ACT_NONE) if down else None

    def units(self):
        return [self.c1, self.c2] + ([self.down] if self.down else [])

    def fwd(self, x, training, tape, out=None):
        a1 = self.c1.fwd(x, training, tape)
        pre = self.c2.conv_stats(a1, training)
        res = self.down.fwd(x, training, tape) if self.down else x
        return self.c2.fwd(a1, training, tape, res=res, out=out, pre=pre)

    def bwd(self, tape, dy):
        dres = self.eng.new(dy.N, dy.H, dy.W, dy.c)
        da1 = self.c2.bwd(tape, dy, dres=dres)
        g1 = self.c1.bwd_bn(tape, da1)
        del da1
        dx = self.down.bwd(tape, dres) if self.down else dres       # the downsample chain between c1's wgrad and its (accumulating) dgrad
        self.c1.bwd_dx(g1, out=dx, acc=True)
        return dx


class PSPNet:
    drop_keys = tuple(DROP_P)

    def __init__(self, eng, params, prefix="segmentation_model", blur_dim=None):
        """blur_dim: build PSPNet_BlurSkip (pspnet.py:127-207) whose forward also takes the kernel code [B, blur_dim]; in that
        variant only blur_skip.* is trainable (build_model.py:352-368), so the backward stops there."""
        self.eng, self.P, self.prefix = eng, params, prefix
        self.blur_dim = blur_dim
        self.blur_skip = []
        e, P, f = eng, params, prefix + ".feats"
        if blur_dim is not None:
            for i in range(2):
                bs = f"{prefix}.blur_skip.{2 * i + 1}"
                self.blur_skip.append((_SFTLike(e, P, f"{prefix}.blur_skip.{2 * i}", 64, blur_dim), ConvBN(e, P, bs + ".layer", bs + ".norm", 3)))
            self.Mtap = border_tap_mask().to(eng.device)
        self.stem = ConvBN(e, P, f + ".conv1", f + ".bn1", 7, 2)
        self.blocks = []
        inpl = 64
        for li, (planes, nblk, stride, dil) in enumerate(RESNET34, 1):
            for b in range(nblk):
                s_, d_ = (stride, 1) if b == 0 else (1, dil)
                self.blocks.append(_ResBlock(e, P, f"{f}.layer{li}.{b}", s_, d_, b == 0 and (stride != 1 or inpl != planes), li))
            inpl = planes
        self.x3_block = [b for b in self.blocks if b.layer == 3][-1]       # its output feeds the aux head
        self.psp_convs = [Conv(e, f"{prefix}.psp.stages.{i}.1", P, 1, bias=False) for i in range(4)]
        self.bottleneck = Conv(e, prefix + ".psp.bottleneck", P, 1, bias=True, act=L.ACT_RELU)
        self.ups = [ConvBN(e, P, f"{prefix}.{n}.conv.0", f"{prefix}.{n}.conv.1", 3, bias=True, act=L.ACT_PRELU, prelu=P[f"{prefix}.{n}.conv.2.weight"])
                    for n in ("up_1", "up_2", "up_3")]
        self.final = Conv(e, prefix + ".final.0", P, 1, bias=True, act=L.ACT_SIGMOID)
        self.aux0 = ConvBN(e, P, prefix + ".aux.0", prefix + ".aux.1", 3)
        self.aux4 = Conv(e, prefix + ".aux.4", P, 1, bias=True, act=L.ACT_SIGMOID)
        self.saved = None       # the tape of the last training forward (None otherwise); the train step moves it to its autograd node
        # "split": every forward activation of the detector is an fp16 hi + lo pair (~22 mantissa bits) and every forward conv runs
        # three MFMA passes (x_hi w_hi + x_lo w_hi + x_hi w_lo) in one fp32 accumulator; the backward reads the hi planes (BatchNorm /
        # max-pool backward also the lo planes, so their masks are the forward's).  Set by the model (detector_precision).
        self.split = False
        # split mode: how many of the three upsample stages, counted from the output, run plain fp16 again (their input is the hi plane of
        # the stage before).  Rounding introduced there only passes the remaining 1-2 conv + BatchNorm layers and the 1x1 head, so it is
        # not amplified like the trunk's, while those stages hold the largest maps of the detector (64 channels at HR / HR/2).
        self.split_tail_plain = int(os.environ.get("CSBSR_SPLIT_TAIL_PLAIN", "0"))

    def all_convs(self):
        cs = [u.conv for u in [self.stem] + [u for b in self.blocks for u in b.units()]]
        cs += self.psp_convs + [self.bottleneck] + [u.conv for u in self.ups] + [self.final, self.aux0.conv, self.aux4]
        for sft, cb in self.blur_skip:
            cs += sft.convs() + [cb.conv]
        return cs

    def invalidate(self):
        for c in self.all_convs():
            c.invalidate()

    def make_dropout(self, B, training, enabled=True):
        if not training or not enabled:
            return {k: None for k in DROP_P}
        out = {}
        for k, p in DROP_P.items():
            keep = (torch.rand(B, DROP_C[k], device=self.eng.device) >= p).to(torch.float32) / (1.0 - p)
            out[k] = keep.contiguous()
        return out

    # ------------------------------------------------------------------ forward
    def forward(self, xin, drop, training=True, kvec=None):
        """xin: FM [B,H,W,8] (3 real channels, already normalised); kvec [B, blur_dim] fp32 for the BlurSkip variant.
        Returns (seg32, aux32) fp32 [B,1,H,W].  A training forward with gradients enabled leaves its tape in ``self.saved``."""
        e = self.eng
        B, H, W = xin.N, xin.H, xin.W
        tape = {} if training and torch.is_grad_enabled() else None
        trunk = tape if self.blur_dim is None else None      # BlurSkip: the trunk is frozen, nothing of it is needed by the backward
        a = self.stem.fwd(xin, training, trunk)
        PH, PW = (a.H + 2 - 3) // 2 + 1, (a.W + 2 - 3) // 2 + 1
        x = e.new(B, PH, PW, 64, split=bool(a.lo))
        L.call("csbsr_maxpool3x3s2_fwd_split", _ptr(a.t), a.ld, a.lo, _ptr(x.t), x.ld, x.lo, B, a.H, a.W, 64, e.stream)
        pool = (a, x)
        for blk in self.blocks:
            out = None
            if blk is self.blocks[-1]:    # last block writes straight into the PSP concat buffer (channels 2048:2560)
                cat = e.new(B, x.H, x.W, 2560, split=bool(x.lo))
                out = cat.slice(2048, 2560)
            x = blk.fwd(x, training, trunk, out=out)
            if blk is self.x3_block:
                x3 = x
        fH, fW = x.H, x.W
        # pyramid pooling
        psp = []
        for i, size in enumerate((1, 2, 3, 6)):
            pooled = e.new(B, size, size, 512, split=bool(x.lo))
            L.call("csbsr_adaptive_avgpool_fwd_split", _ptr(x.t), x.ld, x.lo, _ptr(pooled.t), pooled.ld, pooled.lo, B, fH, fW, 512, size, size,
                   e.stream)
            pc = self.psp_convs[i].fwd(pooled)
            e.bilinear(pc, fH, fW, False, out=cat.slice(512 * i, 512 * (i + 1)))
            psp.append((pooled, pc))
        bott = self.bottleneck.fwd(cat)
        # upsample stages; the dropout that follows stage j is fused into stage j+1's resize (or the last BN apply)
        cur, cur_drop = bott, drop["drop_1"]
        ups = []
        for j, (up, name) in enumerate(zip(self.ups, ("drop_2a", "drop_2b", "drop_2c"))):
            if cur.lo and j >= len(self.ups) - self.split_tail_plain:
                cur = FM(cur.t, cur.c, H=cur.H, W=cur.W)          # the hi plane alone: this stage and everything after it is plain fp16
            u = e.bilinear(cur, cur.H * 2, cur.W * 2, False, drop=cur_drop)
            ups.append((cur, cur_drop))
            cur, cur_drop = up.fwd(u, training, trunk, drop=drop[name] if j == 2 else None), drop[name]
        if trunk is not None:
            tape.update(pool=pool, psp=(cat, psp, bott), ups=ups)
        if self.blur_dim is not None:
            cur = self._blur_skip_fwd(cur, kvec, training, tape)
        seg32 = e.f32(B, 1, H, W, zero=False)
        self.final.fwd(cur, out32=seg32)
        # aux head on layer3 output
        aa = self.aux0.fwd(x3, training, trunk, drop=drop["aux_drop"])
        aux_lo = e.f32(B, 1, x3.H, x3.W, zero=False)
        self.aux4.fwd(aa, out32=aux_lo)
        aux32 = e.f32(B, 1, H, W, zero=False)
        L.call("csbsr_bilinear32_fwd", _ptr(aux_lo), _ptr(aux32), B, x3.H, x3.W, H, W, 1, e.stream)
        if tape is not None:
            tape.update(seg32=seg32, p3=cur)
        if trunk is not None:
            tape["aux"] = (aa, aux_lo)
        self.saved = tape
        return seg32, aux32

    # ------------------------------------------------------------------ BlurSkip branch (pspnet.py:191-198)
    def _blur_skip_fwd(self, p, kvec, training, tape):
        e = self.eng
        q, bsv = p, []
        for sft, cb in self.blur_skip:
            t1, f1 = sft.sc0.fwd_folded(q, kvec, self.Mtap)
            sc = sft.sc1.fwd(t1)
            t2, f2 = sft.sh0.fwd_folded(q, kvec, self.Mtap)
            y = sft.sh1.fwd(t2, res=q, res2=sc, res_mode=L.RES_FMA)              # q * scale + shift
            bsv.append((q, (t1, f1, sc, t2, f2, y)))
            q = cb.fwd(y, training, tape)
        out = e.new(p.N, p.H, p.W, p.c, split=bool(p.lo))
        L.call("csbsr_axpby_split", p.npix, p.cp, _ptr(p.t), p.ld, p.lo, 1.0, _ptr(q.t), q.ld, q.lo, 1.0, _ptr(out.t), out.ld, out.lo,
               e.stream)    # p + _p
        if tape is not None:
            tape["blur_skip"] = bsv
        return out

    def _blur_skip_bwd(self, tape, d):
        """d: gradient wrt (p + _p).  Accumulates the blur_skip.* gradients; nothing upstream of it is trainable."""
        bsv = tape.pop("blur_skip")
        for i in (1, 0):
            sft, cb = self.blur_skip[i]
            q, saves = bsv.pop()
            dy = cb.bwd(tape, d)
            del d
            dq = self.eng.new(q.N, q.H, q.W, q.c) if i > 0 else None      # block 0's input is the frozen trunk's output
            sft_bwd(sft.sc0, sft.sc1, sft.sh0, sft.sh1, saves, q, dy, self.Mtap, dx=dq)
            del dy, saves
            d = dq

    # ------------------------------------------------------------------ backward
    def _sigmoid_head_bwd(self, conv, dprob32, prob32, x, frozen=False):
        """1-channel sigmoid head: returns dgrad wrt x; accumulates weight / bias grads."""
        e = self.eng
        B, _, H, W = prob32.shape
        dpre = e.new(B, H, W, 1)
        L.call("csbsr_sigmoid_bwd_to_nhwc8", _ptr(dprob32), _ptr(prob32), _ptr(dpre.t), B * H * W, 1.0, e.stream)
        if not frozen:
            act_bwd(conv, dpre)
            conv.bwd_weights(dpre, x)
        return conv.bwd_input(dpre)

    def backward(self, dseg32, daux32, need_dxin=True):
        """Gradients (scaled) wrt the two probability maps -> returns FM gradient wrt xin [B,H,W,8]; ``need_dxin=False`` (the input is no
        function of a parameter: MODEL.SR="bicubic") skips the stem's input gradient and returns None.  Consumes ``self.saved``."""
        e = self.eng
        tape, self.saved = self.saved, None
        B, _, H, W = dseg32.shape
        if self.blur_dim is not None:
            self._blur_skip_bwd(tape, self._sigmoid_head_bwd(self.final, dseg32, tape.pop("seg32"), tape.pop("p3"), frozen=True))
            return None
        # aux head
        aa, aux_lo = tape.pop("aux")
        daux_lo = e.f32(B, 1, *aux_lo.shape[2:], zero=False)
        L.call("csbsr_bilinear32_bwd", _ptr(daux32), _ptr(daux_lo), B, *aux_lo.shape[2:], H, W, 1, e.stream)
        dx3_aux = self.aux0.bwd(tape, self._sigmoid_head_bwd(self.aux4, daux_lo, aux_lo, aa))
        del aa
        # main head, upsample stages
        d = self._sigmoid_head_bwd(self.final, dseg32, tape.pop("seg32"), tape.pop("p3"))
        ups = tape.pop("ups")
        for up in reversed(self.ups):
            cur, cur_drop = ups.pop()
            du = up.bwd(tape, d)
            d = e.new(B, cur.H, cur.W, cur.c)
            e.bilinear_bwd(du, d, False, False, drop=cur_drop)
            del du, cur
        cat, psp, bott = tape.pop("psp")
        act_bwd(self.bottleneck, d, bott)
        self.bottleneck.bwd_weights(d, cat)
        dcat = self.bottleneck.bwd_input(d)
        del d, bott
        fH, fW = cat.H, cat.W
        dy = dcat.slice(2048, 2560)
        for i, size in enumerate((1, 2, 3, 6)):
            pooled, pc = psp[i]
            dpc = e.new(B, size, size, 512)
            e.bilinear_bwd(dcat.slice(512 * i, 512 * (i + 1)), dpc, False, False)
            self.psp_convs[i].bwd_weights(dpc, pooled)
            dpool = self.psp_convs[i].bwd_input(dpc)
            L.call("csbsr_adaptive_avgpool_bwd", _ptr(dpool.t), _ptr(dy.t), dy.ld, 1, B, fH, fW, 512, size, size, e.stream)
        del cat, psp
        for blk in reversed(self.blocks):
            if blk is self.x3_block:       # the aux head's gradient joins where its input was tapped
                L.call("csbsr_axpby", dy.npix, dy.cp, _ptr(dy.t), dy.ld, 1.0, _ptr(dx3_aux.t), dx3_aux.ld, 1.0, _ptr(dy.t), dy.ld, e.stream)
            dy = blk.bwd(tape, dy)
        a, p = tape.pop("pool")
        da = e.new(B, a.H, a.W, 64)
        assert dy.flat_ok() and dy.ld == dy.cp
        L.call("csbsr_maxpool3x3s2_bwd_split", _ptr(a.t), a.ld, a.lo, _ptr(p.t), p.ld, p.lo, _ptr(dy.t), _ptr(da.t), B, a.H, a.W, 64, e.stream)
        return self.stem.bwd(tape, da, need_dx=need_dxin)
