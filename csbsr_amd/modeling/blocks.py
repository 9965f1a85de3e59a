"""What the networks share: the conv + BatchNorm unit of both detectors, the epilogue backward of a fused conv, and the backward of an
SFT layer (KBPN's SFTlayer, PSPNet_BlurSkip's SFTLikeBlock).

No unit keeps an activation on itself.  What a backward needs goes onto a *tape*: a plain dict the network's ``forward`` creates, keyed
by the unit that wrote the entry.  It becomes the network's ``saved`` and travels with it (the train step's autograd node carries it:
build_model.py, ``psp_saved``).  ``tape=None`` -- eval, ``no_grad``, a frozen trunk -- writes nothing, and a backward pops its entry, so
activations die layer by layer.
"""
import torch

from .. import _lib as L
from ..engine import Conv, BatchNorm, grad_acc


class ConvBN:
    """conv (+bias) -> BatchNorm (batch statistics from the conv epilogue in training, running statistics otherwise) -> optional residual
    add -> none / ReLU / PReLU (``prelu``: the slope parameter) -> optional fused Dropout2d channel mask -> optional ``out=`` slice."""

    def __init__(self, eng, P, conv, norm, k, stride=1, pad=None, dil=1, bias=False, act=L.ACT_RELU, prelu=None):
        self.conv = Conv(eng, conv, P, k, stride, (k - 1) // 2 if pad is None else pad, dil, bias=bias, act=L.ACT_NONE)
        self.bn = BatchNorm(eng, norm, P, self.conv.cout)
        self.act, self.prelu = act, prelu

    def conv_stats(self, x, training):
        """the conv and its BatchNorm statistics: (raw, mean, invstd)"""
        if not training:                # eval: running statistics (F.batch_norm(training=False))
            return self.conv.fwd(x), self.bn.rmean, torch.rsqrt(self.bn.rvar + 1e-5)
        stat = self.bn.new_stat()
        raw = self.conv.fwd(x, stat=stat, stat_mode=L.STAT_BN)
        return (raw,) + self.bn.finalize(stat, raw.npix)

    def fwd(self, x, training, tape=None, res=None, out=None, drop=None, pre=None):
        """``pre``: the result of ``conv_stats`` where the caller ran it earlier (or computed the conv another way)"""
        raw, m, iv = pre or self.conv_stats(x, training)
        y = self.bn.apply(raw, m, iv, act=self.act, prelu=self.prelu, res=res, drop=drop, out=out)
        if tape is not None:
            tape[self] = (x, raw, m, iv, res, drop)
        return y

    # the backward comes in two halves, so that a caller can place other launches between them (a ResNet block's downsample chain)
    def bwd_bn(self, tape, dy, dres=None, dres_acc=False):
        """BatchNorm backward and the weight gradient; returns what ``bwd_dx`` takes: (draw, the input's (H, W))"""
        x, raw, m, iv, res, drop = tape.pop(self)
        draw = self.bn.backward(dy, raw, m, iv, act=self.act, prelu=self.prelu, res=res, drop=drop, dres=dres, dres_acc=dres_acc,
                                dprelu=None if self.prelu is None else grad_acc(self.prelu))
        self.conv.bwd_weights(draw, x)
        if self.conv.b is not None:
            grad_acc(self.conv.b)          # a conv bias feeding train-mode BN has an identically zero gradient (not None)
        x0 = x[0] if isinstance(x, (tuple, list)) else x
        return draw, (x0.H, x0.W)

    def bwd_dx(self, g, out=None, acc=False):
        return self.conv.bwd_input(g[0], out=out, accumulate=acc, in_hw=g[1])

    def bwd(self, tape, dy, dres=None, dres_acc=False, dx_out=None, dx_acc=False, need_dx=True):
        g = self.bwd_bn(tape, dy, dres, dres_acc)
        return self.bwd_dx(g, dx_out, dx_acc) if need_dx else None


def act_bwd(conv, dout, out=None, dpre=None, **res):
    """dOut -> dPre for the fused epilogue of ``conv`` (in place unless ``dpre`` is given); accumulates the bias / PReLU-slope gradients
    unless the layer is frozen.  ``res``: the residual arguments of Engine.epilogue_bwd.  ``out=None``: ``dout`` already is dPre (a head
    whose activation derivative was taken elsewhere) and only the bias gradient is summed."""
    fz = getattr(conv, "frozen", False)
    if out is not None:
        res.update(out=out, act=conv.act, slope=conv.slope, prelu=conv.prelu, dpre=dout if dpre is None else dpre)
    conv.eng.epilogue_bwd(dout, dbias=None if (conv.b is None or fz) else grad_acc(conv.b),
                          dprelu=None if (conv.prelu is None or fz) else grad_acc(conv.prelu), creal=conv.cout, **res)
    return dout if dpre is None else dpre


def sft_bwd(sc0, sc1, sh0, sh1, saves, x, dout, mtap, dx=None, dx_acc=False):
    """Backward of  out = x * sigmoid-branch(x, code) + shift-branch(x, code),  each branch conv1(act(conv0(cat(x, code)))) with the
    spatially constant code folded into conv0 (Conv.fwd_folded).  ``saves`` = (t1, fold1, sc, t2, fold2, out) of the forward; ``dout`` is
    consumed.  The gradient wrt ``x`` goes to ``dx`` (None: not wanted); returns the two branches' gradients wrt the code, [B, c_code]."""
    e = sh1.eng
    t1, fold1, sc, t2, fold2, out = saves
    dsc = e.new(x.N, x.H, x.W, x.c)
    act_bwd(sh1, dout, out, res=x, res2=sc, res_mode=L.RES_FMA, dres=dx, dres_acc=dx_acc, dres2=dsc)
    dcode = []
    for c1, c0, t, dz, fold in ((sh1, sh0, t2, dout, fold2), (sc1, sc0, t1, None, fold1)):
        if dz is None:
            dz = act_bwd(c1, dsc, sc)
        fz = getattr(c0, "frozen", False)
        if not getattr(c1, "frozen", False):
            c1.bwd_weights(dz, t)
        # a learned slope takes the folded form where csbsr_border_class_sums_prelu's precondition holds and the slope is safely > 0
        if c0.prelu is None or (t.H >= 3 and t.W >= 3 and t.H * t.W >= 1024 and e.fold_prelu and e.prelu_fold_ok(c0.prelu)):
            # conv0's activation derivative rides on conv1's dgrad (mask = conv0's saved output, a PReLU slope read on the device); its
            # bias gradient is the sum of the border-class sums the folded weight gradient takes anyway, a slope gradient comes out of
            # the same pass over (dPre, t): no epilogue-backward pass over the C-channel map (8.5 ms each for BlurSkip's 505 at B = 4)
            dt = c1.bwd_input(dz, mask=(t, c0.slope if c0.prelu is None else c0.prelu))
            dcode.append(c0.bwd_weights_folded(dt, x, fold, mtap, frozen=fz, bias_grad=True, prelu_out=t))
        else:
            dt = c1.bwd_input(dz)
            act_bwd(c0, dt, t)
            dcode.append(c0.bwd_weights_folded(dt, x, fold, mtap, frozen=fz))
        if dx is not None:
            c0.bwd_input(dt, seg=0, out=dx, accumulate=True)
        del dt
    return dcode
