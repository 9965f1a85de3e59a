"""Record which library entry points ``csbsr_amd.engine.Conv`` calls, in which order and with which arguments, for a table of layers and
engine modes -- the characterisation fixture of the convolution dispatch (tests/test_conv_dispatch_cpu.py replays it).  No GPU and no
built library: ``_lib.load`` returns a stub whose ``*_eligible`` answers come from a table, ``_lib.call`` is a recorder, the tensors live
on the CPU.

    python tests/golden/make_dispatch_golden.py          # rewrites tests/golden/conv_dispatch_trace.json

Only Conv's public methods and these patch points are used, so the trace does not depend on how the dispatch is written: ``_lib.load``,
``_lib.call``, ``Engine.stream``, ``Engine.workspace`` and, of torch.cuda, ``is_available`` / ``current_stream`` / ``Event`` (dummies).

Per case: the ordered ``_lib.call`` entries (entry point + arguments; a descriptor as the dict of its non-zero fields, segments
expanded; a pointer as null, the name of the case's tensor it points to, ``pack#i`` = the destination of the case's i-th pack call,
else ``ptr``; a ``workspace`` request as a pseudo entry), then ``conv.last_fused``, the sorted keys of ``conv._packed`` and the
``eng.timing`` tuples without their two events.  The stub's queries are not recorded: their number and order are free.
"""
import ctypes as C
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from csbsr_amd import _lib as L  # noqa: E402
from csbsr_amd import engine as E  # noqa: E402
from conv_exact_cases import ROWS  # noqa: E402

PATH = os.path.join(HERE, "conv_dispatch_trace.json")
FAMILIES = ("hr", "x3n", "x3w", "x3", "tp", "thin_dact", "split_fused")
ALL1 = {f: 1 for f in FAMILIES}
KID_FAMILY = {8: "hr", 9: "tp", 10: "x3", 12: "x3", 17: "x3", 18: "x3", 19: "x3w", 20: "x3n"}
ENV_VARS = ("CSBSR_WGRAD_DBG", "CSBSR_CONV_X3", "CSBSR_CONV_X3W", "CSBSR_CONV_X3N", "CSBSR_WGRAD_HR", "CSBSR_CONV_TP", "CSBSR_CONV_GLDS",
            "CSBSR_CONV_HR", "CSBSR_HEAD1", "CSBSR_SPLIT_FUSED", "CSBSR_DC_COMP", "CSBSR_TAPSUM", "CSBSR_WGRAD_MIRROR", "CSBSR_KBUP_FUSED",
            "CSBSR_THIN_DACT", "CSBSR_FOLD_PRELU", "CSBSR_WGRAD_STREAM")
SLOPE = 0.25
STREAM = object()
REAL_LOAD = L.load          # (taken before anything is patched: the environment cases run the real loader against a fake ctypes.CDLL)


class Stub:
    """stands for the loaded library: eligibility from a table, constant sizes"""

    def __init__(self, elig):
        self.elig = dict(elig)
        self.debug = []

    def __getattr__(self, name):
        if name.endswith("_eligible"):
            fam = name[len("csbsr_conv_"):-len("_eligible")]
            return lambda *a: self.elig.get(fam, 0)
        if name.startswith("csbsr_packed_weight_elems"):
            return lambda *a: 64
        if name == "csbsr_wgrad_splits_desc":
            return lambda *a: 4
        if name == "csbsr_thin_tp_backward_slabs":
            return lambda *a: 2
        if name in ("csbsr_debug_last_conv_kernel", "csbsr_debug_last_wgrad_kernel"):
            return lambda: 7
        if name.startswith("csbsr_debug_set_"):
            return lambda v: self.debug.append([name, v])
        raise AttributeError(name)


class Recorder:
    def __init__(self):
        self.calls, self.packs, self.names, self.ranges, self.keep = [], {}, {}, [], []

    def name(self, t, label):
        self.keep.append(t)         # a named tensor lives as long as the case: no later tensor can take its address (and its name)
        self.names[t.data_ptr()] = label
        return t

    def ptr(self, v, wt=False):
        if not v:
            return None
        if v in self.packs:
            return "pack#%d" % self.packs[v]
        if wt:
            return "caller's"
        if v in self.names:
            return self.names[v]
        for base, end, label in self.ranges:
            if base <= v < end:
                return "%s+%d" % (label, v - base)
        return "ptr"

    def struct(self, s):
        out = {}
        for fname, ftype in s._fields_:
            v = getattr(s, fname)
            if ftype is L.vp:
                v = self.ptr(v, wt=fname == "wt")
            elif isinstance(v, C.Array):
                v = [self.struct(e) for e in v]
            if v:
                out[fname] = v
        return out

    def enc(self, a):
        if a is None or isinstance(a, (bool, int, float, str)):
            return int(a) if isinstance(a, bool) else a
        if a is STREAM:
            return "stream"
        if isinstance(a, C.c_void_p):
            return self.ptr(a.value)
        if isinstance(a, C.Structure):
            return self.struct(a)
        if hasattr(a, "_obj"):              # ctypes.byref(descriptor)
            return self.struct(a._obj)
        raise TypeError(f"unexpected argument {a!r}")

    def call(self, name, *args):
        if name.startswith("csbsr_pack_weights"):
            self.packs[args[1].value] = sum(1 for c in self.calls if c[0].startswith("csbsr_pack_weights"))
        self.calls.append([name] + [self.enc(a) for a in args])


class Ctx:
    """one case: a stub, a recorder and a CPU engine"""
    current = None

    def __init__(self, elig, **eng_attrs):
        Ctx.current = self
        self.stub, self.rec = Stub(elig), Recorder()
        self.eng = E.Engine("cpu")
        self.eng.timing = []
        for k, v in eng_attrs.items():
            assert hasattr(self.eng, k), k
            setattr(self.eng, k, v)
        self.ws = self.rec.name(torch.empty(16), "workspace")
        self.conv_ = None

    def fm(self, c, H=8, W=12, N=2, name="x", split=False, bcast=False):
        if bcast:
            f = E.FM(torch.zeros(N, 1, 1, E.pad8(c), dtype=torch.float16), c, bcast=True, H=H, W=W)
        else:
            f = self.eng.new(N, H, W, c, zero=True, split=split)
        self.rec.name(f.t, name)
        return f

    def f32(self, *shape, name):
        return self.rec.name(torch.zeros(*shape), name)

    def conv(self, cin, cout, k, s=1, p=0, tr=False, bias=True, act=L.ACT_NONE, prelu=False, split=None, name="l", cls=E.Conv, **attrs):
        params = {name + ".weight": self.f32(*((cin, cout, k, k) if tr else (cout, cin, k, k)), name=name + ".w"),
                  name + ".bias": self.f32(cout, name=name + ".b"), name + ".a": torch.full((1,), SLOPE)}
        self.rec.name(params[name + ".a"], name + ".a")
        conv = cls(self.eng, name, params, k, s, p, 1, transposed=tr, bias=bias, act=act, slope=SLOPE,
                   prelu=name + ".a" if prelu else False, split=split)
        for key, v in attrs.items():
            assert hasattr(conv, key), key
            setattr(conv, key, v)
        self.track(conv)
        if self.conv_ is None:
            self.conv_ = conv
        self.rec.keep.append(conv)
        return conv

    def track(self, conv):
        for t, label in ((conv.w, ".gacc"), (conv.b, ".b.gacc"), (conv.prelu, ".a.gacc")):
            if t is not None:
                g = E.grad_acc(t)
                self.rec.ranges.append((g.data_ptr(), g.data_ptr() + 4 * g.numel(), conv.name + label))

    def note(self, *entry):
        self.rec.calls.append(list(entry))

    def result(self):
        conv = self.conv_
        timing = [[list(x) if isinstance(x, tuple) else x for i, x in enumerate(t) if i not in (3, 4)] for t in self.eng.timing]
        return {"calls": self.rec.calls, "last_fused": getattr(conv, "last_fused", None),
                "packed": sorted(repr(k) for k in conv._packed), "timing": timing}


class _Event:
    def __init__(self, **kw):
        pass

    def record(self, *a):
        pass

    def query(self):
        return True


class _Stream:
    cuda_stream = 0


def install(mp):
    """the patch points, on a pytest ``monkeypatch`` (or pytest.MonkeyPatch) object"""
    mp.setattr(L, "load", lambda: Ctx.current.stub)
    mp.setattr(L, "call", lambda name, *a: Ctx.current.rec.call(name, *a))
    mp.setattr(E.Engine, "stream", property(lambda self: STREAM))

    def workspace(self, nfloat):
        Ctx.current.note("workspace", int(nfloat))
        return Ctx.current.ws
    mp.setattr(E.Engine, "workspace", workspace)
    mp.setattr(torch.cuda, "is_available", lambda: False)
    mp.setattr(torch.cuda, "current_stream", lambda *a: _Stream())
    mp.setattr(torch.cuda, "Event", _Event)


# ------------------------------------------------------------------------------------------------------------ the cases

ACTS = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "prelu": L.ACT_PRELU, "sigmoid": L.ACT_SIGMOID}
RES = {"add": L.RES_ADD, "sub": L.RES_SUB, "fma": L.RES_FMA}


def run_row(r, elig):
    """a row of tests/conv_exact_cases.py at 2 x 8 x 12 (the stub answers eligibility; the layer and its epilogue are the row's)"""
    c = Ctx(elig, **{n[4:]: v for n, v in r.modes if n.startswith("eng.")})
    N, H, W = 2, 8, 12
    act, _, res = r.epi.partition("_")
    fwdlike = r.op in ("fwd", "classbias")
    has_bias = fwdlike and r.kid not in (8, 13, 15, 16) and r.epi not in ("bn", "sum")
    a = ACTS.get(act, L.ACT_NONE) if fwdlike else L.ACT_NONE
    cin = sum(r.segs) if r.op == "classbias" else r.cin
    conv = c.conv(cin, r.cout, r.k, r.s, r.p, r.tr, bias=has_bias, act=a, prelu=a == L.ACT_PRELU, split=r.segs or None)
    OH, OW = conv.out_size(H, W)

    def inputs():
        if r.segs and r.op != "classbias":
            return tuple(c.fm(n, H, W, N, name="x%d" % i) for i, n in enumerate(r.segs))
        return c.fm(r.cin, H, W, N)
    if r.op == "wgrad":
        conv.bwd_weights(c.fm(r.cout, OH, OW, N, name="dpre"), inputs())
    elif r.op == "dgrad":
        conv.bwd_input(c.fm(r.cout, OH, OW, N, name="dpre"), out=c.fm(r.cin, H, W, N, name="dx"), accumulate="acc" in r.epi, in_hw=(H, W),
                       mask=(c.fm(r.cin, H, W, N, name="below"), SLOPE) if "mask" in r.epi else None)
    elif r.op == "classbias":
        mode = dict(r.modes).get("arg.cb_mode", 0)
        conv.fwd_classbias(inputs(), c.f32(N, 16 if mode == 0 else 25, E.pad8(r.cout), name="cb"), mode, out=c.fm(r.cout, OH, OW, N, name="y"))
    else:
        kw = {}
        if res:
            kw = dict(res=c.fm(r.cout, OH, OW, N, name="r1"), res_mode=RES[res])
            if res == "fma":
                kw["res2"] = c.fm(r.cout, OH, OW, N, name="r2")
        if r.epi in ("bn", "sum"):
            kw.update(stat=c.f32(*((2, E.pad8(r.cout)) if r.epi == "bn" else (N, E.pad8(r.cout))), name="stat"),
                      stat_mode=L.STAT_BN if r.epi == "bn" else L.STAT_SAMPLE_SUM)
        if r.epi == "sum":
            conv.fwd(inputs(), store=False, **kw)
        else:
            conv.fwd(inputs(), out=c.fm(r.cout, OH, OW, N, name="y"), **kw)
    return c


def fwd3x3(elig, cin=128, cout=128, conv_attrs=None, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(cin, cout, 3, 1, 1, act=L.ACT_LRELU, **(conv_attrs or {}))
    conv.fwd(c.fm(cin))
    conv.fwd(c.fm(cin))             # packs cached
    conv.bwd_input(c.fm(cout, name="dpre"))
    return c


def split_fwd(elig, blocks, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(64, 64, 3, 1, 1, act=L.ACT_RELU, fwd_blocks=blocks)
    conv.fwd(c.fm(64, split=True))
    conv.fwd(c.fm(64, split=True), stat=c.f32(2, 64, name="stat"), stat_mode=L.STAT_BN)
    thin = c.conv(16, 24, 3, 1, 1, name="thin", fwd_blocks=blocks)      # below the fused form's 32-channel threshold
    thin.fwd(c.fm(16, split=True, name="xt"))
    return c


def dc_case(elig, split=False, blocks=3, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(32, 32, 3, 1, 1, act=L.ACT_PRELU, prelu=True, dc_comp=True, fwd_blocks=blocks)
    conv.fwd(c.fm(32, 16, 16, split=split))
    conv.fwd(c.fm(32, 8, 12, split=split, name="x_small"))          # (OH * OW) % 256 != 0: the layer's own bias
    two = c.conv(48, 32, 3, 1, 1, split=(32, 16), name="two", dc_comp=True)
    two.fwd((c.fm(32, 16, 16, name="x0"), c.fm(16, 16, 16, name="code", bcast=True)))
    two.bwd_input(c.fm(32, 16, 16, name="dpre"), seg=0)
    two.bwd_weights(c.fm(32, 16, 16, name="dpre"), (c.fm(32, 16, 16, name="x0"), c.fm(16, 16, 16, name="code", bcast=True)))
    return c


MTAP = torch.tensor([[1., 1., 1.], [0., 1., 1.], [1., 1., 0.], [0., 1., 0.]])


def folded(elig, split=False, blocks=3, HW=(8, 12), dc=False, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(80, 64, 3, 1, 1, act=L.ACT_PRELU, prelu=True, split=(64, 16), fwd_blocks=blocks, dc_comp=dc)
    x = c.fm(64, *HW, split=split)
    out, saved = conv.fwd_folded(x, torch.ones(2, 16), MTAP)
    dpre = c.fm(64, *HW, name="dpre")
    conv.bwd_weights_folded(dpre, E.FM(x.t, x.c, H=x.H, W=x.W), saved, MTAP, bias_grad=True, prelu_out=out if not split else None)
    conv.bwd_weights_folded(dpre, E.FM(x.t, x.c, H=x.H, W=x.W), saved, MTAP, frozen=True)
    conv.bwd_input(dpre, seg=0, mask=(c.fm(64, *HW, name="below"), conv.prelu))
    return c


def const_1x1(elig, split=False, blocks=3, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(80, 64, 1, split=(16, 64), act=L.ACT_LRELU, fwd_blocks=blocks)
    conv.fwd_const_1x1(torch.ones(2, 16), c.fm(64, split=split))
    conv.fwd_const_1x1(torch.ones(2, 16), c.fm(64, split=split), stat=c.f32(2, 64, name="stat"), stat_mode=L.STAT_BN)
    return c


def classbias(elig, k, mode, prelu, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(48, 32, k, 1, k // 2, act=L.ACT_PRELU if prelu else L.ACT_LRELU, prelu=prelu, split=(32, 16))
    conv.fwd_classbias(c.fm(32), c.f32(2, 16 if mode == 0 else 25, 32, name="cb"), mode)
    return c


def dact(elig, dres, below_prelu=True, fold_ok=True, frozen=False, thin3x3=False, **eng):
    """the dgrad that may take over the epilogue-backward pass of the layer below"""
    c = Ctx(elig, **eng)
    c.eng.prelu_fold_ok = lambda p: fold_ok
    if thin3x3:             # a stride-1 3x3 layer: its dgrad has no transposed-form kernel
        conv = c.conv(128, 3, 3, 1, 1)
        H, W, OH, OW = 8, 12, 8, 12
    else:                   # 8x8 stride-4 conv: its dgrad is the 2x2-tap transposed form
        conv = c.conv(128, 128, 8, 4, 2)
        H, W, OH, OW = 8, 12, 2, 3
    below = c.conv(128, 128, 3, 1, 1, act=L.ACT_PRELU if below_prelu else L.ACT_LRELU, prelu=below_prelu, name="below")
    if frozen:
        below.frozen = True
    kw = {}
    if dres:
        kw["dres"] = (c.fm(128, H, W, name="rfm"), c.fm(128, H, W, name="dfm"), L.RES_ADD)
    conv.bwd_input(c.fm(conv.cout, OH, OW, name="dpre"), out=c.fm(128, H, W, name="dx"), in_hw=(H, W),
                   dact=(below, c.fm(128, H, W, name="saved")), **kw)
    c.note("last_fused", bool(conv.last_fused))
    conv.bwd_input(c.fm(conv.cout, OH, OW, name="dpre"), out=c.fm(128, H, W, name="dx"), in_hw=(H, W), accumulate=True)
    return c


def head1(elig, split=False, act=L.ACT_SIGMOID, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(64, 1, 1, act=act)
    conv.fwd(c.fm(64, split=split), out32=c.f32(2, 1, 8, 12, name="y32"))
    conv.bwd_input(c.fm(1, name="dpre"))
    conv.bwd_input(c.fm(1, name="dpre"), accumulate=True, out=c.fm(64, name="dx"))        # not the streaming form
    conv.fwd(c.fm(64), res=c.fm(1, name="r1"), res_mode=L.RES_ADD)                         # a head with a residual: the general path
    odd = c.conv(48, 1, 1, name="odd")                                                     # 48 channels: not a head1 width
    odd.fwd(c.fm(48, name="x48"), out32=c.f32(2, 1, 8, 12, name="y32"))
    return c


def hp_dgrad(elig, s, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(64, 64, 3, s, 1, hp_dgrad=True)
    OH, OW = conv.out_size(8, 12)
    conv.bwd_input(c.fm(64, OH, OW, name="dpre"), in_hw=(8, 12))
    conv.bwd_input(c.fm(64, OH, OW, name="dpre"), in_hw=(8, 12), stat=c.f32(2, 64, name="stat"))
    conv.bwd_input(c.fm(64, OH, OW, name="dpre", bcast=True), in_hw=(8, 12))              # a broadcast gradient: plain weights
    return c


def shuffle(elig, **eng):
    c = Ctx(elig, **eng)
    conv = E.ShuffleConv(c.eng, "ps", {"ps.weight": c.f32(64 * 4, 64, 3, 3, name="ps.master"), "ps.a": torch.full((1,), SLOPE)}, 2,
                         act=L.ACT_PRELU, prelu="ps.a")
    c.conv_ = conv
    c.rec.name(conv.w, "ps.w")
    c.track(conv)
    x = c.fm(64)
    y = conv.fwd(x)
    dpre = c.fm(64, y.H, y.W, name="dpre")
    conv.bwd_input(dpre, in_hw=(8, 12))
    conv.bwd_weights(dpre, x)
    return c


def thin_tp(elig, W=12, frozen=False, **eng):
    c = Ctx(elig, **eng)
    conv = c.conv(3, 64, 8, 4, 2, tr=True, bias=False, act=L.ACT_PRELU, prelu=True)
    x = c.fm(3, 8, W)
    c.note("thin_tp_fused_ok", bool(conv.thin_tp_fused_ok(x)))
    OH, OW = conv.out_size(8, W)
    conv.bwd_thin_tp_fused(c.fm(64, OH, OW, name="dout"), x, c.fm(64, OH, OW, name="dpre"), frozen=frozen)
    conv.bwd_weights(c.fm(64, OH, OW, name="dpre"), x)
    return c


def strided_pair(elig, **eng):
    """8x8 stride-4 conv and transposed conv: forward and dgrad of each"""
    c = Ctx(elig, **eng)
    down = c.conv(128, 128, 8, 4, 2, act=L.ACT_LRELU)
    up = c.conv(128, 128, 8, 4, 2, tr=True, act=L.ACT_PRELU, prelu=True, name="up")
    y = down.fwd(c.fm(128, 8, 12))
    down.bwd_input(c.fm(128, y.H, y.W, name="dpre"), in_hw=(8, 12))
    down.bwd_input(c.fm(128, y.H, y.W, name="dpre"), in_hw=(8, 12), stat=c.f32(2, 128, name="stat"))
    z = up.fwd(c.fm(128, 2, 3, name="xs"), res=c.fm(128, 8, 12, name="r1"), res_mode=L.RES_ADD)
    up.bwd_input(c.fm(128, z.H, z.W, name="dz"))
    up.bwd_weights(c.fm(128, z.H, z.W, name="dz"), c.fm(128, 2, 3, name="xs"))
    return c


def basket(elig, **eng):
    """one launch of every kind against one engine setting"""
    c = fwd3x3(elig, conv_attrs=dict(winograd=True), **eng)
    thin = c.conv(32, 32, 3, 1, 1, name="hr32")
    thin.fwd(c.fm(32))
    thin.fwd(c.fm(32), stat=c.f32(2, 32, name="sum"), stat_mode=L.STAT_SAMPLE_SUM, store=False)
    thin.bwd_input(c.fm(32, name="d32"), mask=(c.fm(32, name="below"), SLOPE))
    one = c.conv(32, 48, 1, name="1x1", act=L.ACT_PRELU, prelu=True)
    one.fwd(c.fm(32))
    two = c.conv(256, 3, 3, 1, 1, split=(128, 128), name="two")
    two.fwd((c.fm(128, name="x0"), c.fm(128, name="x1")))
    two.bwd_input(c.fm(3, name="d3"), seg=1)
    two.bwd_weights(c.fm(3, name="d3"), (c.fm(128, name="x0"), c.fm(128, name="x1")))
    return c


def all_cases():
    """(name, thunk returning the finished Ctx)"""
    out = []

    def add(name, fn, *a, **kw):
        out.append((name, lambda: fn(*a, **kw)))
    for r in ROWS:
        fam = KID_FAMILY.get(r.kid) if r.op != "wgrad" else None
        for tag, elig in (("none", {}), ("own", {fam: 1} if fam else {}), ("all", ALL1)):
            add(f"row/{r.name}/{tag}", run_row, r, elig)
    # tie-breaks
    add("tie/x3n2_hr1", fwd3x3, {"x3n": 2, "hr": 1})
    add("tie/x3n1_hr1", fwd3x3, {"x3n": 1, "hr": 1})
    add("tie/x3n1_hr0", fwd3x3, {"x3n": 1})
    for wino in (False, True):
        for mode in (0, 1, 2):
            add(f"tie/x3w_winograd{int(wino)}_use{mode}", fwd3x3, {"x3w": 1, "x3": 1}, conv_attrs=dict(winograd=wino), use_x3w=mode)
    # split inputs
    for blocks in (1, 2, 3):
        for sf in (1, 0):
            add(f"split/blocks{blocks}_fused{sf}", split_fwd, {"split_fused": sf}, blocks)
            add(f"split/blocks{blocks}_fused{sf}_all", split_fwd, dict(ALL1, split_fused=sf), blocks)
        add(f"split/blocks{blocks}_engine_off", split_fwd, ALL1, blocks, split_fused=False)
    # rounding compensation (16 x 16: the pixel-count gate of Conv._dc_bias)
    for tag, kw in (("plain", {}), ("nearest", dict(tapsum=False)), ("off", dict(dc_comp=False)), ("split3", dict(split=True)),
                    ("split2", dict(split=True, blocks=2)), ("split1", dict(split=True, blocks=1))):
        add(f"dc/{tag}", dc_case, {}, **kw)
        add(f"dc/{tag}_all", dc_case, ALL1, **kw)
    # folded / constant / class-bias forms
    for tag, elig in (("none", {}), ("all", ALL1), ("x3n", {"x3n": 1}), ("x3", {"x3": 1}), ("hr", {"hr": 1})):
        add(f"folded/plain_{tag}", folded, elig)
        for blocks in (1, 2, 3):
            add(f"folded/split{blocks}_{tag}", folded, elig, split=True, blocks=blocks)
        add(f"folded/dc_{tag}", folded, elig, HW=(16, 16), dc=True)
        add(f"const1x1/plain_{tag}", const_1x1, elig)
        for blocks in (1, 2, 3):
            add(f"const1x1/split{blocks}_{tag}", const_1x1, elig, split=True, blocks=blocks)
        for k in (1, 3):
            for mode in (0, 1):
                for pre in (False, True):
                    add(f"classbias/k{k}_mode{mode}_prelu{int(pre)}_{tag}", classbias, elig, k, mode, pre)
    # the dgrad that takes over the epilogue-backward pass below it
    for dres in (False, True):
        d = "_dres" if dres else ""
        add(f"dact/tp{d}", dact, {"tp": 1}, dres)
        add(f"dact/tp_engine_off{d}", dact, {"tp": 1}, dres, use_tp=False)
        add(f"dact/thin{d}", dact, {"thin_dact": 1}, dres, thin_dact=True)
        add(f"dact/thin_flag_off{d}", dact, {"thin_dact": 1}, dres)
        add(f"dact/thin_slope_low{d}", dact, {"thin_dact": 1}, dres, fold_ok=False, thin_dact=True)
        add(f"dact/thin_no_prelu{d}", dact, {"thin_dact": 1}, dres, below_prelu=False, fold_ok=False, thin_dact=True)
        add(f"dact/thin_3x3{d}", dact, {"thin_dact": 1, "x3": 1, "x3n": 1, "hr": 1}, dres, thin3x3=True, thin_dact=True)
        add(f"dact/both{d}", dact, {"tp": 1, "thin_dact": 1}, dres, thin_dact=True)
        add(f"dact/neither{d}", dact, {}, dres, thin_dact=True)
        add(f"dact/all{d}", dact, ALL1, dres, thin_dact=True)
        add(f"dact/frozen{d}", dact, {"tp": 1}, dres, frozen=True)
    # 1-channel heads
    for on in (True, False):
        add(f"head1/use{int(on)}", head1, {}, use_head1=on)
        add(f"head1/use{int(on)}_split", head1, ALL1, split=True, use_head1=on)
    add("head1/relu", head1, {}, act=L.ACT_RELU)
    for s in (1, 2):
        add(f"hp_dgrad/s{s}", hp_dgrad, {}, s)
        add(f"hp_dgrad/s{s}_all", hp_dgrad, ALL1, s)
    add("shuffle/none", shuffle, {})
    add("shuffle/all", shuffle, ALL1)
    add("thin_tp/fused", thin_tp, {})
    add("thin_tp/frozen", thin_tp, {}, frozen=True)
    add("thin_tp/wide", thin_tp, {}, W=1028)
    add("thin_tp/flag_off", thin_tp, {}, thin_tp_fused=False)
    for tag, elig in (("none", {}), ("all", ALL1), ("tp", {"tp": 1}), ("x3", {"x3": 1})):
        add(f"strided/{tag}", strided_pair, elig)
    # every engine flag off once against the all-1 table
    add("flags/default", basket, ALL1)
    add("flags/none", basket, {})
    for flag, v in (("use_hr", False), ("use_x3n", False), ("use_x3w", 1), ("use_x3w", 2), ("use_x3", False), ("use_tp", False),
                    ("use_head1", False), ("split_fused", False), ("dc_comp", False), ("tapsum", False), ("wgrad_mirror", False),
                    ("thin_tp_fused", False), ("thin_dact", True)):
        add(f"flags/{flag}={int(v)}", basket, ALL1, **{flag: v})
        add(f"flags/{flag}={int(v)}/strided", strided_pair, ALL1, **{flag: v})
    return out


# ------------------------------------------------------------------------------------------------------------ the environment

class _FakeCDLL:
    """what ctypes.CDLL returns while ``_lib.load`` itself runs: every declared symbol, the debug setters recorded"""

    def __init__(self, path):
        self.debug = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def fn(*a):
            if name.startswith("csbsr_debug_set_"):
                self.debug.append([name] + list(a))
            return 0
        self.__dict__[name] = fn
        return fn


def env_case(mp, var, value):
    """Engine attributes and library debug calls with ``var`` = ``value`` (None: unset) and every other hook unset"""
    with mp.context() as m:
        for v in ENV_VARS:
            m.delenv(v, raising=False)
        if value is not None:
            m.setenv(var, value)
        m.setattr(L, "_lib", None)
        m.setattr(L, "LIB_PATH", os.path.abspath(__file__))
        m.setattr(L.C, "CDLL", _FakeCDLL)
        lib = REAL_LOAD()
        m.setattr(L, "load", lambda: lib)
        m.setattr(L, "call", lambda *a: None)
        m.setattr(torch.cuda, "is_available", lambda: False)
        eng = E.Engine("cpu")
        attrs = {k: v for k, v in sorted(vars(eng).items())
                 if (not k.startswith("_") or k == "_wg_on") and isinstance(v, (bool, int, float, str, type(None)))}
        return {"debug": lib.debug, "engine": attrs}


def env_cases(mp):
    out = {}
    for var in ENV_VARS:
        for value in (None, "0", "1", "2") + (("all",) if var == "CSBSR_CONV_X3W" else ()):
            out["%s=%s" % (var, "unset" if value is None else value)] = env_case(mp, var, value)
    return out


def env_vars_in_sources():
    """the CSBSR_* names csbsr_amd/_lib.py and csbsr_amd/engine.py mention as string literals (CSBSR_LIB, a path, aside)"""
    found = set()
    for name in ("_lib.py", "engine.py"):
        with open(os.path.join(ROOT, "csbsr_amd", name)) as f:
            found |= set(re.findall(r"[\"'](CSBSR_[A-Z0-9_]+)[\"']", f.read()))
    return found - {"CSBSR_LIB"}


def _intern(table, index, obj):
    key = json.dumps(obj)
    if key not in index:
        index[key] = len(table)
        table.append(obj)
    return index[key]


def _wrap(name, items, last=False, width=240):
    """``"name": [items...]`` with as many items per line as fit"""
    lines, cur = [], ""
    for i, it in enumerate(items):
        piece = json.dumps(it, separators=(",", ":")) + ("," if i + 1 < len(items) else "")
        if cur and len(cur) + len(piece) > width:
            lines.append(cur)
            cur = ""
        cur += piece
    return [' "%s": [' % name] + ["  " + ln for ln in lines + ([cur] if cur else [])] + [" ]" + ("" if last else ",")]


def dumps(doc):
    """the document as compact JSON: every distinct descriptor, call, timing tuple and case body is written once and referred to by
    its index (descriptor: ``{"$": i}`` among a call's arguments, itself written as ``{"=": j, "-": [fields it lacks], fields that differ}``
    from an earlier descriptor j where that is shorter; body: [call indices, last_fused, packed keys, timing indices]); the
    environment settings as the Engine attributes with everything unset plus, per setting, [library debug calls, attributes that differ]"""
    tables = {k: ([], {}) for k in ("descs", "calls", "timing", "bodies")}
    cases = {}
    for name, case in doc["cases"].items():
        calls = [_intern(*tables["calls"], [{"$": _intern(*tables["descs"], a)} if isinstance(a, dict) else a for a in c]) for c in case["calls"]]
        cases[name] = _intern(*tables["bodies"], [calls, case["last_fused"], case["packed"], [_intern(*tables["timing"], t) for t in case["timing"]]])
    base = next(v for k, v in doc["env"].items() if k.endswith("=unset"))["engine"]
    env = [[k, v["debug"], {a: x for a, x in v["engine"].items() if base[a] != x}] for k, v in doc["env"].items()]
    assert all(set(v["engine"]) == set(base) for v in doc["env"].values())
    descs = tables["descs"][0]
    for i in range(len(descs) - 1, 0, -1):          # a descriptor as its difference from the most similar earlier one
        size = lambda j: sum(descs[j].get(k) != v for k, v in descs[i].items()) + sum(k not in descs[i] for k in descs[j])
        j = min(range(i), key=size)
        if size(j) < len(descs[i]) - 2:
            descs[i] = dict({"=": j, "-": [k for k in descs[j] if k not in descs[i]]}, **{k: v for k, v in descs[i].items() if descs[j].get(k) != v})
    lines = ["{"]
    for k in ("descs", "calls", "timing", "bodies"):
        lines += _wrap(k, tables[k][0])
    lines += _wrap("cases", [[n, i] for n, i in cases.items()])
    lines += [' "env_unset": %s,' % json.dumps(base)] + _wrap("env", env, last=True) + ["}"]
    return "\n".join(lines) + "\n"


def loads(text):
    """the document ``dumps`` wrote, expanded again"""
    z = json.loads(text)
    for i, d in enumerate(z["descs"]):
        if "=" in d:
            z["descs"][i] = dict({k: v for k, v in z["descs"][d["="]].items() if k not in d["-"]}, **{k: v for k, v in d.items() if k not in "=-"})
    calls = [[z["descs"][a["$"]] if isinstance(a, dict) else a for a in c] for c in z["calls"]]
    cases = {}
    for name, i in z["cases"]:
        ci, fused, packed, ti = z["bodies"][i]
        cases[name] = {"calls": [calls[c] for c in ci], "last_fused": fused, "packed": packed, "timing": [z["timing"][t] for t in ti]}
    return {"cases": cases, "env": {k: {"debug": dbg, "engine": dict(z["env_unset"], **diff)} for k, dbg, diff in z["env"]}}


def record(mp):
    """the whole document, under the patches of ``install``"""
    with mp.context() as m:
        install(m)
        cases = {name: thunk().result() for name, thunk in all_cases()}
    return {"cases": cases, "env": env_cases(mp)}


def main():
    import pytest
    doc = record(pytest.MonkeyPatch())
    text = dumps(doc)
    assert loads(text) == json.loads(json.dumps(doc))
    with open(PATH, "w") as f:
        f.write(text)
    assert os.path.getsize(PATH) < 1 << 20
    ncalls = sum(len(c["calls"]) for c in doc["cases"].values())
    print("wrote", PATH, os.path.getsize(PATH), "bytes;", len(doc["cases"]), "cases,", ncalls, "calls,", len(doc["env"]), "environment settings")


if __name__ == "__main__":
    main()
