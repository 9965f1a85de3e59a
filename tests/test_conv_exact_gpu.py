"""Bit-exact parity of every convolution kernel and dispatch path on exact-lattice operands.

Each row of tests/conv_exact_cases.py is run through the engine (Conv.fwd / bwd_input / bwd_weights) on integer-times-power-of-two
operands whose exact result every kernel can represent (tests/exact_lattice.py proves the bounds on the reference).  There is no
legitimate rounding left, so the kernel's output must EQUAL the CPU reference -- fp32 where the lattice bound makes any summation order
exact.  Per row:
  * the kernel ID (and template instance) it must reach, asserted after the launch;
  * operand bounds: the input as a channel slice of a wider buffer whose other channels are NaN; the output as a channel slice at c0 = 0
    and at c0 = 128 of a wider buffer, the rest of it (and one guard row below every sample) filled with a canary bit pattern that must
    survive, the slice itself prefilled with NaN (so an output element the kernel never writes shows) and its pad channels
    [cout, coutp) exactly zero afterwards (conv_common.h: the epilogue zeroes the pad lanes);
  * wgrad: the slab workspace filled with NaN before every launch, so an unwritten slab or split shows;
  * launches with partial rows (BatchNorm sums, per-sample sums): the reduction scratch refilled with NaN first;
  * the persistent-grid families (conv_x3 / x3n / x3w / tp / hr): again on a stream with a CU budget of 1, 3 and 7 CUs (8 and 16 for
    conv_hr), so every workgroup walks many tiles with a ragged tail -- bit-identical to the run without a budget.
Debug modes are restored to the library's defaults (conv_exact_cases.DEFAULT_MODES) and budgets cleared in ``finally``."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import exact_lattice as XL
from conv_exact_cases import BUDGETS, DEFAULT_MODES, ROWS

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A          # int16 bit pattern of the guard elements (fp16 203.25)
SLOPE = 0.25             # LReLU / PReLU / mask slope: a power of two
QX, QW = 2, 3            # activations i / 4, weights j / 8: every product on the 2^-5 lattice
QB = 5                   # bias, residual, old gradient: k / 32
ACTS = ("none", "relu", "lrelu", "prelu", "sigmoid")


def _L():
    from csbsr_amd import _lib as L
    return L


def pad8(c):
    return (c + 7) // 8 * 8


def _nhwc(x):
    N, c, H, W = x.shape
    t = torch.zeros(N, H, W, pad8(c), dtype=torch.float16)
    t[..., :c] = x.permute(0, 2, 3, 1).half()
    return t


def _fm(x, c0=None):
    """NCHW fp32 (fp16-exact) -> FM on the GPU; c0: as channels [c0, c0 + cp) of a wider buffer whose other channels are NaN"""
    from csbsr_amd.engine import FM
    t = _nhwc(x)
    if c0 is not None:
        N, H, W, cp = t.shape
        big = torch.full((N, H, W, c0 + cp + 64), float("nan"), dtype=torch.float16)
        big[..., c0:c0 + cp] = t
        return FM(big.cuda()[..., c0:c0 + cp], x.shape[1])
    return FM(t.cuda(), x.shape[1])


def _from_fm(fm):
    return fm.t[..., :fm.c].float().cpu().permute(0, 3, 1, 2)


class Guarded:
    """an output FM as channels [c0, c0 + coutp) of a wider buffer with a guard row below every sample; everything outside the slice
    holds CANARY, the slice holds ``old`` (accumulating launches) or NaN"""

    def __init__(self, N, OH, OW, c, c0, old=None):
        from csbsr_amd.engine import FM
        cp = pad8(c)
        self.big = torch.empty(N, OH + 1, OW, c0 + cp + 64, dtype=torch.float16, device="cuda")
        self.big.view(torch.int16).fill_(CANARY)
        v = self.big[:, :OH, :, c0:c0 + cp]
        if old is None:
            v.fill_(float("nan"))
        else:
            v.copy_(_nhwc(old).cuda())
        self.fm = FM(v, c)
        self.region = torch.zeros(self.big.shape, dtype=torch.bool)
        self.region[:, :OH, :, c0:c0 + cp] = True
        self.c, self.cp = c, cp

    def check(self, what):
        g = self.big.view(torch.int16).cpu()
        bad = (g != CANARY) & ~self.region
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} guard elements overwritten, first at {tuple(torch.nonzero(bad)[0].tolist())}"
        pads = self.fm.t[..., self.c:].float().cpu()
        assert bool((pads == 0).all()), f"{what}: pad channels [{self.c}, {self.cp}) not zero: {XL.mismatch(pads, torch.zeros_like(pads))}"


def _act(t, act):
    if act == "none":
        return t
    if act == "relu":
        return torch.relu(t)
    if act == "sigmoid":
        return torch.sigmoid(t.double())
    return torch.where(t > 0, t, t * SLOPE)


def _poison_scratch():
    from csbsr_amd import engine
    for buf in engine._RED_SCRATCH.values():
        buf.fill_(float("nan"))


def _apply_modes(lib, eng, modes):
    for name, v in modes:
        if name.startswith("arg."):          # (an argument of the launch, not a mode)
            continue
        if name.startswith("eng."):
            setattr(eng, name[4:], v)
        else:
            getattr(lib, "csbsr_debug_set_" + name)(v)


def _restore_modes(lib):
    for name, v in DEFAULT_MODES.items():
        getattr(lib, "csbsr_debug_set_" + name)(v)


def _kernel_id(lib, op):
    return int(lib.csbsr_debug_last_wgrad_kernel() if op == "wgrad" else lib.csbsr_debug_last_conv_kernel())


def _fp16_ulp(t):
    """the spacing of fp16 at |t| (subnormal spacing below 2^-14)"""
    e = torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def _class_index(OH, OW, cb_mode):
    """position class of every output pixel (conv_common.h conv_class_bias_row): 16 border classes or 25 two-ring classes"""
    oy, ox = torch.arange(OH)[:, None], torch.arange(OW)[None, :]
    if cb_mode == 0:
        return (oy == 0) * 8 + (oy == OH - 1) * 4 + (ox == 0) * 2 + (ox == OW - 1)
    ty = torch.where(oy < 2, oy, torch.where(oy >= OH - 2, oy - OH + 5, torch.full_like(oy, 2)))
    tx = torch.where(ox < 2, ox, torch.where(ox >= OW - 2, ox - OW + 5, torch.full_like(ox, 2)))
    return ty * 5 + tx


def _check_kid(row, kid, what):
    if row.op == "wgrad":
        assert kid == row.kid, f"{row.name} {what}: reached wgrad kernel {kid}, the table says {row.kid} ({row.why})"
    else:
        assert (kid & 255, kid >> 8 if row.var is not None else None) == (row.kid, row.var), \
            f"{row.name} {what}: reached conv kernel {kid & 255} instance {kid >> 8}, the table says {row.kid} / {row.var} ({row.why})"


class Budget:
    """a side stream with a CU budget (csbsr_debug_stream_set_cu_budget); the budget is cleared on exit"""

    def __init__(self, ncu):
        self.ncu, self.s = ncu, torch.cuda.Stream()

    def __enter__(self):
        L = _L()
        self.h = C.c_void_p(self.s.cuda_stream)
        L.call("csbsr_debug_stream_set_cu_budget", self.h, self.ncu)
        assert L.load().csbsr_debug_stream_cu_budget(self.h) == self.ncu
        self.s.wait_stream(torch.cuda.current_stream())
        self.ctx = torch.cuda.stream(self.s)
        self.ctx.__enter__()
        return self

    def __exit__(self, *exc):
        try:
            self.ctx.__exit__(*exc)
            torch.cuda.current_stream().wait_stream(self.s)
            torch.cuda.synchronize()
        finally:
            _L().call("csbsr_debug_stream_set_cu_budget", self.h, 0)
        return False


# ---------------------------------------------------------------------------------------------------------------- one row

class Case:
    """operands, reference and launcher of one table row"""

    def __init__(self, row):
        self.row = row
        g = torch.Generator().manual_seed(sum(map(ord, row.name)))
        r = row
        taps = ((r.k + r.s - 1) // r.s) ** 2 if r.tr else r.k * r.k
        if r.tr:
            self.OH, self.OW = (r.H - 1) * r.s - 2 * r.p + r.k, (r.W - 1) * r.s - 2 * r.p + r.k
            wshape = (r.cin, r.cout, r.k, r.k)
        else:
            self.OH, self.OW = (r.H + 2 * r.p - r.k) // r.s + 1, (r.W + 2 * r.p - r.k) // r.s + 1
            wshape = (r.cout, r.cin, r.k, r.k)
        conv = (lambda a, w_, b_=None: F.conv_transpose2d(a, w_, b_, r.s, r.p)) if r.tr else (lambda a, w_, b_=None: F.conv2d(a, w_, b_, r.s, r.p))
        self.unit = 2.0 ** -(QX + QW)
        if r.op in ("fwd", "classbias"):
            K = taps * r.cin
            dens = XL.density_for(K)
            self.x = XL.draw((r.N, r.cin, r.H, r.W), QX, amp=2, density=dens, gen=g)
            if r.op == "classbias":         # segment 1 (a map constant per position class) enters as a [N, classes, coutp] table
                wshape = (r.cout, sum(r.segs), r.k, r.k)
                self.cb_mode = dict(r.modes).get("arg.cb_mode", 0)
                ncls = 16 if self.cb_mode == 0 else 25
                self.cb = torch.zeros(r.N, ncls, pad8(r.cout))
                self.cb[..., :r.cout] = XL.draw((r.N, ncls, r.cout), QB, amp=64, density=1.0, gen=g)
            self.w = XL.draw(wshape, QW, amp=2, density=dens, gen=g)
            XL.assert_sum_bound(K, 2.0 ** (1 - QX), 2.0 ** (1 - QW), self.unit, r.name)
            act, _, res = r.epi.partition("_")
            self.act = act if act in ACTS else "none"
            self.res = res
            # (no bias on the kernels that refuse one: conv_hr, the thin streaming kernels)
            self.has_bias = r.kid not in (8, 13, 15, 16) and r.epi not in ("bn", "sum")
            self.b = XL.draw((r.cout,), QB, amp=64, density=1.0, gen=g) if self.has_bias else None
            with torch.no_grad():
                pre = conv(self.x, self.w[:, :r.cin] if r.op == "classbias" else self.w, self.b)
            if r.op == "classbias":
                cls = _class_index(self.OH, self.OW, self.cb_mode)
                pre = pre + self.cb[:, cls, :r.cout].permute(0, 3, 1, 2)
            XL.assert_on_lattice(pre, self.unit, r.name + " pre-activation")
            y = _act(pre, self.act)
            self.r1 = self.r2 = None
            if res:
                self.r1 = XL.draw(y.shape, QB if res != "fma" else 3, amp=64 if res != "fma" else 8, density=1.0, gen=g)
                if res == "fma":
                    self.r2 = XL.draw(y.shape, 2, amp=4, density=1.0, gen=g)
                y = y + self.r1 if res == "add" else (y - self.r1 if res == "sub" else y + self.r1 * self.r2)
            self.pre, self.ref = pre, y
            if r.epi == "bn":
                XL.assert_sq_sum_bound(pre, self.unit, (0, 2, 3), r.name)
                self.ref_stat = torch.stack([pre.sum((0, 2, 3)), (pre * pre).sum((0, 2, 3))])
            if r.epi == "sum":
                assert float(pre.abs().sum((2, 3)).max()) / self.unit < XL.FP32_EXACT, f"{r.name}: the per-sample sums break the fp32 bound"
                self.ref_stat = pre.sum((2, 3))
            self.sigmoid = self.act == "sigmoid"
            if self.sigmoid:                # no exact result: the sigmoid of the exact pre-activation, to 1 fp16 ulp
                self.tol = _fp16_ulp(self.ref)
            else:
                XL.assert_on_lattice(self.ref, self.unit * SLOPE, r.name)
                XL.assert_fp16_exact(self.ref, r.name)
        elif r.op == "dgrad":
            K = taps * r.cout
            dens = XL.density_for(K)
            self.w = XL.draw(wshape, QW, amp=2, density=dens, gen=g)
            self.dpre = XL.draw((r.N, r.cout, self.OH, self.OW), QX, amp=2, density=dens, gen=g)
            XL.assert_sum_bound(K, 2.0 ** (1 - QX), 2.0 ** (1 - QW), self.unit, r.name)
            xr = torch.zeros(r.N, r.cin, r.H, r.W, requires_grad=True)
            conv(xr, self.w).backward(self.dpre)
            ref = xr.grad.detach()
            XL.assert_on_lattice(ref, self.unit, r.name)
            self.acc, self.masked = "acc" in r.epi, "mask" in r.epi
            self.old = XL.draw(ref.shape, QB, amp=64, density=1.0, gen=g) if self.acc else None
            if self.acc:
                ref = ref + self.old
            self.below = XL.draw(ref.shape, 0, amp=1, density=1.0, gen=g) if self.masked else None
            if self.masked:
                ref = ref * torch.where(self.below > 0, torch.ones(()), torch.full((), SLOPE))
            self.ref = ref
            XL.assert_fp16_exact(self.ref, r.name)
        else:
            M = r.N * (r.H * r.W if r.tr else self.OH * self.OW)
            self.x = XL.draw((r.N, r.cin, r.H, r.W), QX, amp=2, density=0.5, gen=g)
            self.w = XL.draw(wshape, QW, amp=2, density=0.5, gen=g)
            self.dpre = XL.draw((r.N, r.cout, self.OH, self.OW), QW, amp=2, density=0.5, gen=g)
            XL.assert_sum_bound(M * (r.s * r.s if r.tr else 1), 2.0 ** (1 - QX), 2.0 ** (1 - QW), self.unit, r.name)
            wr = self.w.clone().requires_grad_(True)
            conv(self.x, wr).backward(self.dpre)
            self.ref = wr.grad.detach()
            XL.assert_on_lattice(self.ref, self.unit, r.name)
            XL.assert_fp32_exact(self.ref, r.name)

    def conv(self, eng):
        from csbsr_amd.engine import Conv
        r = self.row
        L = _L()
        params = {"l.weight": self.w.cuda(), "l.a": torch.tensor([SLOPE]).cuda()}
        bias = r.op in ("fwd", "classbias") and self.has_bias
        if bias:
            params["l.bias"] = self.b.cuda()
        act = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "prelu": L.ACT_PRELU,
               "sigmoid": L.ACT_SIGMOID}[self.act if r.op in ("fwd", "classbias") else "none"]
        return Conv(eng, "l", params, r.k, r.s, r.p, 1, transposed=r.tr, bias=bias, act=act, slope=SLOPE,
                    prelu="l.a" if act == L.ACT_PRELU else False, split=r.segs or None), params

    def _inputs(self, t, c0):
        r = self.row
        if r.segs and r.op != "classbias":
            return tuple(_fm(p, c0) for p in torch.split(t, list(r.segs), 1))
        return _fm(t, c0)

    def run(self, eng, conv, params, out_c0, in_c0):
        """one launch; returns (result on the CPU, guard object or None, stat or None)"""
        r = self.row
        L = _L()
        if r.op == "wgrad":
            orig = type(eng).workspace

            def poisoned(nfloat):
                ws = orig(eng, nfloat)
                ws.fill_(float("nan"))
                return ws
            eng.workspace = poisoned
            try:
                from csbsr_amd.engine import grad_acc
                grad_acc(conv.w).zero_()
                conv.bwd_weights(_fm(self.dpre, in_c0), self._inputs(self.x, in_c0))
                torch.cuda.synchronize()
            finally:
                del eng.workspace
            return params["l.weight"].gacc.cpu().clone(), None, None
        if r.op == "dgrad":
            gd = Guarded(r.N, r.H, r.W, r.cin, out_c0, self.old)
            conv.bwd_input(_fm(self.dpre, in_c0), out=gd.fm, accumulate=self.acc, in_hw=(r.H, r.W),
                           mask=(_fm(self.below), SLOPE) if self.masked else None)
            torch.cuda.synchronize()
            return _from_fm(gd.fm), gd, None
        kw = {}
        if self.res:
            kw = dict(res=_fm(self.r1), res_mode={"add": L.RES_ADD, "sub": L.RES_SUB, "fma": L.RES_FMA}[self.res])
            if self.res == "fma":
                kw["res2"] = _fm(self.r2)
        stat = None
        if r.epi in ("bn", "sum"):
            _poison_scratch()
            # (both kinds of sums ADD to the buffer -- csbsr_sum_partials' last level, BatchNorm.new_stat is zeroed -- so it starts at zero)
            stat = torch.zeros((2, pad8(r.cout)) if r.epi == "bn" else (r.N, pad8(r.cout)), device="cuda")
            kw.update(stat=stat, stat_mode=L.STAT_BN if r.epi == "bn" else L.STAT_SAMPLE_SUM)
        if r.epi == "sum":
            conv.fwd(self._inputs(self.x, in_c0), store=False, **kw)
            torch.cuda.synchronize()
            return None, None, stat[:, :r.cout].cpu()
        gd = Guarded(r.N, self.OH, self.OW, r.cout, out_c0)
        if r.op == "classbias":
            conv.fwd_classbias(self._inputs(self.x, in_c0), self.cb.cuda(), self.cb_mode, out=gd.fm)
        else:
            conv.fwd(self._inputs(self.x, in_c0), out=gd.fm, **kw)
        torch.cuda.synchronize()
        return _from_fm(gd.fm), gd, (None if stat is None else stat[:, :r.cout].cpu())

    def check(self, got, gd, stat, what):
        r = self.row
        if got is not None and getattr(self, "sigmoid", False):
            err = (got.double() - self.ref).abs()
            assert bool((err <= self.tol).all()), f"{r.name} {what}: {int((~(err <= self.tol)).sum())} values more than 1 fp16 ulp from the sigmoid"
        elif got is not None:
            assert torch.equal(got, self.ref), f"{r.name} {what}: {XL.mismatch(got, self.ref)}"
        if gd is not None:
            gd.check(f"{r.name} {what}")
        if stat is not None:
            assert torch.equal(stat, self.ref_stat), f"{r.name} {what} sums: {XL.mismatch(stat, self.ref_stat)}"


def run_row(row, check_kid=True, budgets=True):
    """every check of one row; returns the kernel ID the plain launch reached"""
    from csbsr_amd.engine import Engine
    L = _L()
    lib = L.load()
    case = Case(row)
    eng = Engine("cuda:0")
    try:
        _apply_modes(lib, eng, row.modes)
        conv, params = case.conv(eng)
        base = case.run(eng, conv, params, 0, None)
        kid = _kernel_id(lib, row.op)
        if check_kid:
            _check_kid(row, kid, "plain")
        case.check(*base, "plain")
        # operand bounds: input channels [128, 128 + cp) of a NaN-filled buffer, output at c0 = 128 and at c0 = 0 of wider buffers
        for out_c0, in_c0 in ((128, 128), (0, 64)):
            res = case.run(eng, conv, params, out_c0, in_c0)
            what = f"output at channel {out_c0}, input at channel {in_c0} (NaN around it)"
            if check_kid:
                _check_kid(row, _kernel_id(lib, row.op), what)
            case.check(*res, what)
        # tile walks: the persistent grids under CU budgets, bit-identical to the launch without one
        if budgets and row.budget:
            for ncu in BUDGETS["hr" if row.kid == 8 else "default"]:
                with Budget(ncu):
                    res = case.run(eng, conv, params, 0, None)
                what = f"CU budget {ncu}"
                if check_kid:
                    _check_kid(row, _kernel_id(lib, row.op), what)
                case.check(*res, what)
                for a, b in zip(res, base):
                    if torch.is_tensor(a):
                        assert torch.equal(a, b), f"{row.name} {what}: differs from the launch without a budget: {XL.mismatch(a, b)}"
        return kid
    finally:
        _restore_modes(lib)


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_conv_exact(row):
    run_row(row)
