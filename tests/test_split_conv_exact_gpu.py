"""Bit-exact parity of the split-fp16 (hi + lo) convolution paths on exact-lattice operands: the loop of tests/test_conv_exact_gpu.py for
split operands.

Each row of tests/split_conv_cases.py runs through the engine entry point it names (Conv.fwd / fwd_folded / fwd_const_1x1 with a split
input, Conv.bwd_input with hp_dgrad) on operands whose three products x_hi w_hi + x_lo w_hi + x_hi w_lo are whole multiples of one unit
and sum to less than 2^24 units in magnitude (tests/split_conv_cases.py proves it on the drawn operands), so the fp32 accumulator holds
the exact value in any summation order, every epilogue step is exact, and BOTH output planes -- hi = fp16(t), lo = fp16(t - hi) -- must
EQUAL the CPU reference.  A kernel that drops x_hi w_lo, reads the lo plane of the wrong 32-channel slice, forgets out_scale or rounds
the lo plane twice fails (tests/test_split_conv_cases_cpu.py: every such mutant of the reference changes the expected planes).  Per row:
  * the kernel ID and template instance the row's ``why`` claims, asserted after the launch;
  * the input as a whole [hi | lo] buffer of Engine.new(split=True) (FM.split_segs refuses slices), pad channels zero;
  * the output as channels [c0, c0 + coutp) of a wider split buffer (the slice form of PSPNet's concat buffer: the lo plane one buffer
    pitch further on), a canary bit pattern around both planes and in a guard row below every sample, both planes prefilled with NaN,
    their pad channels [cout, coutp) exactly zero afterwards;
  * BatchNorm rows: the reduction scratch refilled with NaN first, the sums exact (sums of squares below 2^24 units^2);
  * conv_x3n rows: again under CU budgets of 1, 3 and 7, bit-identical.
Measured on an MI355X: the MFMA's fp32 accumulation is exact over this span -- the largest sum of |terms| of a row is 2^19.5 (1x1 rows)
to 2^21.35 units, under proven bounds of 2^20.1 to 2^22.26 units (every row prints its bound as ``span``; the plain rows of
tests/test_conv_exact_gpu.py span about 2^12) -- in the fused stages, the two- and three-block forms, conv_x3n and the register-staged
kernels alike, and no lo plane differed anywhere, so nothing had to shrink."""
import pytest
import torch

import exact_lattice as XL
import split_conv_cases as SC
from conv_exact_cases import BUDGETS
from split_conv_cases import SLOPE, SPLIT_ROWS
from test_conv_exact_gpu import CANARY, Budget, Guarded, _apply_modes, _check_kid, _fm, _poison_scratch, _restore_modes, pad8

pytestmark = pytest.mark.gpu


def _L():
    from csbsr_amd import _lib as L
    return L


def _lo_view(fm):
    """the lo plane of a split FM: ``lo`` elements further on in the same allocation, same strides (csbsr_amd/engine.py FM)"""
    return fm.t.as_strided(fm.t.shape, fm.t.stride(), fm.t.storage_offset() + fm.lo)


def _nhwc16(x):
    return x.permute(0, 2, 3, 1).half().cuda()


def _split_fm(eng, hi, lo):
    """NCHW fp32 planes (fp16-exact) -> a whole [hi | lo] split map; pad channels zero"""
    N, c, H, W = hi.shape
    fm = eng.new(N, H, W, c, zero=True, split=True)
    fm.t[..., :c] = _nhwc16(hi)
    _lo_view(fm)[..., :c] = _nhwc16(lo)
    assert fm.lo == fm.cp
    return fm


class GuardedSplit:
    """a split output FM as channels [c0, c0 + coutp) of a wider split buffer (plane pitch Cw, the lo plane Cw elements after the hi
    plane) with a guard row below every sample; everything outside the two slices holds CANARY, the slices NaN"""

    def __init__(self, N, OH, OW, c, c0):
        from csbsr_amd.engine import FM
        cp = pad8(c)
        Cw = c0 + cp + 64
        self.big = torch.empty(N, OH + 1, OW, 2 * Cw, dtype=torch.float16, device="cuda")
        self.big.view(torch.int16).fill_(CANARY)
        self.region = torch.zeros(self.big.shape, dtype=torch.bool)
        for base in (c0, Cw + c0):
            self.big[:, :OH, :, base:base + cp].fill_(float("nan"))
            self.region[:, :OH, :, base:base + cp] = True
        self.fm = FM(self.big[:, :OH, :, c0:c0 + cp], c, lo=Cw)
        self.c, self.cp = c, cp

    def planes(self):
        """(hi, lo) as NCHW fp16 on the CPU"""
        return tuple(t[..., :self.c].cpu().permute(0, 3, 1, 2) for t in (self.fm.t, _lo_view(self.fm)))

    def check(self, what):
        g = self.big.view(torch.int16).cpu()
        bad = (g != CANARY) & ~self.region
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} guard elements overwritten, first at {tuple(torch.nonzero(bad)[0].tolist())}"
        for name, t in (("hi", self.fm.t), ("lo", _lo_view(self.fm))):
            pads = t[..., self.c:].float().cpu()
            assert bool((pads == 0).all()), f"{what}: pad channels [{self.c}, {self.cp}) of the {name} plane not zero: {XL.mismatch(pads, torch.zeros_like(pads))}"


def _layer(eng, row, c):
    """the Conv of a row: master weights = the drawn scaled weights / WSCALE (and the plain constant-segment weights)"""
    from csbsr_amd.engine import Conv
    L = _L()
    r = row
    assert Conv.WSCALE == SC.WSCALE
    if r.op == "folded":
        w, split = torch.cat([c.w_split, c.w_const], 1), r.segs
    elif r.op == "const":
        w, split = torch.cat([c.w_const, c.w_split], 1), r.segs
    else:
        w, split = c.w_split, (r.segs or None)
    params = {"l.weight": w.cuda(), "l.a": torch.tensor([SLOPE]).cuda()}
    bias = r.op != "dgrad" and c.b is not None
    if bias:
        params["l.bias"] = c.b.cuda()
    act = L.ACT_NONE if r.op == "dgrad" else {"none": L.ACT_NONE, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "prelu": L.ACT_PRELU}[c.act]
    conv = Conv(eng, "l", params, r.k, r.s, r.p, r.dil, bias=bias, act=act, slope=SLOPE, prelu="l.a" if act == L.ACT_PRELU else False, split=split)
    conv.fwd_blocks = r.blocks
    conv.hp_dgrad = r.op == "dgrad"
    return conv


def _launch(eng, conv, row, c, out_c0):
    """one launch; returns (planes or gradient on the CPU, guard object, BatchNorm sums or None)"""
    L = _L()
    r = row
    if r.op == "dgrad":
        gd = Guarded(r.N, r.H, r.W, c.cseg, out_c0, c.old)
        conv.bwd_input(_fm(c.dpre, 128 if out_c0 else None), seg=r.seg, out=gd.fm, accumulate=c.old is not None, in_hw=(r.H, r.W))
        torch.cuda.synchronize()
        return (gd.fm.t[..., :c.cseg].cpu().permute(0, 3, 1, 2),), gd, None
    x = _split_fm(eng, c.x_hi, c.x_lo)
    gd = GuardedSplit(r.N, c.OH, c.OW, r.cout, out_c0)
    kw, stat = {}, None
    if c.res:
        kw = dict(res=_split_fm(eng, *c.r1), res_mode={"add": L.RES_ADD, "sub": L.RES_SUB, "fma": L.RES_FMA}[c.res])
        if c.res == "fma":
            kw["res2"] = _split_fm(eng, *c.r2)
    if c.bn:
        _poison_scratch()
        stat = torch.zeros(2, pad8(r.cout), device="cuda")
        kw.update(stat=stat, stat_mode=L.STAT_BN)
    if r.op == "folded":
        from fused_exact_cases import border_tap_mask
        conv.fwd_folded(x, c.kvec.cuda(), border_tap_mask().cuda(), out=gd.fm)
    elif r.op == "const":
        conv.fwd_const_1x1(c.cvec.cuda(), x, out=gd.fm)
    else:
        conv.fwd(x, out=gd.fm, **kw)
    torch.cuda.synchronize()
    return gd.planes(), gd, (None if stat is None else stat[:, :r.cout].cpu())


def _check(row, c, got, gd, stat, what):
    if row.op == "dgrad":
        assert torch.equal(got[0], c.ref), f"{row.name} {what}: {XL.mismatch(got[0], c.ref)}"
    else:
        assert torch.equal(got[0], c.hi), f"{row.name} {what}, hi plane: {XL.mismatch(got[0], c.hi)}"
        assert torch.equal(got[1], c.lo), f"{row.name} {what}, lo plane: {XL.mismatch(got[1], c.lo)}"
    gd.check(f"{row.name} {what}")
    if stat is not None:
        assert torch.equal(stat, c.stat), f"{row.name} {what}, BatchNorm sums: {XL.mismatch(stat, c.stat)}"


def run_row(row, check_kid=True, budgets=True):
    """every check of one row; returns the kernel ID the first launch reached"""
    from csbsr_amd.engine import Engine
    lib = _L().load()
    c = SC.build(row)
    print(f"{row.name}: span 2^{SC.span_log2(c):.2f} units")
    eng = Engine("cuda:0")
    fused0 = eng.split_fused
    try:
        _apply_modes(lib, eng, row.modes)
        eng.split_fused = row.fused
        conv = _layer(eng, row, c)
        first, base = None, None
        for out_c0 in row.out_c0:
            got, gd, stat = _launch(eng, conv, row, c, out_c0)
            kid = int(lib.csbsr_debug_last_conv_kernel())
            what = f"output at channel {out_c0}"
            if check_kid:
                _check_kid(row, kid, what)
            _check(row, c, got, gd, stat, what)
            if first is None:
                first, base = kid, (got, stat)
        if budgets and row.budget:          # the persistent grid of conv_x3n under CU budgets: bit-identical to the launch without one
            for ncu in BUDGETS["default"]:
                with Budget(ncu):
                    got, gd, stat = _launch(eng, conv, row, c, 0)
                what = f"CU budget {ncu}"
                if check_kid:
                    _check_kid(row, int(lib.csbsr_debug_last_conv_kernel()), what)
                _check(row, c, got, gd, stat, what)
                for a, b in zip(got + (stat,), base[0] + (base[1],)):
                    if torch.is_tensor(a):
                        assert torch.equal(a, b), f"{row.name} {what}: differs from the launch without a budget: {XL.mismatch(a, b)}"
        return first
    finally:
        _restore_modes(lib)
        eng.split_fused = fused0


@pytest.mark.parametrize("row", SPLIT_ROWS, ids=[r.name for r in SPLIT_ROWS])
def test_split_conv_exact(row):
    run_row(row)


def test_exact_weights_need_no_rounding_compensation():
    """Conv._wq / Conv._dc_bias on fp16-exact master weights with dc_comp: the tap-sum-preserving rounding returns the weights bit for bit,
    its tap-sum table is zero, and the per-sample bias rows are the bias (for a plain and for a split input)"""
    from csbsr_amd.engine import Conv, Engine
    eng = Engine("cuda:0")
    assert eng.tapsum and eng.dc_comp
    g = torch.Generator().manual_seed(11)
    N, cin, cout, H, W = 2, 128, 100, 16, 16
    w = XL.draw((cout, cin, 3, 3), 3, amp=2, density=0.5, gen=g) / SC.WSCALE          # fp16-exact, normal
    XL.assert_fp16_exact(w, "weights")
    XL.assert_fp16_normal(w, "weights")
    b = XL.draw((cout,), SC.QB, amp=64, density=1.0, gen=g)
    conv = Conv(eng, "l", {"l.weight": w.cuda(), "l.bias": b.cuda()}, 3, 1, 1, 1, bias=True)
    conv.dc_comp = True
    q = conv._wq()
    torch.cuda.synchronize()
    assert q is not conv.w, "dc_comp: _wq() must return the rounded copy"
    assert torch.equal(q.cpu().view(torch.int32), w.view(torch.int32)), f"_wq() changed fp16-exact weights: {XL.mismatch(q.cpu(), w)}"
    S = conv._packed["dc_table"].cpu()
    assert tuple(S.shape) == (cout, cin) and bool((S == 0).all()), f"tap sums of a zero residual: {XL.mismatch(S, torch.zeros_like(S))}"
    x_hi, x_lo = XL.draw_split_planes((N, cin, H, W), 0, density=0.5, gen=g)
    for name, fm in (("plain", _fm(x_hi)), ("split", _split_fm(eng, x_hi, x_lo))):
        rows = conv._dc_bias((fm,))
        torch.cuda.synchronize()
        assert tuple(rows.shape) == (N, cout)
        assert torch.equal(rows.cpu(), b[None, :].expand(N, cout)), f"{name} input: bias rows: {XL.mismatch(rows.cpu(), b[None, :].expand(N, cout))}"
